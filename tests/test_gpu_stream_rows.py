"""GPU: `ssrhip_stream_rows` (csrc/stream_rows.hip, DESIGN.md Part I.29) against its numpy model
(tests/test_wmstream_batch_host.py `apply_row_ops`) on whole poisoned buffers: copies and zeros only, so every comparison is
`torch.equal`. Widths on both sides of the 16-byte path, misaligned rows, a source walked backwards, mode 0, empty ops among live ones,
1 op and 64 ops, and a table of empty ops."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd.codec.wmencodec import RowOp
from test_wmstream_batch_host import apply_row_ops

pytestmark = pytest.mark.gpu
POISON = -12345.0


def _arenas(n_dst, n_src, seed):
    """(dst poisoned, src random) as flat CPU arrays; their device copies are made per launch"""
    g = np.random.default_rng(seed)
    return np.full(n_dst, POISON, dtype=np.float32), g.standard_normal(n_src).astype(np.float32)


def _launch(ops, dst: np.ndarray, src: np.ndarray):
    """One `ssrhip_stream_rows` call for `ops` (offsets in floats of dst / src) -> (rc, dst after the call, on the CPU)"""
    L = _lib.lib()
    d, s = torch.from_numpy(dst).cuda(), torch.from_numpy(src).cuda()
    t = (_lib.RowsOp * max(len(ops), 1))()
    for r, op in zip(t, ops):
        r.dst, r.src = d.data_ptr() + 4 * op.dst, s.data_ptr() + 4 * op.src
        r.dst_ld, r.src_ld, r.rows, r.width, r.mode = op.dst_ld, op.src_ld, op.rows, op.width, op.mode
    dev = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
    rc = L.ssrhip_stream_rows(C.addressof(t), dev.data_ptr(), len(ops), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), torch.from_numpy(src)), "the source was written"
    return rc, d.cpu()


def _check(ops, n_dst, n_src, seed=0):
    dst, src = _arenas(n_dst, n_src, seed)
    want = dst.copy()
    apply_row_ops(ops, want, src)
    rc, got = _launch(ops, dst, src)
    assert rc == 0, _lib.lib().ssrhip_last_error()
    assert torch.equal(got, torch.from_numpy(want))
    return want


@pytest.mark.parametrize("width", [1, 3, 4, 128, 130])
def test_copy_and_zero_rows_of_every_width(width):
    """7 rows of `width` floats, copied and zeroed, with aligned starts and steps (the 16-byte path where width % 4 == 0) and with a row
    step of width + 1 (rows that leave the 16-byte grid: the 4-byte path), in one table."""
    ld = (width + 3) // 4 * 4 + 4
    ops, at = [], 8
    for dst_ld, src_ld, mode in ((ld, ld, 1), (ld, 0, 0), (width + 1, width + 1, 1), (width + 1, 0, 0), (ld, 0, 1)):     # (src_ld 0: one row, 7 times)
        ops.append(RowOp(at, 4 + 3 * len(ops), 7, width, dst_ld, src_ld, mode))
        at += (7 * max(dst_ld, width) + 7) // 4 * 4 + 8
    want = _check(ops, at, 8 * 140 + 64, seed=width)
    assert (want == POISON).sum() > 0 and (want == 0.0).sum() == 2 * 7 * width


def test_misaligned_pointers_take_the_scalar_path():
    """width 8 and steps of 8, but a destination / a source 4 bytes off the 16-byte grid"""
    ops = [RowOp(1, 0, 5, 8, 8, 8, 1), RowOp(64, 3, 5, 8, 8, 8, 1), RowOp(129, 0, 5, 8, 8, 0, 0), RowOp(192, 64, 5, 8, 12, 9, 1)]
    _check(ops, 320, 160)


@pytest.mark.parametrize("width", [4, 6])
def test_a_negative_source_step_reflects(width):
    """row r of the destination <- row -r of the source: the reflected edge of a [rows][width] buffer, as `rows_right_edge` writes it"""
    x = np.random.default_rng(9).standard_normal((12, width)).astype(np.float32)
    d = torch.from_numpy(np.concatenate([x, np.full((3, width), POISON, dtype=np.float32)]).reshape(-1).copy()).cuda()
    t = (_lib.RowsOp * 1)()
    t[0].dst, t[0].src = d.data_ptr() + 4 * 12 * width, d.data_ptr() + 4 * 10 * width
    t[0].dst_ld, t[0].src_ld, t[0].rows, t[0].width, t[0].mode = width, -width, 3, width, 1
    dev = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
    assert _lib.lib().ssrhip_stream_rows(C.addressof(t), dev.data_ptr(), 1, _lib.stream_ptr()) == 0
    want = np.pad(x, ((0, 3), (0, 0)), mode="reflect")
    assert torch.equal(d.cpu(), torch.from_numpy(want.reshape(-1)))
    # ... and through the model, source and destination apart, both steps negative
    _check([RowOp(40, 50, 4, width, -8, -8, 1), RowOp(64, 20, 3, width, 8, -width, 1)], 96, 64)


@pytest.mark.parametrize("n_ops", [1, 64])
def test_one_op_and_a_full_table_with_empty_ops_mixed_in(n_ops):
    """`n_ops` ops of different shapes — every third one empty (no rows, or no width, with pointers that must not matter) — in ONE launch;
    the longest op alone spans several workgroups."""
    g = np.random.default_rng(n_ops)
    ops, at = [], 0
    for i in range(n_ops):
        rows, width = int(g.integers(1, 9)), int(g.choice([1, 2, 4, 5, 8, 12, 64]))
        if i == 0:
            rows, width = 300, 36                                               # 2700 units of 4 floats: 11 workgroups
        if n_ops > 1 and i % 3 == 1:
            rows, width = (0, width) if i % 2 else (rows, 0)
        ld = width + int(g.choice([0, 0, 3, 4]))
        ops.append(RowOp(at, int(g.integers(0, 64)), rows, width, ld, int(g.choice([0, width, width + 4])), int(i % 4 != 2)))
        at += (rows * max(ld, 1) + 3) // 4 * 4 + 4 * int(g.integers(0, 3))
    assert n_ops == 1 or (sum(op.rows == 0 or op.width == 0 for op in ops) > 10 and {op.mode for op in ops} == {0, 1})
    _check(ops, at + 16, 64 + 300 * 40 + 64, seed=n_ops)


def test_a_table_of_empty_ops_launches_nothing():
    """rc 0 and an untouched buffer (the CPU suite shows the same where a launch would fail: tests/test_wmstream_batch_host.py)"""
    L = _lib.lib()
    d = torch.full((256,), POISON, device="cuda")
    t = (_lib.RowsOp * 3)()
    for r, (rows, width) in zip(t, ((0, 8), (4, 0), (0, 0))):
        r.dst, r.src, r.rows, r.width, r.dst_ld, r.src_ld, r.mode = d.data_ptr(), d.data_ptr(), rows, width, 8, 8, 1
    dev = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
    assert L.ssrhip_stream_rows(C.addressof(t), dev.data_ptr(), 3, _lib.stream_ptr()) == 0
    assert L.ssrhip_stream_rows(None, None, 0, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.full((256,), POISON))
