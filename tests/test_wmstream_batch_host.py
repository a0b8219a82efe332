"""CPU: the host side of the batched watermarked stream (DESIGN.md Part I.29). The sibling of `layout.check_stream_batch`, the row-op
tables `BatchWMDecodeStream` builds (`rows_front_zero`, `rows_right_edge` / `rows_left_edge`, `rows_core_copy`) applied to numpy arrays
by a model of `ssrhip_stream_rows`, the chain's window rule, and the C entry's contract errors, which return before any HIP call."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec import wmencodec as WM
from ssr_speech_amd.engine import MAX_ROWS

K = 4
B, PROMPTS, ENDS, FRONT = 3, (4, 9, 6), (21, 33, 17), 3           # ENDS: the row behind each item's last frame
PLAN = WM.batch_align_plan(PROMPTS, FRONT)                        # off = (8, 3, 6), E = 12
ROWS = 40


def apply_row_ops(ops, dst: np.ndarray, src: np.ndarray = None):
    """What one `ssrhip_stream_rows` launch does with a table whose offsets count floats of flat `dst` / `src` (None: the same array),
    in place. Refuses what the launcher refuses: an op's dst range may meet no other op's dst range and no op's src range."""
    src = dst if src is None else src
    same = src is dst
    snap = src.copy()
    d_idx, s_idx = [], []
    for op in ops:
        assert op.rows >= 0 and op.width >= 0 and op.mode in (0, 1)
        d = np.array([op.dst + r * op.dst_ld + c for r in range(op.rows) for c in range(op.width)], dtype=np.int64)
        s = np.array([op.src + r * op.src_ld + c for r in range(op.rows) for c in range(op.width)], dtype=np.int64) if op.mode else d[:0]
        assert d.size == 0 or (d.min() >= 0 and d.max() < dst.size and len(set(d.tolist())) == d.size)
        assert s.size == 0 or (s.min() >= 0 and s.max() < src.size)
        d_idx.append(d)
        s_idx.append(s)
    for i, d in enumerate(d_idx):
        for j in range(len(ops)):
            assert j == i or not np.intersect1d(d, d_idx[j]).size, f"ops {i} and {j} overlap in dst"
            assert not (same and np.intersect1d(d, s_idx[j]).size), f"op {i} writes what op {j} reads"
    for op, d, s in zip(ops, d_idx, s_idx):
        dst[d] = snap[s] if op.mode else 0.0


def _items(C_, seed):
    return np.random.default_rng(seed).standard_normal((B, ROWS, C_)).astype(np.float32)


# ----------------------------------------------------------------------------------------------- the sibling of check_stream_batch
def test_check_wmstream_batch_accepts_tts_and_names_the_watermarked_call(monkeypatch):
    assert LY.check_wmstream_batch([9, 12], [np.array([[9, 9]]), np.array([[7, 12]])], 2, MAX_ROWS) == [9, 7]
    with pytest.raises(ValueError, match=r"watermarked stream.*speech edit.*render_many\(use_watermark=True\)"):
        LY.check_wmstream_batch([9], [np.array([[2, 5]])], 1, MAX_ROWS)                    # the span does not end the utterance
    with pytest.raises(ValueError, match=r"one generated span, got 2.*render_many\(use_watermark=True\)"):
        LY.check_wmstream_batch([9], [np.array([[1, 3], [5, 9]])], 1, MAX_ROWS)
    with pytest.raises(ValueError, match=r"17 utterances x 2 rows do not fit.*render_many\(use_watermark=True\)"):
        LY.check_wmstream_batch([9] * 17, [np.array([[9, 9]])] * 17, 2, MAX_ROWS)
    with pytest.raises(ValueError):
        LY.check_wmstream_batch([], [], 1, MAX_ROWS)
    # the un-watermarked check keeps its refusal
    with pytest.raises(ValueError, match="render_many"):
        LY.check_stream_batch([9], [np.array([[9, 9]])], 2, MAX_ROWS, use_watermark=True)

    # the model's entry and the public generators: refusals before any library call
    from ssr_speech_amd.models.ssr import SSR_Speech
    from ssr_speech_amd import inference_scale as S

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    m = SSR_Speech(W.lm_args_tiny())
    monkeypatch.setattr(m, "_get_engine", boom)
    utt = lambda T=9, mi=None: {"x": torch.zeros(1, 5, dtype=torch.long), "y": torch.zeros(1, T, K, dtype=torch.long),      # noqa: E731
                                "mask_interval": torch.tensor([mi if mi is not None else [[T, T]]], dtype=torch.long)}
    with pytest.raises(ValueError, match="use_watermark=True"):
        m.inference_batch_wmstream([utt(), utt(mi=[[2, 5]])])
    with pytest.raises(ValueError, match="use_watermark=True"):
        m.inference_batch_wmstream([utt()] * (MAX_ROWS // 2 + 1), aug_text=True)
    it = m.inference_batch_wmstream([utt()] * (MAX_ROWS // 2), aug_text=True)
    assert it.results is None and it.polls == 0 and it.prompt_lens == [9] * (MAX_ROWS // 2)
    gen = S.inference_samples_wmstream(None, None, None, None, None, None, "", "", None, 1.5, 1, True, False, True, False, "cpu", {}, seeds=[1, 2])
    with pytest.raises(ValueError, match=r"inference_samples\(use_watermark=True\)"):
        next(gen)
    b = inspect.signature(SSR_Speech.inference_batch_stream).parameters
    w = inspect.signature(SSR_Speech.inference_batch_wmstream).parameters
    assert list(w) == [p for p in b if p != "return_logprobs"] and all(w[p].default == b[p].default for p in w if p != "self")
    for twin, mine in ((S.inference_batch_stream, S.inference_batch_wmstream), (S.inference_samples_stream, S.inference_samples_wmstream)):
        assert list(inspect.signature(twin).parameters) == list(inspect.signature(mine).parameters)
    from ssr_speech_amd.data.tokenizer import AudioTokenizer
    for cls in (WM.WMEncodecModel, AudioTokenizer):
        assert list(inspect.signature(cls.wmdecode_stream_batch).parameters)[1:] == ["prompt_lens", "max_new_frames", "max_window"]
        assert inspect.signature(cls.wmdecode_stream_batch).parameters["max_window"].default == 16


# ----------------------------------------------------------------------------------------------- the row-op tables
def test_front_zero_rows():
    """A batched call over the rows [a, b): the rows in front of each item's first frame are zeroed, nothing else moves."""
    off = PLAN["off"]
    assert off == [8, 3, 6] and PLAN["E"] == 12
    for C_ in (4, 6):
        x = _items(C_, 1)
        got = x.copy()
        for a, b in ((0, 5), (5, 7), (7, 12), (12, 20)):
            ops = WM.rows_front_zero(off, a, b, ROWS, C_)
            assert len(ops) == sum(a < min(b, o) for o in off)
            apply_row_ops(ops, got.reshape(-1))
        for u in range(B):
            assert not got[u, :off[u]].any() and np.array_equal(got[u, off[u]:], x[u, off[u]:])
    assert WM.rows_front_zero(off, 8, 20, ROWS, 4) == []                       # behind every item's first frame: no op, no launch


@pytest.mark.parametrize("pl,pr", [(3, 3), (2, 1)])
def test_right_and_left_edges_zero_and_reflect(pl, pr):
    """An ended item's padding behind its end, and the reflected rows in front of an item's first frame: the rows a batch-1 pass pads
    the item's own rows [off, end) with."""
    off, C_ = PLAN["off"], 4
    for reflect in (False, True):
        x = _items(C_, 2)
        got = x.copy()
        ops = [WM.rows_right_edge(u, ENDS[u], pr, reflect, ROWS, C_) for u in range(B)]
        if reflect:
            ops += [WM.rows_left_edge(u, off[u], pl, ROWS, C_) for u in range(B)]
        assert all(op.mode == int(reflect) and op.rows in (pl, pr) for op in ops) and all(op.src_ld == -C_ for op in ops if reflect)
        apply_row_ops(ops, got.reshape(-1))
        for u in range(B):
            own = x[u, off[u]: ENDS[u]]
            want = np.pad(own, ((pl, pr), (0, 0)), mode="reflect" if reflect else "constant")
            lo = off[u] - pl if reflect else off[u]                            # (constant: the rows in front are the producer's zeros)
            assert np.array_equal(got[u, lo: ENDS[u] + pr], want[(0 if reflect else pl):]), (u, reflect)
            assert np.array_equal(got[u, :lo], x[u, :lo]) and np.array_equal(got[u, ENDS[u] + pr:], x[u, ENDS[u] + pr:])


@pytest.mark.parametrize("rep,C_,pad", [(1, 8, 0), (40, 2, 1), (8, 3, 1)])
def test_tap_core_copies(rep, C_, pad):
    """A window [lo, hi) with the core [c0, c1): the core's rows of every member go from the window's buffer (a halo of `pad` rows in
    front) into the whole-utterance buffer, all members in one op when they sit in their own slots, else one op each."""
    c0, c1, lo, hi = 12, 28, 10, 30
    g = np.random.default_rng(3)
    win = g.standard_normal((B, pad + (hi - lo) * rep + pad, C_)).astype(np.float32)
    one = g.standard_normal((1,) + win.shape[1:]).astype(np.float32)
    for pairs, src in (([(0, 0), (1, 1), (2, 2)], win), ([(0, 0), (2, 2)], win), ([(1, 1), (2, 2)], win), ([(1, 0)], one)):
        whole = g.standard_normal((B, ROWS * rep, C_)).astype(np.float32)
        got = whole.copy()
        ops = WM.rows_core_copy(pairs, c0, c1, lo, rep, C_, ROWS * rep * C_, src.shape[1] * C_, pad)
        assert len(ops) == (1 if pairs == [(i, i) for i in range(len(pairs))] else len(pairs))
        apply_row_ops(ops, got.reshape(-1), src.reshape(-1))
        for u in range(B):
            slot = dict(pairs).get(u)
            if slot is None:
                assert np.array_equal(got[u], whole[u])
                continue
            assert np.array_equal(got[u, c0 * rep: c1 * rep], src[slot, pad + (c0 - lo) * rep: pad + (c1 - lo) * rep])
            assert np.array_equal(got[u, :c0 * rep], whole[u, :c0 * rep]) and np.array_equal(got[u, c1 * rep:], whole[u, c1 * rep:])


def test_the_model_refuses_overlapping_tables():
    x = np.zeros(64, dtype=np.float32)
    with pytest.raises(AssertionError, match="overlap in dst"):
        apply_row_ops([WM.RowOp(0, 0, 2, 4, 4, 0, 0), WM.RowOp(4, 0, 1, 4, 4, 0, 0)], x)
    with pytest.raises(AssertionError, match="reads"):
        apply_row_ops([WM.RowOp(0, 2, 1, 4, 4, 4, 1)], x)


def test_chain_windows_of_a_short_prompt_and_of_an_ended_item():
    """`chain_window_item` with margins (2, 2): a core in front of the item's first frame is skipped, a window that would reach in front
    of it is cut there, a live item stops two rows short of its last frame, an ended one runs to it."""
    m = (2, 2)
    assert WM.chain_window_item(3, 3, 12, False, m, 16) == (3, 10, 3, 12)              # the longest prompt: its first row is a true edge
    assert WM.chain_window_item(11, 3, 12, False, m, 16) == ("skip", 10)               # a 1-frame prompt: nothing of it in [3, 10)
    assert WM.chain_window_item(11, 10, 28, False, m, 16) == (11, 26, 11, 28)          # cut at its first frame
    assert WM.chain_window_item(3, 10, 28, False, m, 16) == (10, 26, 8, 28)
    assert WM.chain_window_item(9, 10, 28, False, m, 16) == (10, 26, 9, 28)            # the margin reaches in front of the item: cut
    assert WM.chain_window_item(3, 26, 28, False, m, 16) is None
    assert WM.chain_window_item(3, 26, 28, True, m, 16) == (26, 28, 24, 28)            # ended: to its end, a true edge
    assert WM.chain_window_item(3, 10, 60, True, m, 16) == (10, 26, 8, 28)
    wins = [WM.chain_window_item(o, 10, 28, False, m, 16) for o in (3, 11, 9, 5)]
    assert WM.batch_window_groups(wins) == ((10, 26, 8, 28), [0, 3], [1, 2])


# ----------------------------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _table(*ops):
    """ops: (dst, src, rows, width, dst_ld, src_ld, mode) with addresses that are never dereferenced"""
    t = (_lib.RowsOp * max(len(ops), 1))()
    for r, op in zip(t, ops):
        r.dst, r.src, r.rows, r.width, r.dst_ld, r.src_ld, r.mode = op
    return t


def test_symbol_and_sizeof_are_present(L):
    assert "ssrhip_stream_rows" in [n for n, _, _ in _lib.SYMBOLS] and "ssrhip_stream_rows_sizeof" in [n for n, _, _ in _lib.SYMBOLS]
    assert L.ssrhip_stream_rows_sizeof() == C.sizeof(_lib.RowsOp) == 48 and _lib.STREAM_ROWS_MAX_OPS == 64
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssrhip.h")).read()
    assert "#define SSRHIP_STREAM_ROWS_MAX_OPS 64" in hdr and "#define SSRHIP_VERSION 107" in hdr
    assert L.ssrhip_version() == 107 == _lib.ABI_VERSION and L.ssrhip_sizeof(16) == -1        # additions only: no new index either


def test_stream_rows_contract_errors_need_no_gpu(L):
    call = lambda t, n, dev=4096: L.ssrhip_stream_rows(C.addressof(t), dev, n, None)        # noqa: E731
    err = lambda: L.ssrhip_last_error()                                                     # noqa: E731
    ok = (1 << 20, 2 << 20, 3, 8, 8, 8, 1)
    big = (_lib.RowsOp * 65)()
    assert call(big, 65) < 0 and b"65 ops" in err()
    assert call(big, -1) < 0
    assert L.ssrhip_stream_rows(None, 4096, 1, None) < 0 and b"null" in err()
    assert call(_table(ok), 1, dev=None) < 0 and b"null" in err()
    assert call(_table((1 << 20, 2 << 20, -1, 8, 8, 8, 1)), 1) < 0 and b"negative" in err()
    assert call(_table((1 << 20, 2 << 20, 3, -8, 8, 8, 1)), 1) < 0 and b"negative" in err()
    assert call(_table((1 << 20, 2 << 20, 3, 8, 8, 8, 2)), 1) < 0 and b"mode 2" in err()
    assert call(_table((0, 2 << 20, 3, 8, 8, 8, 1)), 1) < 0 and b"null pointer" in err()
    assert call(_table((1 << 20, 0, 3, 8, 8, 8, 1)), 1) < 0 and b"null pointer" in err()
    assert call(_table((1 << 20, 2 << 20, 3, 8, 4, 8, 1)), 1) < 0 and b"apart" in err()       # rows of 8 floats 4 apart: they overlap
    # overlapping dst ranges: the second op starts inside the first one's last row; touching ranges are fine
    assert call(_table(ok, ((1 << 20) + 4 * 20, 2 << 20, 1, 8, 8, 8, 0)), 2) < 0 and b"ops 0 and 1 overlap in dst" in err()
    # a dst range that meets a src range: another op's, and the op's own (a reflect whose source runs into its destination)
    assert call(_table(ok, (3 << 20, (1 << 20) + 4 * 8, 1, 8, 8, 8, 1)), 2) < 0 and b"op 0 writes what op 1 reads" in err()
    assert call(_table((1 << 20, (1 << 20) + 4 * 8, 2, 8, 8, -8, 1)), 1) < 0 and b"op 0 writes what op 0 reads" in err()
    # an empty table, and a table of empty ops (whatever their other fields say): no error and no launch — with no GPU a launch would fail
    assert call(_table(), 0) == 0 and L.ssrhip_stream_rows(None, None, 0, None) == 0
    assert call(_table((0, 0, 0, 8, 8, 8, 1), (1 << 20, 0, 5, 0, 0, 0, 1), (1 << 20, 1 << 20, 0, 0, 8, 8, 0)), 3) == 0
