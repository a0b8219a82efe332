"""GPU: every kernel and dispatch branch of csrc/codec.hip called through the C-ABI against a plain float64 reference of the same
operation (tests/helpers_codec.py, pinned to oracle/codec.py by tests/test_codec_kernel_refs.py). The end-to-end codec tests reach
only the branch the product's two configurations happen to take; here each launcher is driven through all of its template
instantiations, its tile edges, batch strides with slack (pre-filled with a sentinel that must survive) and its refusals.

Bars: the copying kernels (padding, RVQ dequantiser) and the RVQ codes are exact; the arithmetic kernels meet rtol = atol = 2e-5 on
O(1) data with 1/sqrt(K)-scaled weights (the bar of the residual-block and split-LSTM kernel tests: fp32 everywhere, differences
come from summation order only). Set SSRHIP_CODEC_TEST_REPORT to a path to get the largest observed errors and the RVQ kept shares
as JSON."""
import ctypes as C
import functools
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
import helpers_codec as H

pytestmark = pytest.mark.gpu

SENT = -777.25                      # exactly representable; no kernel here can produce it from O(1) data by accident
TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_report = {"max_abs_err": {}, "rvq_kept_share": {}}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _lib.lib()
    path = os.environ.get("SSRHIP_CODEC_TEST_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(_report, sort_keys=True) + "\n")


def dev(t):
    return t.to("cuda").contiguous()


def sync():
    torch.cuda.synchronize()


def _close(family, got, want):
    """rtol = atol = 2e-5 against float64, and the largest absolute error of the family for the report."""
    err = float((got.double() - want).abs().max())
    _report["max_abs_err"][family] = max(_report["max_abs_err"].get(family, 0.0), err)
    print(f"{family}: max |kernel - fp64| = {err:.3g}")
    torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL)


def _child(env, k_expr, n_expected):
    """Run tests of THIS module once more in a fresh child process (a switch the library reads once per process), and count them."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", k_expr],
                         env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-2000:]
    n_passed = int(re.search(r"(\d+) passed", out.stdout).group(1))
    assert n_passed == n_expected, f"`-k {k_expr}` ran {n_passed} tests, not {n_expected}: {out.stdout[-500:]}"


# ------------------------------------------------------------------------------------------ ssrhip_conv_cin1
def _conv_cin1_case(L, k, stride, Cout, T_out, family, B=3):
    g = torch.Generator().manual_seed(100000 * k + 10000 * stride + 7 * Cout + T_out)
    n_in = (T_out - 1) * stride + k
    xs, os_ = n_in + 5, (T_out + 2) * Cout + 8                       # slack behind every item, on both sides
    x = torch.randn(B, xs, generator=g)
    w = torch.randn(Cout, k, generator=g) / math.sqrt(k)
    bias = torch.randn(Cout, generator=g) * 0.1
    dx, dw, db = dev(x), dev(w), dev(bias)
    out = torch.full((B, os_), SENT, device="cuda")
    _lib.check(L.ssrhip_conv_cin1(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), out.data_ptr(), B, T_out, k, stride, Cout, xs, os_,
                                  _lib.stream_ptr()))
    sync()
    o = out.cpu()
    _close(family, o[:, : T_out * Cout].reshape(B, T_out, Cout), H.conv_cin1_ref(x, w, bias, T_out, stride))
    assert (o[:, T_out * Cout:] == SENT).all(), "rows at and beyond T_out / the slack between items were written"


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_conv_cin1_vector_form_matches_fp64(L, k, stride):
    """`conv_cin1_vec_kernel<3|5|7>`: one thread per row (C_out = 4) up to 256 (C_out = 1024), output lengths around the 512-step tile,
    three items whose strides are larger than their dense size."""
    for Cout in (4, 8, 64, 1024):
        for T_out in (1, 511, 512, 513, 1500):
            _conv_cin1_case(L, k, stride, Cout, T_out, "conv_cin1 vector form")


@pytest.mark.parametrize("k,stride,Cout", [(7, 1, 6), (7, 1, 40), (9, 1, 64), (7, 5, 64), (9, 5, 6)])
def test_conv_cin1_generic_form_matches_fp64(L, k, stride, Cout):
    """`conv_cin1_kernel`, taken for C_out not a multiple of 4, C_out / 4 not a divisor of 256, k outside {3, 5, 7}, stride > 4."""
    for T_out in (1, 511, 512, 513, 1500):
        _conv_cin1_case(L, k, stride, Cout, T_out, "conv_cin1 generic form")


# ------------------------------------------------------------------------------------------ ssrhip_conv_few_out
def _few_out_call(L, x, w, bias, out, B, T_out, k, Cin, Cout, act, xs, os_):
    return L.ssrhip_conv_few_out(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T_out, k, Cin, Cout, act, xs, os_,
                                 _lib.stream_ptr())


def _few_out_case(L, Cout, Cin, k, act, T_out, family, B=3):
    g = torch.Generator().manual_seed(1000003 * Cout + 10007 * Cin + 101 * k + 13 * act + T_out)
    rows = T_out + k - 1
    xs, os_ = rows * Cin + 12, (T_out + 2) * Cout + 3
    x = torch.randn(B, xs, generator=g)
    w = torch.randn(Cout, k, Cin, generator=g) / math.sqrt(k * Cin)
    bias = torch.randn(Cout, generator=g) * 0.1
    dx, dw, db = dev(x), dev(w), dev(bias)
    out = torch.full((B, os_), SENT, device="cuda")
    _lib.check(_few_out_call(L, dx, dw, db, out, B, T_out, k, Cin, Cout, act, xs, os_), "ssrhip_conv_few_out")
    sync()
    o = out.cpu()
    want = H.conv_few_out_ref(x[:, : rows * Cin].reshape(B, rows, Cin), w, bias, act == _lib.ACT_ELU)
    _close(family, o[:, : T_out * Cout].reshape(B, T_out, Cout), want)
    assert (o[:, T_out * Cout:] == SENT).all(), "rows at and beyond T_out / the slack between items were written"


@pytest.mark.parametrize("act", [_lib.ACT_NONE, _lib.ACT_ELU])
@pytest.mark.parametrize("k", [1, 3, 7, 16])
def test_conv_few_out_matrix_core_shapes_match_fp64(L, k, act):
    """C_out = 1, C_in = 64, k <= 16: `conv_one_out_mfma_kernel` (one tap, the product's 7, all 16 columns of the tile), output lengths
    around its 256-step workgroup tile. With SSRHIP_CONV_FEW_MFMA=0 in the environment the same shapes take the LDS form (below)."""
    for T_out in (1, 255, 256, 257, 5000):
        _few_out_case(L, 1, 64, k, act, T_out, "conv_few_out at (1, 64, k <= 16)")


@pytest.mark.parametrize("act", [_lib.ACT_NONE, _lib.ACT_ELU])
@pytest.mark.parametrize("Cout,Cin,k", [(1, 64, 17), (2, 64, 7), (4, 8, 7), (3, 72, 1), (1, 128, 7), (1, 192, 7), (1, 256, 7), (1, 512, 7)])
def test_conv_few_out_lds_form_matches_fp64(L, Cout, Cin, k, act):
    """`conv_few_out_kernel` on shapes that never take the matrix-core form. By the launcher's sizing rule (two workgroups per CU) the
    last four run at tiles of 128, 64, 32 and 32 time steps; (1, 64, 17) needs 78,336 bytes of dynamic LDS and (1, 512, 7) 92,768 — above
    the 64 KiB a kernel gets without hipFuncSetAttribute; (4, 8, 7), (1, 192, 7) and (1, 256, 7) stay below it."""
    for T_out in (1, 31, 32, 33, 65, 129, 300):
        _few_out_case(L, Cout, Cin, k, act, T_out, "conv_few_out LDS form")


def test_conv_few_out_lds_form_at_the_product_shape_in_a_child_process():
    """The product's own last layer (1, 64, 7) takes the LDS form only behind SSRHIP_CONV_FEW_MFMA=0, which the library reads once per
    process: the matrix-core cases again in a fresh child process with the switch set (73,056 bytes of dynamic LDS at the default tile of 256 steps)."""
    _child({"SSRHIP_CONV_FEW_MFMA": "0"}, "conv_few_out_matrix_core_shapes_match_fp64", 8)


@pytest.mark.parametrize("what,Cout,Cin,k,act", [("C_in % 8 != 0", 1, 12, 7, _lib.ACT_NONE), ("C_out = 5", 5, 64, 7, _lib.ACT_NONE),
                                                 ("act_in RELU", 1, 64, 7, _lib.ACT_RELU), ("act_in 99", 2, 64, 7, 99),
                                                 ("LDS need above 160 KB", 1, 1024, 7, _lib.ACT_ELU)])
def test_conv_few_out_refuses_what_it_cannot_run(L, what, Cout, Cin, k, act):
    B, T_out = 2, 40
    xs, os_ = (T_out + k - 1) * Cin + 4, T_out * Cout + 2
    x, w, bias = torch.randn(B, xs, device="cuda"), torch.randn(Cout, k, Cin, device="cuda"), torch.zeros(Cout, device="cuda")
    out = torch.full((B, os_), SENT, device="cuda")
    assert _few_out_call(L, x, w, bias, out, B, T_out, k, Cin, Cout, act, xs, os_) != 0, what
    sync()
    assert (out == SENT).all(), what


# ------------------------------------------------------------------------------------------ ssrhip_pad_reflect / ssrhip_pad_ragged
PADS = [(3, 3), (6, 0), (0, 6), (2, 5), (0, 0)]


@pytest.mark.parametrize("Cc", [1, 5, 64])
@pytest.mark.parametrize("padL,padR", PADS)
def test_pad_reflect_equals_the_reference_rule(L, padL, padR, Cc):
    """`pad_reflect_kernel` copies: exact. Inputs shorter than, equal to and longer than the pad (the reference's small-input rule: zero-
    extend, reflect, drop), one-sided and unequal pads, three items with slack between them; the halo is pre-filled with other values."""
    B = 3
    for T in (1, 2, 3, 4, 7, 50):
        g = torch.Generator().manual_seed(1000 * T + 100 * padL + 10 * padR + Cc)
        rows = padL + T + padR
        bs = rows * Cc + 7
        buf = torch.randn(B, bs, generator=g)                          # halo rows: stale values the kernel must overwrite
        buf[:, rows * Cc:] = SENT
        want = buf.clone()
        for b in range(B):
            item = buf[b, padL * Cc: (padL + T) * Cc].view(T, Cc)
            want[b, : rows * Cc] = H.pad_rows_ref(item, padL, padR, True).reshape(-1)
        d = dev(buf)
        _lib.check(L.ssrhip_pad_reflect(d.data_ptr(), B, T, padL, padR, Cc, bs, _lib.stream_ptr()))
        sync()
        assert torch.equal(d.cpu(), want), (T, padL, padR, Cc)


@pytest.mark.parametrize("reflect", [0, 1])
@pytest.mark.parametrize("Cc", [1, 5, 64])
@pytest.mark.parametrize("padL,padR", PADS)
def test_pad_ragged_equals_the_reference_rule_per_item(L, padL, padR, Cc, reflect):
    """`pad_ragged_kernel`: item b's halo for ITS OWN length (full, one short, shorter than the pad, 1, 0, and two out-of-range lengths
    that the kernel clamps to T and 0), exact. The interior [padL, padL + len) is bit-unchanged, rows right of padL + len + padR keep what
    the producer wrote (random values), the slack keeps its sentinel. With reflect == 0 the kernel writes the trailing halo only (the
    leading rows of a zero-padded buffer are zero for every length: include/ssrhip.h), so they are pre-filled as the producer leaves them."""
    T, lens = 50, [50, 49, 7, 3, 1, 0, 77, -4]
    B = len(lens)
    g = torch.Generator().manual_seed(100 * padL + 10 * padR + Cc + 7 * reflect)
    rows = padL + T + padR
    bs = rows * Cc + 9
    buf = torch.randn(B, bs, generator=g)
    buf[:, rows * Cc:] = SENT
    if not reflect:
        buf[:, : padL * Cc] = 0.0
    want = buf.clone()
    for b in range(B):
        Ti = min(max(lens[b], 0), T)
        item = buf[b, padL * Cc: (padL + Ti) * Cc].view(Ti, Cc)
        want[b, : (padL + Ti + padR) * Cc] = H.pad_rows_ref(item, padL, padR, bool(reflect)).reshape(-1)
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d = dev(buf)
    _lib.check(L.ssrhip_pad_ragged(d.data_ptr(), dl.data_ptr(), B, T, padL, padR, Cc, bs, reflect, _lib.stream_ptr()))
    sync()
    got = d.cpu()
    for b in range(B):
        Ti = min(max(lens[b], 0), T)
        lo, hi = padL * Cc, (padL + Ti) * Cc
        assert torch.equal(got[b, lo:hi], buf[b, lo:hi]), f"item {b}: interior changed"
        assert torch.equal(got[b, :lo], want[b, :lo]), f"item {b} (length {lens[b]}): leading halo"
        assert torch.equal(got[b, hi: hi + padR * Cc], want[b, hi: hi + padR * Cc]), f"item {b} (length {lens[b]}): trailing halo"
        assert torch.equal(got[b, hi + padR * Cc:], buf[b, hi + padR * Cc:]), f"item {b}: rows behind its halo / the slack changed"
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ ssrhip_rvq_decode
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("bins", [50, 2048])
@pytest.mark.parametrize("n_q", [1, 8])
@pytest.mark.parametrize("D", [20, 128, 130])
def test_rvq_decode_is_the_fp32_sum_in_the_documented_order(L, D, n_q, bins, T):
    """`rvq_decode_kernel` (128 threads per frame: D below, at and above it): 0.0 + q0 + q1 + ... in fp32, bit for bit."""
    B = 3
    g = torch.Generator().manual_seed(D + 1000 * n_q + bins + T)
    cb = torch.randn(n_q, bins, D, generator=g)
    codes = torch.randint(0, bins, (B, n_q, T), generator=g)
    codes[0, :, 0], codes[B - 1, :, T - 1] = 0, bins - 1
    os_ = T * D + 11
    out = torch.full((B, os_), SENT, device="cuda")
    dc, dcb = dev(codes.int()), dev(cb)
    _lib.check(L.ssrhip_rvq_decode(dc.data_ptr(), dcb.data_ptr(), out.data_ptr(), B, T, D, n_q, bins, os_, _lib.stream_ptr()))
    sync()
    o = out.cpu()
    assert torch.equal(o[:, : T * D].reshape(B, T, D), H.rvq_decode_ref(codes, cb))
    assert (o[:, T * D:] == SENT).all()


# ------------------------------------------------------------------------------------------ ssrhip_rvq_encode
def _rvq_encode(L, emb, cb, e2):
    """emb [B][T][D] with a slack batch stride (NaN: never to be read) -> codes int64 [B][n_q][T] on the host."""
    B, T, D = emb.shape
    n_q, bins, _ = cb.shape
    es = T * D + 24
    buf = torch.full((B, es), float("nan"))
    buf[:, : T * D] = emb.reshape(B, -1)
    codes = torch.full((B, n_q, T), -1, dtype=torch.int32, device="cuda")
    de, dcb, de2 = dev(buf), dev(cb), dev(e2)
    _lib.check(L.ssrhip_rvq_encode(de.data_ptr(), dcb.data_ptr(), de2.data_ptr(), codes.data_ptr(), B, T, D, n_q, bins, es,
                                   _lib.stream_ptr()))
    sync()
    return codes.cpu().long()


def _rvq_shape(L, monkeypatch, D, bins, n_q, kernels):
    kept = total = 0
    for T in H.RVQ_TS:
        emb, cb, e2 = H.rvq_case(D, bins, n_q, T)
        want, margins, err = H.rvq_encode_ref(emb, cb)
        keep = H.rvq_kept_frames(margins, err)                          # the float64 reference alone decides what is compared
        kept, total = kept + int(keep.sum()), total + keep.numel()
        got = {}
        for kern in kernels:
            if kern == "scalar":
                monkeypatch.setenv("SSRHIP_RVQ_SCALAR", "1")
            else:
                monkeypatch.delenv("SSRHIP_RVQ_SCALAR", raising=False)
            got[kern] = _rvq_encode(L, emb, cb, e2)
            monkeypatch.delenv("SSRHIP_RVQ_SCALAR", raising=False)
            assert int(got[kern].min()) >= 0 and int(got[kern].max()) < bins
            bad = (got[kern] != want).any(dim=1) & keep
            assert not bad.any(), (f"{kern} kernel, D={D} bins={bins} n_q={n_q} T={T}: {int(bad.sum())} of {int(keep.sum())} kept frames differ "
                                   f"from the float64 search (threshold {8 * err:.3g}); first at {bad.nonzero()[0].tolist()}")
        if len(kernels) == 2:
            k2 = keep[:, None, :].expand_as(want)
            assert torch.equal(got["mfma"][k2], got["scalar"][k2])
    share = kept / total
    _report["rvq_kept_share"][f"D={D} bins={bins} n_q={n_q}"] = round(share, 4)
    print(f"rvq_encode D={D} bins={bins} n_q={n_q}: {kept} of {total} frames kept ({100 * share:.1f} %)")
    assert share >= H.RVQ_MIN_KEPT, f"mis-designed case: the margin filter keeps only {kept} of {total} frames"


@pytest.mark.parametrize("D,bins,n_q", H.RVQ_MFMA_SHAPES)
def test_rvq_encode_both_kernels_match_the_fp64_search(L, monkeypatch, D, bins, n_q):
    """`rvq_encode_mfma_kernel<2|4|8|16>` and, on the same input with SSRHIP_RVQ_SCALAR set, `rvq_encode_kernel`: every code of every
    stage equals the float64 search on every frame whose smallest margin is at least 8 x the fp32 score error of the case (no excused
    mismatches; the filter must keep >= 90 % of the shape's frames), frame counts around the 16-frame tile."""
    _rvq_shape(L, monkeypatch, D, bins, n_q, ("mfma", "scalar"))


@pytest.mark.parametrize("D,bins,n_q", H.RVQ_SCALAR_ONLY_SHAPES)
def test_rvq_encode_scalar_kernel_matches_the_fp64_search(L, monkeypatch, D, bins, n_q):
    """Shapes only `rvq_encode_kernel` takes without a switch (D not in {32, 64, 128, 256}; fewer bins than threads, not a multiple of 16),
    and the full-config shape forced onto it."""
    _rvq_shape(L, monkeypatch, D, bins, n_q, ("scalar",))


@pytest.mark.parametrize("rows", [(5, 69), (3, 19), (1, 6), (40, 9), (5, 261), (9, 40, 133)])
@pytest.mark.parametrize("D,bins", [(64, 1024), (128, 2048)])
@pytest.mark.parametrize("kern", ["mfma", "scalar"])
def test_rvq_encode_exact_tie_goes_to_the_first_index(L, monkeypatch, kern, D, bins, rows):
    """torch.max's rule. Codebook row rows[0] is copied to the other rows and every frame equals it: both kernels do the same arithmetic
    for identical rows, so the scores tie bit for bit and the code must be min(rows). In the matrix-core kernel the pairs sit in the same
    lane one tile on, in different waves, in different k-slot lanes of one tile, and with the higher index in the lower wave's turn; in
    the scalar kernel in different threads and waves, and (5, 261) in the same thread 256 codes apart. And a three-way tie."""
    emb, cb, _ = H.rvq_case(D, bins, 1, 17)
    for r in rows[1:]:
        cb[0, r] = cb[0, rows[0]]
    e2 = cb.pow(2).sum(-1)
    assert all(e2[0, r] == e2[0, rows[0]] for r in rows)
    emb[:] = cb[0, rows[0]]
    want, margins, _ = H.rvq_encode_ref(emb, cb)
    assert (want == min(rows)).all() and (margins == 0).all()
    if kern == "scalar":
        monkeypatch.setenv("SSRHIP_RVQ_SCALAR", "1")
    got = _rvq_encode(L, emb, cb, e2)
    assert (got == min(rows)).all(), (kern, rows, got.unique().tolist())


# ------------------------------------------------------------------------------------------ ssrhip_lstm_layer without split planes
@functools.lru_cache(maxsize=None)
def _whh(Cc):
    return H.lstm_weights(Cc, seed=Cc)


@functools.lru_cache(maxsize=4)
def _whh_dev(Cc, packed):
    return dev(H.pack_whh(_whh(Cc)) if packed else _whh(Cc))


def _lstm_args(B, T, Cc, w, packed, gin, skip, out, hbuf, cbuf, strides, t0, t1, out_act):
    a = _lib.LstmArgs()
    a.gin, a.w_hh, a.out, a.skip = gin.data_ptr(), w.data_ptr(), out.data_ptr(), (skip.data_ptr() if skip is not None else 0)
    a.hbuf, a.cbuf, a.gates = hbuf.data_ptr(), cbuf.data_ptr(), 0
    a.B, a.T, a.C = B, T, Cc
    a.gin_bstride, a.out_bstride, a.skip_bstride = strides
    a.t_begin, a.t_end, a.w_packed, a.out_act = t0, t1, packed, out_act
    return a


def _lstm_case(L, B, Cc, packed, epilogue, family, T=5):
    """One layer in two time windows (the chunked pipeline's calling pattern), hbuf and cbuf pre-filled with NaN (the library zeroes h_0,
    and c is not read at t = 0), batch strides with slack, with or without the skip add + ELU-on-store epilogue."""
    g = torch.Generator().manual_seed(1000 * B + Cc + 7 * packed + int(epilogue))
    gs, os_, ss = T * 4 * Cc + 16, T * Cc + 8, T * Cc + 4
    gin = torch.randn(B, gs, generator=g)
    skip = torch.randn(B, ss, generator=g) if epilogue else None
    out_act = _lib.ACT_ELU if epilogue else _lib.ACT_NONE
    want = H.lstm_ref(gin[:, : T * 4 * Cc].reshape(B, T, 4 * Cc), _whh(Cc), skip[:, : T * Cc].reshape(B, T, Cc) if epilogue else None, epilogue)
    dgin, dskip, w = dev(gin), (dev(skip) if epilogue else None), _whh_dev(Cc, packed)
    rows = (B + 15) // 16 * 16
    out = torch.full((B, os_), float("nan"), device="cuda")
    hbuf, cbuf = torch.full((2, rows, Cc), float("nan"), device="cuda"), torch.full((B, Cc), float("nan"), device="cuda")
    for t0, t1 in ((0, T // 2), (T // 2, T)):
        a = _lstm_args(B, T, Cc, w, packed, dgin, dskip, out, hbuf, cbuf, (gs, os_, ss), t0, t1, out_act)
        _lib.check(L.ssrhip_lstm_layer(C.byref(a), _lib.stream_ptr()), "ssrhip_lstm_layer")
    sync()
    o = out.cpu()
    _close(family, o[:, : T * Cc].reshape(B, T, Cc), want)
    assert torch.isnan(o[:, T * Cc:]).all(), "the slack between items was written"


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("Cc", [256, 512, 1024, 2048])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_lstm_small_batch_kernel_matches_fp64(L, B, Cc, epilogue):
    """`lstm_step_kernel<B, C / 256>`: all sixteen instantiations."""
    _lstm_case(L, B, Cc, 0, epilogue, "lstm small-batch kernel")


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("B,Cc", [(5, 48), (16, 128), (17, 272), (33, 272), (20, 1024), (3, 128), (9, 512)])
def test_lstm_matrix_core_kernel_matches_fp64(L, B, Cc, packed, epilogue):
    """`lstm_step_mfma_kernel<1>` (one batch tile, or one wave) and `<2>` with W_hh in torch's layout and packed. C = 272 has 17 k-steps: a
    second wave that owns one, so the `min(tbase + i, last)` clamps and the zeroed operands are the active case; B = 33 leaves the second
    workgroup row one real batch tile of its two; (3, 128) is a small batch at a width the small-batch kernel does not have; (9, 512) is
    `<1>` on two waves."""
    _lstm_case(L, B, Cc, packed, epilogue, "lstm matrix-core kernel")


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("B,Cc", [(113, 64), (130, 1024), (128, 272)])
def test_lstm_wide_kernel_matches_fp64(L, B, Cc, epilogue):
    """`lstm_step_wide_kernel<4>` (packed W_hh, 8 batch tiles and more) against the independent reference: a ragged last tile, a ragged
    last group of four tiles at full width, and the ragged-k-step width. With SSRHIP_LSTM_NOWIDE in the environment the same calls take
    `lstm_step_mfma_kernel<2>` / `<1>`, the kernel it replaces (below)."""
    _lstm_case(L, B, Cc, 1, epilogue, "lstm wide kernel" if "SSRHIP_LSTM_NOWIDE" not in os.environ else "lstm matrix-core kernel, 8+ batch tiles")


def test_lstm_large_batches_without_the_wide_kernel_in_a_child_process():
    """SSRHIP_LSTM_NOWIDE is read once per process: the large-batch cases again in a fresh child process, same bar."""
    _child({"SSRHIP_LSTM_NOWIDE": "1"}, "lstm_wide_kernel_matches_fp64", 6)


@pytest.mark.parametrize("what,B,Cc,packed,window", [("packed W_hh on the small-batch path", 2, 256, 1, (0, 0)), ("C % 16 != 0", 5, 24, 0, (0, 0)),
                                                     ("matrix-core path above C = 1024", 5, 2048, 0, (0, 0)), ("empty time window", 5, 48, 0, (3, 2)),
                                                     ("time window beyond T", 5, 48, 0, (0, 6)), ("negative t_begin", 2, 256, 0, (-1, 2))])
def test_lstm_layer_refuses_what_it_cannot_run(L, what, B, Cc, packed, window):
    T = 5
    w = torch.zeros(4 * Cc, Cc, device="cuda")
    gin, out = torch.zeros(B, T * 4 * Cc, device="cuda"), torch.full((B, T * Cc), SENT, device="cuda")
    hbuf, cbuf = torch.zeros(2, 16, Cc, device="cuda"), torch.zeros(B, Cc, device="cuda")
    a = _lstm_args(B, T, Cc, w, packed, gin, None, out, hbuf, cbuf, (T * 4 * Cc, T * Cc, T * Cc), window[0], window[1], _lib.ACT_NONE)
    assert L.ssrhip_lstm_layer(C.byref(a), _lib.stream_ptr()) != 0, what
    sync()
    assert (out == SENT).all(), what
