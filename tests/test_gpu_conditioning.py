"""GPU: every hand-written copy of the LayerNorm prologue and of the split-KV softmax merge / online-softmax rescale against fp64, on
the ill-conditioned inputs of helpers_conditioning.py (offset, step, outlier, tiny and constant rows; partial maxima and logits that
span far beyond what exp() holds in fp32 without the max subtraction).

One rule for every bound: tol = max(floor, M * err_ref32), err_ref32 = max |fp32 torch CPU - fp64| on the same inputs (helpers_conditioning
.tol; the measured err_kernel / err_ref32 per form are in profiles/numerics_conditioning.md). tests/test_conditioning_inputs.py shows
that a one-pass variance, a slice merge without its between-slice term, eps outside the square root and a softmax without the max
subtraction each miss the widest such bound at least tenfold, so reverting any copy to one of them fails here. Every test prints a
`RATIO|form|case|err_kernel|err_ref32|ratio` line per comparison before it asserts.

Which kernel a shape reaches (read from the launch plans, csrc/gemv_shared.h `seg_plan`, csrc/gemv_mfma_tile.h `gemv_rows_plan`):
  * 1/2/4 rows, LN folded, K % 1024 == 0: the segment kernel (S = K / 1024 slices); at 2 rows and N = 4096 / 6144, K = 2048 its
    straight-line `segu` form (the form exists for 2 rows only: at 1 and 4 rows the same shapes run the segment kernel again);
  * 1/2/4 rows, gamma / beta given, or K = 512, or SSRHIP_GEMV_SEG=0: the row-per-wave kernels (staged form with gamma / beta, folded
    wave form; a folded LayerNorm beyond K = 2048 is refused there);
  * 5..16 rows: a LayerNorm launch always keeps x in registers (`xreg`, 16 k-steps per wave up to K = 2048, 32 at K = 4096), so NO shape
    sends a LayerNorm launch to `gemv_rows_stream_kernel` (plan: xreg = K <= 2048 || LayerNorm) — the stream kernel has no LayerNorm copy
    that can run; SSRHIP_GEMVM_EDGE=1 at K = 2048 with tiled x: the edge kernel; SSRHIP_GEMVM_V=1: the per-tile kernel (row-major weights
    only: the streaming order is a checked refusal);
  * 17..32 rows: the two-panel kernel up to K = 2048; K = 4096 with LayerNorm is a checked refusal."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib

import helpers_conditioning as hc
import helpers_kv16 as HK

pytestmark = pytest.mark.gpu

PAD, POISON = 64, -777.25
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def _ratio(form, case, err_k, err_ref):
    r = err_k / err_ref if err_ref > 0 else (0.0 if err_k == 0 else float("inf"))
    print(f"RATIO|{form}|{case}|{err_k:.4g}|{err_ref:.4g}|{r:.3g}")


# ------------------------------------------------------------------------------------------ layouts
def _to_tiled(t, fill=POISON):
    B, K = t.shape
    out = torch.full((K // 4, 16, 4), fill)
    out[:, :B, :] = t.view(B, K // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def _from_tiled(t, B, K):
    return t.view(K // 4, 16, 4)[:, :B, :].permute(1, 0, 2).reshape(B, K)


def _to_panels(t, fill=POISON):
    B, K = t.shape
    out = torch.full((2, K // 4, 16, 4), fill)
    for p in range(2):
        rows = t[16 * p:min(B, 16 * p + 16)]
        out[p, :, :rows.shape[0], :] = rows.reshape(rows.shape[0], K // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def _from_panels(t, B, K):
    return t.view(2, K // 4, 16, 4).permute(0, 2, 1, 3).reshape(32, K)[:B]


def _pack(t, tiled):
    return (_to_panels(t) if t.shape[0] > 16 else _to_tiled(t)) if tiled else t.reshape(-1)


def _unpack(buf, B, N, tiled):
    return (_from_panels(buf, B, N) if B > 16 else _from_tiled(buf, B, N)) if tiled else buf.view(B, N)


# ------------------------------------------------------------------------------------------ LayerNorm prologue through ssrhip_gemv
def _gemv_ln(L, x, dW, dbias, N, act, y0, dlw, dlb, tiled, w_tiled):
    """One LayerNorm launch; y sits between two poisoned pads. Returns (rc, y [B, N] or None, the buffer was left as it must be)."""
    B, K = x.shape
    body = _pack(y0 if y0 is not None else torch.full((B, N), POISON), tiled)
    buf0 = torch.cat([torch.full((PAD,), POISON), body, torch.full((PAD,), POISON)])
    buf = buf0.cuda()
    dx = _pack(x, tiled).contiguous().cuda()
    a = _lib.GemvArgs()
    a.W, a.bias, a.x, a.y = dW.data_ptr(), dbias.data_ptr(), dx.data_ptr(), buf.data_ptr() + 4 * PAD
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, N
    a.pro, a.act, a.epi, a.ln_eps = _lib.PRO_LAYERNORM, act, (_lib.EPI_RESIDUAL if y0 is not None else _lib.EPI_STORE), hc.LN_EPS
    if dlw is not None:
        a.ln_w, a.ln_b = dlw.data_ptr(), dlb.data_ptr()
    a.x_tiled, a.y_tiled, a.w_tiled = tiled, tiled, w_tiled
    rc = L.ssrhip_gemv(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = buf.cpu()
    pads_ok = bool((got[:PAD] == POISON).all()) and bool((got[PAD + body.numel():] == POISON).all())
    if rc != 0:
        return rc, None, torch.equal(got, buf0)                              # a refusal writes nothing
    if tiled and B > 16:                                                     # rows >= B of panel 1 are nobody's
        pads_ok = pads_ok and bool((got[PAD:PAD + body.numel()].view(2, N // 4, 16, 4)[1, :, B - 16:, :] == POISON).all())
    return 0, _unpack(got[PAD:PAD + body.numel()], B, N, tiled).clone(), pads_ok


def ln_records(L, form, B, N, K, tiled=0, w_tiled=0, unfolded=False, cases=None):
    """Every row case x act in {none, GELU} x {store, residual} of one (form, shape): a list of records, one per launch —
    dict(form, case, act, res, rc, err_k, err_ref, clean, exact). `exact` (const rows only): the output equals, bit for bit, the same
    launch on an all-zero x (x' = 0 both ways, so the pre-activation is the bias term alone and the kernel's own act() is applied to
    it), and with a folded LayerNorm and no activation it equals fp32 bias (+ y0) itself."""
    from ssr_speech_amd.engine import to_streaming_order
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    y0 = torch.randn(B, N, generator=g)
    lw = lb = dlw = dlb = None
    if unfolded:
        lw, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        dlw, dlb = lw.cuda(), lb.cuda()
    dW, dbias = (to_streaming_order(W) if w_tiled else W).contiguous().cuda(), bias.cuda()
    W64, bias64 = W.double(), bias.double()
    recs = []
    for case, x in hc.ln_rows(B, K, K + B).items():
        if cases is not None and case not in cases:
            continue
        for act in (_lib.ACT_NONE, _lib.ACT_GELU_ERF):
            for res in (False, True):
                yy = y0 if res else None
                want = hc.ln_linear_ref(x, W64, bias64, act, yy, lw, lb)
                err_ref = hc.max_err(hc.ln_linear_ref(x, W, bias, act, yy, lw, lb, dtype=torch.float32), want)
                rc, got, clean = _gemv_ln(L, x, dW, dbias, N, act, yy, dlw, dlb, tiled, w_tiled)
                rec = dict(form=form, case=case, act=act, res=res, rc=rc, clean=clean, err_ref=err_ref, err_k=None, exact=None)
                if rc == 0:
                    rec["err_k"] = hc.max_err(got, want)
                    if case == "const":
                        _, zero, _ = _gemv_ln(L, torch.zeros(B, K), dW, dbias, N, act, yy, dlw, dlb, tiled, w_tiled)
                        rec["exact"] = torch.equal(got.view(torch.int32), zero.view(torch.int32))
                        if not unfolded and act == _lib.ACT_NONE:
                            plain = bias.expand(B, N) + y0 if res else bias.expand(B, N)
                            rec["exact"] = rec["exact"] and torch.equal(got, plain)
                recs.append(rec)
    return recs


def check_ln_records(recs, refused=False):
    assert recs
    bad = []
    for r in recs:
        if r["rc"] == 0:
            _ratio(r["form"], f"{r['case']}/act{r['act']}/res{int(r['res'])}", r["err_k"], r["err_ref"])
    for r in recs:
        assert r["clean"], ("the pads around y (or, refused, the whole buffer) changed", r)
        if refused:
            assert r["rc"] != 0, ("the library takes a shape the plan says it refuses", r)
            continue
        assert r["rc"] == 0, r
        if not r["err_k"] <= hc.tol(hc.FLOOR_GEMV, r["err_ref"]):
            bad.append(r)
        if r["case"] == "const" and not r["exact"]:
            bad.append(r)
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("N", [96, 520])
@pytest.mark.parametrize("K", [1024, 2048, 4096])
def test_layernorm_segment_kernel(L, B, N, K):
    """S = 1, 2, 4 slices; N = 96: one row per workgroup, N = 520: 512 workgroups, 8 of them with a second row (`rows_rem`)."""
    check_ln_records(ln_records(L, f"seg/B{B}/N{N}/K{K}", B, N, K))


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("N", [4096, 6144])
def test_layernorm_segu_shapes(L, B, N):
    """The shapes tests/test_gpu_kernels.py::test_gemv_segu_kernel_is_bit_identical_to_the_segment_kernel uses (4 and 6 units per wave):
    `gemv_segu_kernel` at 2 rows, the segment kernel at 1 and 4."""
    check_ln_records(ln_records(L, f"segu/B{B}/N{N}/K2048", B, N, 2048))


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("K", [128, 2048, 4096])
def test_layernorm_row_per_wave_unfolded(L, B, K):
    """gamma / beta given: `seg_plan` declines, the staged form of the row-per-wave kernels runs (1, 2 slices at K = 4096). The staged
    x needs B * K * 4 <= 60 KiB of LDS: 4 rows at K = 4096 are a checked refusal (ssrhip_gemv: "staged prologue needs ...")."""
    refused = B * K * 4 > 60 * 1024
    check_ln_records(ln_records(L, f"rowwave_unfolded/B{B}/K{K}", B, 77, K, unfolded=True), refused=refused)


@pytest.mark.parametrize("B", [1, 2, 4])
def test_layernorm_row_per_wave_folded_k512(L, B):
    check_ln_records(ln_records(L, f"rowwave_folded/B{B}/K512", B, 77, 512))


def _child(what):
    """Entry point of the child processes (switches that are read once per process): prints the records as one JSON line."""
    L = _lib.lib()
    recs = []
    if what == "seg0":
        for B in (1, 2, 4):
            recs += ln_records(L, f"rowwave_folded_seg0/B{B}/K2048", B, 77, 2048)
    elif what == "v1":
        for B in (5, 16):
            for K in (128, 2048, 4096):
                for tiled in (0, 1):
                    recs += ln_records(L, f"pertile/B{B}/K{K}/t{tiled}", B, 204, K, tiled=tiled)
            recs += [dict(r, refused=True) for r in ln_records(L, f"pertile_wt/B{B}", B, 204, 2048, w_tiled=1, cases=("offset",))]
    print("RECORDS" + json.dumps(recs))


def _run_child(what, env):
    code = f"import sys; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; import test_gpu_conditioning as t; t._child({what!r})"
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.split("RECORDS")[-1])


def test_layernorm_row_per_wave_folded_k2048_without_the_segment_kernel():
    check_ln_records(_run_child("seg0", {"SSRHIP_GEMV_SEG": "0"}))


def test_layernorm_per_tile_kernel():
    """SSRHIP_GEMVM_V=1: `gemv_mfma_kernel`, row-major and tiled activations; it has no streaming-order weights: a checked refusal."""
    recs = _run_child("v1", {"SSRHIP_GEMVM_V": "1"})
    check_ln_records([r for r in recs if not r.get("refused")])
    check_ln_records([r for r in recs if r.get("refused")], refused=True)


@pytest.mark.parametrize("B", [5, 16])
@pytest.mark.parametrize("K", [16, 128, 2048, 4096])
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("w_tiled", [0, 1])
def test_layernorm_xreg_kernel(L, monkeypatch, B, K, tiled, w_tiled):
    """`gemv_rows_xreg_kernel`, 16 k-steps of x per wave (K <= 2048: 1, 1 and 8 waves) and 32 (K = 4096); N = 204: 25.5 units of 8 rows."""
    monkeypatch.delenv("SSRHIP_GEMVM_EDGE", raising=False)
    check_ln_records(ln_records(L, f"xreg/B{B}/K{K}/t{tiled}/wt{w_tiled}", B, 204, K, tiled=tiled, w_tiled=w_tiled))


@pytest.mark.parametrize("B", [5, 16])
@pytest.mark.parametrize("w_tiled", [0, 1])
def test_layernorm_edge_kernel(L, monkeypatch, B, w_tiled):
    """`gemv_rows_edge_kernel` (SSRHIP_GEMVM_EDGE=1, read at every launch): K = 2048, tiled x, N = 2048 = one 8-row unit per workgroup."""
    monkeypatch.setenv("SSRHIP_GEMVM_EDGE", "1")
    check_ln_records(ln_records(L, f"edge/B{B}/wt{w_tiled}", B, 2048, 2048, tiled=1, w_tiled=w_tiled))


@pytest.mark.parametrize("B", [17, 32])
@pytest.mark.parametrize("K", [128, 2048])
@pytest.mark.parametrize("tiled", [0, 1])
def test_layernorm_32_row_kernel(L, B, K, tiled):
    check_ln_records(ln_records(L, f"rows32/B{B}/K{K}/t{tiled}", B, 204, K, tiled=tiled, w_tiled=tiled))


@pytest.mark.parametrize("B", [17, 32])
def test_layernorm_32_rows_at_k4096_is_refused(L, B):
    """Two panels of 32 k-steps do not fit the registers: the launcher refuses, and writes nothing."""
    check_ln_records(ln_records(L, f"rows32/B{B}/K4096", B, 204, 4096, cases=("offset", "const")), refused=True)


@pytest.mark.parametrize("D", [128, 2048])
def test_layernorm_kernel_with_gamma_and_beta(L, D):
    """`ssrhip_layernorm` (csrc/gemm.hip), 5 rows; floor: the 1e-5 of tests/test_gpu_kernels.py::test_layernorm_and_kv_scatter."""
    R = 5
    g = torch.Generator().manual_seed(D)
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dw, db = w.cuda(), b.cuda()
    bad = []
    for case, x in hc.ln_rows(R, D, D).items():
        want = hc.layernorm_ref(x, w, b)
        err_ref = hc.max_err(hc.layernorm_ref(x, w, b, dtype=torch.float32), want)
        buf = torch.full((PAD + R * D + PAD,), POISON, device="cuda")
        dx = x.cuda()
        _lib.check(L.ssrhip_layernorm(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), hc.LN_EPS, buf.data_ptr() + 4 * PAD, R, D, _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = buf.cpu()
        assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + R * D:] == POISON).all())
        y = got[PAD:PAD + R * D].view(R, D)
        err_k = hc.max_err(y, want)
        _ratio(f"layernorm/D{D}", case, err_k, err_ref)
        if not err_k <= hc.tol(1e-5, err_ref):
            bad.append((case, err_k, err_ref))
        if case == "const" and not torch.equal(y, b.expand(R, D)):
            bad.append((case, "not beta exactly"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ split-KV merge
def _merge_lens(B, MS):
    return ([1000, 129, 1, 897] if MS == 8 else [128, 1, 77, 100])[:B]


def _gemv_merge(L, B, N, K, H, hd, MS, lens, part_o, part_ml, dW, dbias, y0):
    buf0 = torch.cat([torch.full((PAD,), POISON), y0.reshape(-1), torch.full((PAD,), POISON)])
    buf = buf0.cuda()
    d_po, d_ml, dlen = part_o.cuda(), part_ml.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    a = _lib.GemvArgs()
    a.W, a.bias, a.y, a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = dW.data_ptr(), dbias.data_ptr(), buf.data_ptr() + 4 * PAD, B, N, K, 1, K, N
    a.pro, a.act, a.epi = _lib.PRO_ATTN_COMBINE, 0, _lib.EPI_RESIDUAL
    a.part_o, a.part_ml, a.max_splits, a.row_len = d_po.data_ptr(), d_ml.data_ptr(), MS, dlen.data_ptr()
    a.kv = _lib.KV(0, 0, MS, 1, H, hd)
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + B * N:] == POISON).all())
    return got[PAD:PAD + B * N].view(B, N).clone()


def _merge_linear_check(L, monkeypatch, form, B, K, H, hd, MS, both_grids):
    N = 48
    lens = _merge_lens(B, MS)
    g = torch.Generator().manual_seed(B * 10 + MS + K)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    y0 = torch.randn(B, N, generator=g)
    dW, dbias = W.cuda(), bias.cuda()
    part_o = hc.merge_part_o(B, H, MS, hd, lens, K + B)
    bad = []
    for case, ml in hc.ml_cases(B, H, MS, lens, K + MS).items():
        lin = lambda xin, dt: y0.to(dt) + F.linear(xin, W.to(dt), bias.to(dt))
        want = lin(hc.merge_ref(part_o, ml, lens), torch.float64)
        err_ref = hc.max_err(lin(hc.merge_ref(part_o, ml, lens, dtype=torch.float32), torch.float32), want)
        monkeypatch.delenv("SSRHIP_GEMV_SEG_COMBINE_2", raising=False)
        got = _gemv_merge(L, B, N, K, H, hd, MS, lens, part_o, ml, dW, dbias, y0)
        if both_grids:                                                       # read at every call: one / two workgroups per CU
            monkeypatch.setenv("SSRHIP_GEMV_SEG_COMBINE_2", "1")
            two = _gemv_merge(L, B, N, K, H, hd, MS, lens, part_o, ml, dW, dbias, y0)
            if not torch.equal(got.view(torch.int32), two.view(torch.int32)):
                bad.append((case, "one and two workgroups per CU differ"))
        err_k = hc.max_err(got, want)
        _ratio(form, case, err_k, err_ref)
        if not err_k <= hc.tol(hc.FLOOR_GEMV, err_ref):
            bad.append((case, err_k, err_ref))
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("MS", [8, 1])
def test_merge_prologue_segment_kernel(L, monkeypatch, B, MS):
    """K = 2048, 16 heads of 128; 8 pages: past the prefetched ones (6 at <= 2 rows, 2 at 4 rows), the cold path; and a single page."""
    _merge_linear_check(L, monkeypatch, f"merge_seg/B{B}/MS{MS}", B, 2048, 16, 128, MS, both_grids=True)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("MS", [8, 1])
def test_merge_prologue_row_per_wave_kernel(L, monkeypatch, B, MS):
    """K = 512 (4 heads): not the segment kernel's shape, the row-per-wave kernels merge."""
    _merge_linear_check(L, monkeypatch, f"merge_rowwave/B{B}/MS{MS}", B, 512, 4, 128, MS, both_grids=False)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("tiled", [0, 1])
def test_attn_combine_kernel(L, hd, tiled):
    R, H, MS = 4, 3, 8
    lens = _merge_lens(R, MS)
    D = H * hd
    part_o = hc.merge_part_o(R, H, MS, hd, lens, hd)
    dummy = torch.zeros(64, device="cuda")
    dlen = torch.tensor(lens, dtype=torch.int32).cuda()
    bad = []
    for case, ml in hc.ml_cases(R, H, MS, lens, hd + 1).items():
        want = hc.merge_ref(part_o, ml, lens)
        err_ref = hc.max_err(hc.merge_ref(part_o, ml, lens, dtype=torch.float32), want)
        d_po, d_ml = part_o.cuda(), ml.cuda()
        n_out = (16 if tiled else R) * D
        buf = torch.full((PAD + n_out + PAD,), POISON, device="cuda")
        a = _lib.AttnArgs()
        a.q, a.q_stride = dummy.data_ptr(), 0
        a.kv = _lib.KV(dummy.data_ptr(), dummy.data_ptr(), MS, 1, H, hd)
        a.layer, a.row_seq, a.row_len, a.R, a.max_splits = 0, 0, dlen.data_ptr(), R, MS
        a.scale, a.part_o, a.part_ml, a.out_tiled = 1.0 / math.sqrt(hd), d_po.data_ptr(), d_ml.data_ptr(), tiled
        _lib.check(L.ssrhip_attn_combine(C.byref(a), buf.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = buf.cpu()
        assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + n_out:] == POISON).all())
        y = _unpack(got[PAD:PAD + n_out], R, D, tiled)
        err_k = hc.max_err(y, want)
        _ratio(f"attn_combine/hd{hd}/t{tiled}", case, err_k, err_ref)
        if not err_k <= hc.tol(hc.FLOOR_ATTN, err_ref):
            bad.append((case, err_k, err_ref))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ attention
ALENS = [1, 129, 257, 385]
_PROBLEMS = {}


def _problem(case, hd, kind):
    """Built once per (case, head_dim, kind) and never modified: the problem, its fp64 reference and the fp32 reference's error.
    kind: rows | prefill | rows16 | prefill16 (16: the pool rounded to bf16, references on the ROUNDED values) | group."""
    key = (case, hd, kind)
    if key not in _PROBLEMS:
        causal = kind.startswith("prefill")
        pb = hc.attn_problem(case, 2, hd, ALENS, 7 * hd + hc.LOGIT_CASES.index(case), gains=causal,
                             share=[(0, 1), (2, 3)] if kind == "group" else ())
        pool = HK.round_bf16(pb["pool"]) if kind.endswith("16") else pb["pool"]
        want = hc.attn_problem_ref(pb, causal=causal, pool=pool)
        err_ref = hc.max_err(hc.attn_problem_ref(pb, dtype=torch.float32, causal=causal, pool=pool), want)
        _PROBLEMS[key] = (pb, pool, want, err_ref)
    return _PROBLEMS[key]


def _attn_args(pb, d_pool, d_table, d_q, d_len):
    a = _lib.AttnArgs()
    a.q, a.q_stride = d_q.data_ptr(), 0
    a.kv = _lib.KV(d_pool.data_ptr(), d_table.data_ptr(), pb["max_pages"], pb["n_layer"], pb["H"], pb["hd"])
    a.layer, a.row_seq, a.row_len, a.R, a.max_splits = pb["layer"], 0, d_len.data_ptr(), len(pb["lens"]), pb["max_pages"]
    a.scale = 1.0 / math.sqrt(pb["hd"])
    return a


def _poisoned(n):
    return torch.full((PAD + n + PAD,), POISON, device="cuda")


def _take(buf, n):
    got = buf.cpu()
    assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + n:] == POISON).all())
    return got[PAD:PAD + n]


def _judge(form, results):
    """results: (case, got, want, err_ref) — print every ratio, then assert every bound"""
    bad = []
    for case, got, want, err_ref in results:
        err_k = hc.max_err(got, want)
        _ratio(form, case, err_k, err_ref)
        if not err_k <= hc.tol(hc.FLOOR_ATTN, err_ref):
            bad.append((case, err_k, err_ref))
    assert not bad, (form, bad)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_decode_and_combine(L, hd):
    """`attn_decode_kernel` (one workgroup per page, online softmax inside the page) + `attn_combine_kernel`."""
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "rows")
        R, H, MS, D = 4, pb["H"], pb["max_pages"], pb["H"] * hd
        d_pool, d_table, d_q, d_len = pool.cuda(), pb["table"].cuda(), pb["q"].cuda(), torch.tensor(ALENS, dtype=torch.int32).cuda()
        part_o = torch.full((R * H * MS * hd,), float("nan"), device="cuda")
        part_ml = torch.full((R * H * MS * 2,), float("nan"), device="cuda")
        out = _poisoned(R * D)
        a = _attn_args(pb, d_pool, d_table, d_q, d_len)
        a.part_o, a.part_ml = part_o.data_ptr(), part_ml.data_ptr()
        _lib.check(L.ssrhip_attn_decode(C.byref(a), _lib.stream_ptr()))
        _lib.check(L.ssrhip_attn_combine(C.byref(a), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, R * D).view(R, D), want, err_ref))
    _judge(f"attn_decode+combine/hd{hd}", results)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("tiled", [0, 1])
def test_attention_rows(L, hd, tiled):
    """`attn_rows_kernel`: the fused walk over a row's pages, the online-softmax rescale between pages."""
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "rows")
        R, D = 4, pb["H"] * hd
        d_pool, d_table, d_q, d_len = pool.cuda(), pb["table"].cuda(), pb["q"].cuda(), torch.tensor(ALENS, dtype=torch.int32).cuda()
        n_out = (16 if tiled else R) * D
        out = _poisoned(n_out)
        a = _attn_args(pb, d_pool, d_table, d_q, d_len)
        a.out_tiled = tiled
        _lib.check(L.ssrhip_attn_rows(C.byref(a), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _unpack(_take(out, n_out), R, D, tiled), want, err_ref))
    _judge(f"attn_rows/hd{hd}/t{tiled}", results)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_rows_group(L, hd):
    """`attn_rows_group_kernel`, chunks of 2: rows (0, 1) and (2, 3) name the same first physical page; a member's q is 0.9 x its
    head's, so the shared page gives it 0.9 x the head's logits and its own pages its own targets."""
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "group")
        R, D = 4, pb["H"] * hd
        d_pool, d_table, d_q, d_len = pool.cuda(), pb["table"].cuda(), pb["q"].cuda(), torch.tensor(ALENS, dtype=torch.int32).cuda()
        head, ns = torch.tensor([0, 0, 2, 2], dtype=torch.int32).cuda(), torch.tensor([1, 0, 1, 0], dtype=torch.int32).cuda()
        out = _poisoned(R * D)
        a = _attn_args(pb, d_pool, d_table, d_q, d_len)
        _lib.check(L.ssrhip_attn_rows_group_m(C.byref(a), head.data_ptr(), ns.data_ptr(), 2, out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, R * D).view(R, D), want, err_ref))
    _judge(f"attn_rows_group_m/hd{hd}", results)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_prefill(L, hd):
    """`attn_prefill_body`: causal, every query of a sequence along the direction the keys were built for, gains in [0.5, 1]."""
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "prefill")
        n, D = sum(ALENS), pb["H"] * hd
        d_pool, d_table, d_q = pool.cuda(), pb["table"].cuda(), pb["q"].cuda()
        starts = torch.tensor([0, 1, 130, 387, 772], dtype=torch.int32).cuda()
        out = _poisoned(n * D)
        a = _attn_args(pb, d_pool, d_table, d_q, starts)
        a.row_len, a.R = 0, n
        _lib.check(L.ssrhip_attn_prefill(C.byref(a), starts.data_ptr(), 4, max(ALENS), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, n * D).view(n, D), want, err_ref))
    _judge(f"attn_prefill/hd{hd}", results)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("depth", ["2", "4"])
def test_attention_rows_kv16(L, monkeypatch, hd, depth):
    """The 2-byte cache, 2 and 4 pages in flight (SSRHIP_ATTN_KV16_DEPTH, read at every launch): against fp64 on the rounded pool."""
    monkeypatch.setenv("SSRHIP_ATTN_KV16_DEPTH", depth)
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "rows16")
        R, D = 4, pb["H"] * hd
        d_pool, d_table, d_q, d_len = HK.bf16_bits(pool).cuda(), pb["table"].cuda(), pb["q"].cuda(), torch.tensor(ALENS, dtype=torch.int32).cuda()
        out = _poisoned(R * D)
        a = _attn_args(pb, d_pool, d_table, d_q, d_len)
        _lib.check(L.ssrhip_attn_rows_kv16(C.byref(a), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, R * D).view(R, D), want, err_ref))
    _judge(f"attn_rows_kv16/hd{hd}/depth{depth}", results)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_prefill_kv16(L, hd):
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "prefill16")
        n, D = sum(ALENS), pb["H"] * hd
        d_pool, d_table, d_q = HK.bf16_bits(pool).cuda(), pb["table"].cuda(), pb["q"].cuda()
        starts = torch.tensor([0, 1, 130, 387, 772], dtype=torch.int32).cuda()
        out = _poisoned(n * D)
        a = _attn_args(pb, d_pool, d_table, d_q, starts)
        a.row_len, a.R = 0, n
        _lib.check(L.ssrhip_attn_prefill_kv16(C.byref(a), starts.data_ptr(), 4, max(ALENS), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, n * D).view(n, D), want, err_ref))
    _judge(f"attn_prefill_kv16/hd{hd}", results)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_decode_kv16_with_its_landing_cache(L, hd):
    """`ssrhip_attn_decode_kv16` + combine: a row's last key / value arrive UNROUNDED in the landing cache (position `layer` of the row's
    page there), the pool holds NaN bits at that position; the kernel rounds the landing entry, and fp64 sees the rounded values."""
    results = []
    for case in hc.LOGIT_CASES:
        pb, pool, want, err_ref = _problem(case, hd, "rows16")
        R, H, MS, D, layer = 4, pb["H"], pb["max_pages"], pb["H"] * hd, pb["layer"]
        pool16 = HK.bf16_bits(pool)
        land = torch.randn(R, 1, 2, H, hc.PAGE, hd, generator=torch.Generator().manual_seed(hd))
        for r, ln in enumerate(ALENS):
            page, j = int(pb["table"][r, (ln - 1) // hc.PAGE]), (ln - 1) % hc.PAGE
            land[r, 0, :, :, layer] = pb["pool"][page, layer, :, :, j]                 # the fp32 entries, before rounding
            pool16[page, layer, :, :, j] = 0x7FC0                                      # NaN: the pool's own entry must not be used
        d_pool, d_table, d_q, d_len = pool16.cuda(), pb["table"].cuda(), pb["q"].cuda(), torch.tensor(ALENS, dtype=torch.int32).cuda()
        d_land = land.cuda()
        part_o = torch.full((R * H * MS * hd,), float("nan"), device="cuda")
        part_ml = torch.full((R * H * MS * 2,), float("nan"), device="cuda")
        out = _poisoned(R * D)
        a = _attn_args(pb, d_pool, d_table, d_q, d_len)
        a.part_o, a.part_ml = part_o.data_ptr(), part_ml.data_ptr()
        _lib.check(L.ssrhip_attn_decode_kv16(C.byref(a), d_land.data_ptr(), _lib.stream_ptr()))
        _lib.check(L.ssrhip_attn_combine(C.byref(a), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        results.append((case, _take(out, R * D).view(R, D), want, err_ref))
        assert torch.equal(d_pool.cpu(), HK.bf16_bits(pool))                           # the rounded entries were promoted into the pool
    _judge(f"attn_decode_kv16+combine/hd{hd}", results)
