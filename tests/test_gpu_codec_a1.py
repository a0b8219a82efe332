"""GPU: the opt-in bf16 codec activations (DESIGN I.32) — `ssrhip_codec_gemm_a1`, `ssrhip_resblock_a1` and everything wired to them.

GEMM: a value that already IS a bf16 value splits into itself and two zeros, and the two products the new kernels leave out add +-0 to an
accumulator that starts at +0. So `ssrhip_codec_gemm_a1` on x must equal, bit for bit on whole poisoned buffers, `ssrhip_codec_gemm_w1`
without ELU on load on bf16(E), where E is x, or the library's own elu1(x) for the ELU-on-load forms (taken from `ssrhip_gemm`'s fp32 chain
with an identity matrix and ELU on store: x . 1 plus zeros is exact, and ELU on store is the bit-identical twin of ELU on load).

Residual block: both operands are made inside the kernel, so there is no identity. Every output is held to an fp64 emulation of the
rounding (`_emulate_resblock`) with a slack of its own that covers operands so close to a bf16 rounding boundary that the kernel may
round them the other way; two conditions keep the slack from hiding a failure.

Whole codec: streams equal the one pass, ragged items the batch-1 decode, the counter rises for the bf16-activation model alone, the
default is launch for launch what it was, and the distance from fp32 activations is bounded against the distance the rounded weights
already put between the one-plane model and the fp32 one."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel
from test_gpu_codec_w1 import ELU_SHAPES, PAD, POISON, RES_TOL, STREAM_TOL, TOL, _form, _problem, _ref64, _resblock_case, _tm_folded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ELU = _lib.ACT_NONE, _lib.ACT_ELU
U_BF16 = 2.0 ** -8            # unit roundoff of round-to-nearest bf16 (8 significant bits: half a spacing of 2^-7 at the bottom of a binade)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


# ------------------------------------------------------------------------------------------ GEMM
def _library_elu(L, A, K):
    """elu1(A[..., :K]) as the library computes it: ssrhip_gemm's fp32 chain (no planes) with the identity matrix and ELU on store"""
    batch, M, lda = A.shape
    eye = torch.eye(K, device="cuda")
    out = torch.empty(batch, M, K, device="cuda")
    a = _lib.GemmArgs()
    a.A, a.W, a.C = A.data_ptr(), eye.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act_out = M, K, K, lda, K, ELU
    if batch > 1:
        a.batch, a.strideA, a.strideC = batch, M * lda, M * K
    _lib.check(L.ssrhip_gemm(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


def _rounding_bound(A, Wt, K, act_in):
    """What rounding every activation operand to bf16 can move an output by, per output: |bf16(e) - e| <= 2^-8 |e|, so the sum moves by at
    most 2^-8 sum_k |e_k| |w_k| (ELU on store is 1-Lipschitz, a residual is added behind it unchanged) — plus TOL, the one-plane
    kernel's own bound against fp64. A sanity bound against the UNROUNDED product; the identity is the test."""
    x = A[..., :K].double()
    return U_BF16 * ((F.elu(x) if act_in == ELU else x).abs() @ Wt.double().abs().t()) + TOL


def _launch(L, entry, A, K, Wt, one, b, c0, act_in, residual, act_out, tm=None, want_tmf=None):
    """one launch of a one-plane entry into a poisoned buffer with ldc = N + 8 and a pad behind it -> the whole buffer"""
    batch, M, lda = A.shape
    N = Wt.shape[0]
    ldc = N + 8
    buf = torch.full((batch * M * ldc + PAD,), POISON, device="cuda")
    if residual:
        buf[:batch * M * ldc].view(batch, M, ldc)[:, :, :N] = c0
    a = _lib.GemmArgs()
    a.A, a.W, a.C, a.bias = A.data_ptr(), Wt.data_ptr(), buf.data_ptr(), b.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.residual = M, N, K, lda, ldc, residual
    a.act_in, a.act_out = act_in, act_out
    if batch > 1:
        a.batch, a.strideA, a.strideC = batch, M * lda, M * ldc
    if tm is not None:
        a.tm_c, a.tm_lo, a.tm_hi = tm
        if want_tmf is not None:
            assert _tm_folded(M, N, K, batch, ldc, M * ldc if batch > 1 else 0, tm[0], buf.data_ptr(), residual) is want_tmf
    a.W_split = one.data_ptr()
    rc = entry(C.byref(a), _lib.stream_ptr())
    assert rc == 0, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    return buf


def _identity(L, A, Wt, b, c0, K, act_in, residual=0, act_out=NONE, tm=None, want_tmf=None):
    """(the a1 launch on A, the w1 launch without ELU on load on bf16(E), the w1 launch on A itself, the view [batch][M][N] of the first)"""
    batch, M, _ = A.shape
    N = Wt.shape[0]
    one = Wt.to(torch.bfloat16).contiguous()
    E = _library_elu(L, A, K) if act_in == ELU else A[..., :K].contiguous()
    Er = E.to(torch.bfloat16).float().contiguous()
    assert not torch.equal(Er, E)                                          # the operands are NOT bf16 values to begin with
    n0, w0 = L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()
    ya = _launch(L, L.ssrhip_codec_gemm_a1, A, K, Wt, one, b, c0, act_in, residual, act_out, tm, want_tmf)
    assert (L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()) == (n0 + 1, w0)          # one per launch, and the other counter stands
    yw = _launch(L, L.ssrhip_codec_gemm_w1, Er, K, Wt, one, b, c0, NONE, residual, act_out, tm, want_tmf)
    yx = _launch(L, L.ssrhip_codec_gemm_w1, A, K, Wt, one, b, c0, act_in, residual, act_out, tm, want_tmf)
    assert (L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()) == (n0 + 1, w0 + 2)
    ldc = N + 8
    return ya, yw, yx, ya[:batch * M * ldc].view(batch, M, ldc)[:, :, :N]


@pytest.mark.parametrize("act_out", [NONE, ELU], ids=["store", "elu-on-store"])
@pytest.mark.parametrize("residual", [0, 1], ids=["plain", "residual"])
@pytest.mark.parametrize("act_in", [NONE, ELU], ids=["raw", "elu-on-load"])
@pytest.mark.parametrize("M,N,K,bm", ELU_SHAPES, ids=[f"{m}-{n}-{k}" for m, n, k, _ in ELU_SHAPES])
def test_gemm_identity(L, M, N, K, bm, act_in, residual, act_out):
    assert _form(M, N, K) == bm
    A, Wt, b, c0 = _problem(M, N, K)
    ya, yw, yx, got = _identity(L, A, Wt, b, c0, K, act_in, residual, act_out)
    ref = _ref64(A, Wt, b, c0, K, act_in, residual, act_out)
    print(f"M={M} N={N} K={K} act_in={act_in} res={residual} act_out={act_out} (BM {bm}): max |a1 - w1 on bf16(E)| = {float((ya - yw).abs().max()):.3e}, "
          f"max |a1 - w1 on x| = {float((ya - yx).abs().max()):.3e}, max |a1 - fp64 of the unrounded product| = {float((got.double() - ref).abs().max()):.3e}")
    assert torch.equal(ya, yw)                                             # whole buffers: the ldc padding and the pad included
    assert not torch.equal(ya, yx)                                         # ... and the rounding really happened
    pad_cols = ya[:M * (N + 8)].view(M, N + 8)[:, N:]
    assert bool((pad_cols == POISON).all()) and bool((ya[M * (N + 8):] == POISON).all())
    assert torch.isfinite(got).all()
    assert bool(((got.double() - ref).abs() <= _rounding_bound(A, Wt, K, act_in) + TOL * ref.abs()).all())


def test_gemm_identity_batched_strided(L):
    M, N, K, lda = 700, 260, 136, 144
    A, Wt, b, c0 = _problem(M, N, K, batch=3, lda=lda)
    for act_in in (NONE, ELU):
        ya, yw, yx, _ = _identity(L, A, Wt, b, c0, K, act_in, 1, ELU)
        assert torch.equal(ya, yw) and not torch.equal(ya, yx), act_in


def test_gemm_identity_with_the_time_mask(L):
    """tm_c = N (time row = m) on whole 128-row tiles: the launches take the 16-byte epilogue with the mask folded in — the plan
    conditions are asserted for the shape. Same bits, and nothing outside [tm_lo, tm_hi) is written."""
    M, N, K = 12300, 520, 72
    A, Wt, b, c0 = _problem(M, N, K, seed=5)
    lo, hi = 3, M - 5
    ya, yw, yx, got = _identity(L, A, Wt, b, c0, K, ELU, 0, NONE, tm=(N, lo, hi), want_tmf=True)
    assert torch.equal(ya, yw) and not torch.equal(ya, yx)
    assert bool((got[0, :lo] == POISON).all()) and bool((got[0, hi:] == POISON).all()) and torch.isfinite(got[0, lo:hi]).all()


@pytest.mark.parametrize("act_in", [NONE, ELU], ids=["raw", "elu-on-load"])
def test_gemm_identity_with_a_transposed_convolutions_time_mask(L, act_in):
    """tm_c = N / 2, two items: an output row holds TWO time rows, as a stride-2 transposed convolution's GEMM does; time rows outside
    [3, 2 M - 5) of either item stay poison."""
    M, N, K, B = 12300, 520, 72, 2
    A, Wt, b, c0 = _problem(M, N, K, batch=B, seed=9)
    lo, hi = 3, 2 * M - 5
    ya, yw, yx, got = _identity(L, A, Wt, b, c0, K, act_in, 0, NONE, tm=(N // 2, lo, hi), want_tmf=True)
    assert torch.equal(ya, yw) and not torch.equal(ya, yx)
    rows = got.contiguous().view(B, 2 * M, N // 2)
    assert bool((rows[:, :lo] == POISON).all()) and bool((rows[:, hi:] == POISON).all()) and torch.isfinite(rows[:, lo:hi]).all()


def test_4wave_forms_in_a_child_process():
    """SSRHIP_GEMM_SPLIT_DMA=0 is read once per process: the 4-wave kernels (both tile shapes, K shorter than a tile; raw and ELU on load)
    run the identity, plain store, in a fresh child."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                          "test_gemm_identity and plain and store and not elu-on-store and (raw or elu-on-load) and not time and not batched"],
                         env=dict(os.environ, SSRHIP_GEMM_SPLIT_DMA="0"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 6, out.stdout[-1500:]


@pytest.mark.parametrize("N,K", [(64, 64), (256, 68)], ids=["N64", "K68"])
def test_a_gemm_that_does_not_qualify_answers_1_and_launches_nothing(L, N, K):
    M = 200
    A, Wt, b, c0 = _problem(M, N, K)
    one = Wt.to(torch.bfloat16).contiguous()
    y = torch.full((M * N + PAD,), POISON, device="cuda")
    a = _lib.GemmArgs()
    a.A, a.W, a.bias, a.C = A.data_ptr(), Wt.data_ptr(), b.data_ptr(), y.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = M, N, K, K, N, ELU
    a.W_split = one.data_ptr()
    n0 = L.ssrhip_codec_a1_launches()
    assert L.ssrhip_codec_gemm_a1(C.byref(a), _lib.stream_ptr()) == 1
    assert L.ssrhip_codec_gemm_w1(C.byref(a), _lib.stream_ptr()) == 1      # the twin's condition
    torch.cuda.synchronize()
    assert bool((y == POISON).all()) and L.ssrhip_codec_a1_launches() == n0


# ------------------------------------------------------------------------------------------ residual block
def _bf16_grid(v):
    """(v rounded to bf16 nearest-even, the bf16 spacing at v, the distance of v to the nearest rounding boundary) for an fp64 tensor.
    The rounding goes through fp32 as the kernel's operand does; a value whose fp64 -> fp32 step decides the side lies within an fp32
    ulp of the boundary and is covered by the slack."""
    r = v.float().to(torch.bfloat16).double()
    _, ex = torch.frexp(v)                                                 # |v| = m 2^ex, m in [0.5, 1): bf16 keeps 8 significant bits
    spacing = torch.ldexp(torch.ones_like(v), ex - 8)
    dist = (spacing / 2 - (v - r).abs()).clamp_min(0.0)
    return r, spacing, dist


ELU_ERR2 = 2.4e-7                  # twice elu1's stated absolute error (csrc/common.h: 1.2e-7)


def _emulate_resblock(x, w3, w1, b3, b1, T, out_act):
    """fp64 emulation of the bf16-activation block and the slack of every output:
      stage 1: an ELU(x) operand within 2.4e-7 of a boundary may flip; its spacing goes into S1 = |W3| . U1 + RES_TOL;
      stage 2: an ELU(H + b3) operand within S1 of a boundary may flip; its spacing plus S1 goes into slack = |W1| . U2 + RES_TOL.
    ELU on store is 1-Lipschitz: the slack holds behind it as it is. Also returns the fp64 evaluation of the UNROUNDED block."""
    xd = x.double()
    win = lambda t: torch.cat([t[:, 0:T], t[:, 1:T + 1], t[:, 2:T + 2]], dim=2)     # noqa: E731  [B][T][3C]: taps t-1, t, t+1
    e = F.elu(xd)
    er, sp1, d1 = _bf16_grid(e)
    u1 = torch.where(d1 <= ELU_ERR2, sp1, torch.zeros_like(sp1))
    w3d, w1d = w3.double(), w1.double()
    s1 = win(u1) @ w3d.abs().t() + RES_TOL
    v = F.elu(win(er) @ w3d.t() + b3.double())
    vr, sp2, d2 = _bf16_grid(v)
    u2 = torch.where(d2 <= s1, sp2 + s1, torch.zeros_like(sp2))
    slack = u2 @ w1d.abs().t() + RES_TOL
    emu = xd[:, 1:T + 1] + vr @ w1d.t() + b1.double()
    exact = xd[:, 1:T + 1] + F.elu(win(e) @ w3d.t() + b3.double()) @ w1d.t() + b1.double()
    if out_act:
        emu, exact = F.elu(emu), F.elu(exact)
    return emu, slack, exact


@pytest.mark.parametrize("out_act", [NONE, ELU], ids=["store", "elu-on-store"])
@pytest.mark.parametrize("T", [1, 127, 128, 129, 1000])
@pytest.mark.parametrize("Cc", [64, 128])
def test_resblock_against_the_fp64_emulation(L, Cc, T, out_act):
    """Every output within its own slack of the emulation; at most 2 % of them farther than RES_TOL from it; and the kernel is closer
    (rms) to the emulation than to the fp64 evaluation of the unrounded block. One plane pointer without the other is a contract error."""
    B = 3
    x, w3, w1, b3, b1, _ = _resblock_case(Cc, T, B)
    emu, slack, exact = _emulate_resblock(x, w3, w1, b3, b1, T, out_act)
    Hh = Cc // 2
    kp = torch.arange(Hh)
    perm = 16 * (kp // 16) + (kp % 8) % 4 + 8 * ((kp % 8) // 4) + 4 * ((kp // 8) % 2)
    dx, dw3, dw1, db3, db1 = x.cuda(), w3.cuda(), w1.cuda(), b3.cuda(), b1.cuda()
    o3, o1 = dw3.to(torch.bfloat16).contiguous(), w1[:, perm].contiguous().cuda().to(torch.bfloat16).contiguous()
    y = torch.full((B * T * Cc + PAD,), POISON, device="cuda")
    a = _lib.ResblockArgs()
    a.x, a.y, a.w3, a.b3, a.w1, a.b1 = dx.data_ptr(), y.data_ptr(), dw3.data_ptr(), db3.data_ptr(), dw1.data_ptr(), db1.data_ptr()
    a.B, a.T, a.C, a.x_bstride, a.y_bstride, a.out_act = B, T, Cc, (T + 2) * Cc, T * Cc, out_act
    a.w3_split, a.w1_split = o3.data_ptr(), o1.data_ptr()
    n0, w0 = L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()
    rc = L.ssrhip_resblock_a1(C.byref(a), _lib.stream_ptr())
    assert rc == 0, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    assert (L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()) == (n0 + 1, w0)
    assert bool((y[B * T * Cc:] == POISON).all())
    got = y[:B * T * Cc].view(B, T, Cc).double().cpu()
    assert torch.isfinite(got).all()
    d = (got - emu).abs()
    share = float((d > RES_TOL).double().mean())
    rms_emu, rms_exact = float((got - emu).pow(2).mean().sqrt()), float((got - exact).pow(2).mean().sqrt())
    print(f"C={Cc} T={T} out_act={out_act}: worst |d| / slack = {float((d / slack).max()):.3f}, max |d| = {float(d.max()):.3e}, "
          f"share beyond RES_TOL = {share * 100:.2f} %, rms vs emulation {rms_emu:.3e}, rms vs the unrounded block {rms_exact:.3e}")
    assert bool((d <= slack).all()), float((d / slack).max())
    assert share <= 0.02, share
    assert rms_emu < rms_exact, (rms_emu, rms_exact)
    for drop in ("w3_split", "w1_split"):
        full = getattr(a, drop)
        setattr(a, drop, 0)
        assert L.ssrhip_resblock_a1(C.byref(a), _lib.stream_ptr()) < 0, drop
        setattr(a, drop, full)


def test_resblock_a1_answers_1_at_256_channels_and_writes_nothing(L):
    Cc, T, B = 256, 129, 2
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T + 2, Cc, generator=g).cuda()
    w3 = torch.randn(Cc // 2, 3 * Cc, generator=g).to(torch.bfloat16).cuda()
    w1 = torch.randn(Cc, Cc // 2, generator=g).to(torch.bfloat16).cuda()
    w3f, w1f, b3, b1 = w3.float(), w1.float(), torch.zeros(Cc // 2, device="cuda"), torch.zeros(Cc, device="cuda")
    y = torch.full((B * T * Cc + PAD,), POISON, device="cuda")
    a = _lib.ResblockArgs()
    a.x, a.y, a.w3, a.b3, a.w1, a.b1 = x.data_ptr(), y.data_ptr(), w3f.data_ptr(), b3.data_ptr(), w1f.data_ptr(), b1.data_ptr()
    a.B, a.T, a.C, a.x_bstride, a.y_bstride = B, T, Cc, (T + 2) * Cc, T * Cc
    a.w3_split, a.w1_split = w3.data_ptr(), w1.data_ptr()
    n0 = L.ssrhip_codec_a1_launches()
    assert L.ssrhip_resblock_a1(C.byref(a), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all()) and L.ssrhip_codec_a1_launches() == n0


def test_resblock_with_the_ring_of_2_in_a_child_process():
    """SSRHIP_RESBLOCK_RING is read once per process; unset, the one-plane kernels take the ring of 4. The tile-boundary lengths with the
    ring of 2 in a fresh child."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                          "test_resblock_against_the_fp64_emulation and (129 or 1000) and elu-on-store"],
                         env=dict(os.environ, SSRHIP_RESBLOCK_RING="2"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 4, out.stdout[-1500:]


# ------------------------------------------------------------------------------------------ the whole codec
SEED = 11
FRAMES = 24


def _run_entries(L, cfg, m, wavs, codes, labels):
    """every dense entry point and `decode_ragged` of one model -> (outputs, bf16-activation launches, one-plane launches)"""
    n0, w0 = L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()
    o = {}
    for t, w in wavs.items():
        c, _, emb = m.encode(w)
        o[f"{t}.codes"], o[f"{t}.emb"] = c.clone(), emb.clone()
        o[f"{t}.decode"] = m.decode(codes[t]).clone()
        o[f"{t}.wmdecode"] = m.wmdecode(codes[t], labels[t], w[..., : codes[t].shape[-1] * cfg.hop])[0].clone()
        o[f"{t}.detect"] = m.detect_watermark(w).clone()
    rag = [codes["3x0.7s"][0:1, :, :20], codes["3x0.7s"][1:2], codes["1x0.3s"][0:1], codes["3x0.7s"][2:3, :, :7]]
    o["ragged"] = [y.clone() for y in m.decode_ragged(rag)]
    o["ragged1"] = [m.decode(c).clone() for c in rag]                       # the batch-1 decode of every ragged item
    torch.cuda.synchronize()
    return o, L.ssrhip_codec_a1_launches() - n0, L.ssrhip_codec_w1_launches() - w0


@pytest.fixture(scope="module", params=["tiny", "full"])
def models(request, L):
    """F: fp32, A: bf16 weights (one plane), R: bf16 weights and bf16 activations; their outputs on 1 x 0.3 s and 3 x 0.7 s of seeded
    noise — computed once, never modified."""
    cfg = W.codec_config_full() if request.param == "full" else W.codec_config_tiny()
    sd = W.codec_state_dict(cfg, seed=SEED)
    assert "SSRHIP_CODEC_W1" not in os.environ
    Fm = WMEncodecModel(cfg, sd, "cuda")
    A = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
    R = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16", act_dtype="bf16")
    assert (Fm.act_dtype, A.act_dtype, R.act_dtype) == ("fp32", "fp32", "bf16")
    assert R.one_plane and R.bf16_acts and A.one_plane and not A.bf16_acts and not Fm.bf16_acts
    g = torch.Generator().manual_seed(SEED)
    n = lambda secs: int(secs * cfg.sample_rate) // cfg.hop * cfg.hop      # noqa: E731  whole frames (`wmdecode` takes the waveform of its codes)
    wavs = {"1x0.3s": (torch.randn(1, 1, n(0.3), generator=g) * 0.3).cuda(), "3x0.7s": (torch.randn(3, 1, n(0.7), generator=g) * 0.3).cuda()}
    codes = {t: Fm.encode(w)[0].clone() for t, w in wavs.items()}               # every model decodes the SAME codes
    labels = {t: torch.randint(0, 2, (c.shape[0], c.shape[-1]), generator=g).cuda() for t, c in codes.items()}
    outs, a1, w1 = {}, {}, {}
    for name, m in (("F", Fm), ("A", A), ("R", R)):
        outs[name], a1[name], w1[name] = _run_entries(L, cfg, m, wavs, codes, labels)
    return dict(name=request.param, cfg=cfg, F=Fm, A=A, R=R, outs=outs, a1=a1, w1=w1, codes=codes, labels=labels, wavs=wavs)


def test_whole_codec_takes_the_new_path_and_only_where_asked(models):
    print(f"{models['name']}: bf16-activation launches per model {models['a1']}, one-plane launches {models['w1']}")
    assert models["a1"]["R"] > 0 and models["a1"]["A"] == 0 and models["a1"]["F"] == 0
    assert models["w1"]["R"] == 0 and models["w1"]["A"] == models["a1"]["R"] and models["w1"]["F"] == 0      # entry for entry where A takes the twin
    for n in ("F", "A", "R"):
        assert models[n].mallocs_in_flight == 0, n
    # the plane buffers are the one-plane model's
    ca, cr = models["A"]._plane_cache, models["R"]._plane_cache
    assert len(ca) == len(cr) and all(t.dtype == torch.bfloat16 for v in cr.values() for t in (v if isinstance(v, tuple) else (v,)))
    for k in sorted(models["outs"]["R"]):
        for t in (models["outs"]["R"][k] if isinstance(models["outs"]["R"][k], list) else [models["outs"]["R"][k]]):
            assert torch.isfinite(t.double()).all(), k


def test_ragged_items_equal_the_batch_1_decode(models):
    for n in ("A", "R"):
        for i, (y, want) in enumerate(zip(models["outs"][n]["ragged"], models["outs"][n]["ragged1"])):
            err = float((y - want).abs().max())
            print(f"{models['name']} model {n} ragged item {i}: max |ragged - batch-1 decode| = {err:.3g}")
            assert y.shape == want.shape and err <= STREAM_TOL, (n, i, err)


def test_distance_from_fp32_activations_is_bounded_by_the_rounded_weights(models):
    """d_w = relative rms waveform difference of the one-plane model against fp32, d_a = that of the bf16-activation model against the
    one-plane model, same inputs: 0 < d_a <= 4 d_w (every rounded product rounds one more operand with the same unit roundoff at the same
    sites; 4 is margin over the expected ~1). Synthetic weights: not judged on a real checkpoint. The share of RVQ codes is reported."""
    o = models["outs"]
    for t in models["wavs"]:
        for entry in ("decode", "wmdecode"):
            f, a, r = (o[n][f"{t}.{entry}"].double() for n in ("F", "A", "R"))
            d_w = float((a - f).pow(2).mean().sqrt() / f.pow(2).mean().sqrt())
            d_a = float((r - a).pow(2).mean().sqrt() / a.pow(2).mean().sqrt())
            print(f"{models['name']} {t} {entry}: d_w (bf16 weights vs fp32) = {d_w:.4e}, d_a (bf16 activations vs bf16 weights) = {d_a:.4e}, d_a / d_w = {d_a / d_w:.2f}")
            assert 0.0 < d_a <= 4.0 * d_w, (t, entry, d_a, d_w)
        cr, ca = o["R"][f"{t}.codes"], o["A"][f"{t}.codes"]
        print(f"{models['name']} {t} encode: {float((cr != ca).double().mean()) * 100:.2f} % of {ca.numel()} RVQ codes differ between bf16 activations and "
              f"bf16 weights; first codebook {float((cr[:, 0] != ca[:, 0]).double().mean()) * 100:.2f} %")
        assert not torch.equal(o["R"][f"{t}.emb"], o["A"][f"{t}.emb"])


def test_decode_stream_chunks_equal_the_one_pass(L, models):
    R, cfg = models["R"], models["cfg"]
    codes = models["codes"]["3x0.7s"][1:2, :, :FRAMES]
    want = R.decode(codes).clone()
    st = R.decode_stream(FRAMES + 3)
    n0, w0 = L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()
    got = torch.cat([st.push(codes[..., t: t + 7]) for t in range(0, FRAMES, 7)] + [st.finish()], -1)
    assert L.ssrhip_codec_a1_launches() > n0 and L.ssrhip_codec_w1_launches() == w0
    assert got.shape == want.shape == (1, 1, FRAMES * cfg.hop) and torch.equal(got, want), float((got - want).abs().max())
    assert R.mallocs_in_flight == 0


def test_wmdecode_stream_chunks_equal_the_one_pass(L, models):
    R, cfg = models["R"], models["cfg"]
    hop = cfg.hop
    codes, labels = models["codes"]["3x0.7s"][2:3, :, :FRAMES], models["labels"]["3x0.7s"][2:3, :FRAMES]
    wav = models["wavs"]["3x0.7s"][2:3, :, : FRAMES * hop]
    want = R.wmdecode(codes, labels, wav, with_mark=False)[0].clone()
    st = R.wmdecode_stream(FRAMES + 3)
    n0 = L.ssrhip_codec_a1_launches()
    got = torch.cat([st.push(codes[..., t: t + 7], labels[0, t: t + 7], wav[..., t * hop: (t + 7) * hop]) for t in range(0, FRAMES, 7)] + [st.finish()], -1)
    assert L.ssrhip_codec_a1_launches() > n0
    assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())
    assert R.mallocs_in_flight == 0


_DEFAULT_CHILD = """
import hashlib, os, sys, torch, ssr_speech_amd
from ssr_speech_amd import _lib, weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel
kw = eval(sys.argv[1])
cfg = W.codec_config_full()
sd = W.codec_state_dict(cfg, seed=11)
m = WMEncodecModel(cfg, sd, "cuda", **kw)
built = m.n_launches
g = torch.Generator().manual_seed(11)
h = hashlib.md5()
for B, secs in ((1, 0.3), (3, 0.7)):
    w = (torch.randn(B, 1, int(secs * cfg.sample_rate), generator=g) * 0.3).cuda()
    codes, _, emb = m.encode(w)
    lab = torch.randint(0, 2, (B, codes.shape[-1]), generator=g).cuda()
    outs = [codes, emb, m.decode(codes), *m.wmdecode(codes, lab, w[..., : codes.shape[-1] * cfg.hop]), m.detect_watermark(w)]
    for o in outs:
        h.update(o.detach().cpu().contiguous().numpy().tobytes())
torch.cuda.synchronize()
L = _lib.lib()
log = open(os.environ["SSRHIP_GEMM_LOG"], "rb").read()
print("RESULT", built, m.n_launches, len(log.splitlines()), hashlib.md5(log).hexdigest(), h.hexdigest(), m.sizing_passes, m.mallocs_in_flight,
      len(m._plane_cache), L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches())
"""


@pytest.mark.parametrize("wdt", ["fp32", "bf16"])
def test_the_default_is_launch_for_launch_what_it_was(tmp_path, wdt):
    """One fresh process per arm, full config, every dense entry point on 1 x 0.3 s and 3 x 0.7 s: a model built WITHOUT the new keyword and
    one built with act_dtype="fp32" give the same library-call counts, the same GEMM launch log (SSRHIP_GEMM_LOG: M N K batch grid
    split-or-chain per launch), the same output digest, the same planes — and not one bf16-activation launch."""
    res = {}
    for arm, kw in (("nokw", dict(weight_dtype=wdt)), ("fp32acts", dict(weight_dtype=wdt, act_dtype="fp32"))):
        log = tmp_path / f"{arm}.log"
        out = subprocess.run([sys.executable, "-c", _DEFAULT_CHILD, repr(kw)], env=dict(os.environ, SSRHIP_GEMM_LOG=str(log)), cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        res[arm] = re.search(r"RESULT (.*)", out.stdout).group(1).split()
        print(f"weight_dtype={wdt} {arm}: n_launches build {res[arm][0]} total {res[arm][1]} | gemm log {res[arm][2]} lines md5 {res[arm][3]} | outputs md5 "
              f"{res[arm][4]} | sizing_passes {res[arm][5]} mallocs_in_flight {res[arm][6]} | planes {res[arm][7]} | a1 launches {res[arm][8]} w1 launches {res[arm][9]}")
    assert res["nokw"] == res["fp32acts"]
    assert res["nokw"][8] == "0" and res["nokw"][6] == "0" and (int(res["nokw"][9]) > 0) == (wdt == "bf16")
    if wdt == "fp32":
        # what the commit before the keyword launches for this workload, as recorded in profiles/codec_w1_ab.md ("launch for launch"):
        # 94 library calls while the model is built, 514 in all, 144 GEMM launches, 74 plane-cache entries
        assert res["nokw"][:3] == ["94", "514", "144"] and res["nokw"][7] == "74", res["nokw"]
