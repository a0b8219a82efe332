"""GPU: the opt-in bf16-rounded codec (DESIGN I.30) — `ssrhip_codec_gemm_w1`, `ssrhip_resblock_w1` and everything wired to them.

A weight that IS a bf16 value splits exactly into itself and two planes of zeros. The three-plane entries issue six matrix products per
k block, three of them against zeros; the one-plane entries issue the other three, in the same order, in the same tiles, through the same
epilogues. The claim is IDENTITY: `torch.equal` on whole poisoned buffers, from one launch up to every entry point of a full-size codec
with `weight_dtype="bf16"`. Every weight here is rounded to bf16, every activation is finite. How far the rounded codec is from the fp32
one is REPORTED (test 8), not bounded: no real checkpoint is shipped to judge it on."""
import ctypes as C
import math
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -777.25
PAD = 64                      # poisoned floats behind every output buffer
TOL = 3e-5                    # tests/test_gpu_w1.py's bound, from test_gemm_split_bf16x3_is_as_accurate_as_the_fp32_chain
RES_TOL = 2e-5                # test_resblock_split_dma_kernel_matches_fp64's
STREAM_TOL = 2e-5             # tests/test_gpu_stream_batch.py: a batched stream against the batch-1 decode
NONE, ELU = _lib.ACT_NONE, _lib.ACT_ELU


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


# ------------------------------------------------------------------------------------------ GEMM
def _planes(L, Wd):
    """(the three planes of the exact split [3 N K] int16, the one plane [N K] int16) of a bf16-valued fp32 matrix on the device"""
    three = torch.empty(3 * Wd.numel(), dtype=torch.int16, device="cuda")
    _lib.check(L.ssrhip_split_weights(Wd.data_ptr(), three.data_ptr(), Wd.numel(), _lib.stream_ptr()))
    one = Wd.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
    torch.cuda.synchronize()
    assert torch.equal(three[:Wd.numel()], one) and not bool(three[Wd.numel():].any())   # plane 0 = the weight, planes 1 and 2 = zeros
    return three, one


def _form(M, N, K, batch=1):
    """the tile rows csrc/gemm_split.hip plan_gemm_split picks (restated: the test names which form a shape is there for)"""
    tiles128 = ((N + 127) // 128) * ((M + 127) // 128) * batch
    w128, w64 = (M + 127) // 128 * 128 - M, (M + 63) // 64 * 64 - M
    half_empty = w128 - w64 >= 64 and 8 * (w128 - w64) >= M
    return 128 if tiles128 >= 384 and not half_empty else 64


def _tm_folded(M, N, K, batch, ldc, strideC, tm_c, c_ptr, residual):
    """plan_gemm_split's `tmf` conditions, restated (the switches SSRHIP_EPILOGUE_TM / SSRHIP_EPILOGUE_WIDE / SSRHIP_GEMM_SPLIT_DMA at
    their defaults): the launch takes the kernel with the time mask folded into the 16-byte epilogue"""
    assert not any(os.environ.get(s, "1").startswith("0") for s in ("SSRHIP_EPILOGUE_TM", "SSRHIP_EPILOGUE_WIDE", "SSRHIP_GEMM_SPLIT_DMA"))
    return (_form(M, N, K, batch) == 128 and tm_c > 0 and N % tm_c == 0 and tm_c % 4 == 0 and not residual and ldc % 4 == 0
            and strideC % 4 == 0 and c_ptr % 16 == 0 and M * (N // tm_c) < 0x7FFFFFFF)


def _problem(M, N, K, batch=1, lda=None, seed=None):
    """seeded operands on the device: A [batch][M][lda] (columns K.. are never read), W [N][K] rounded to bf16, bias [N], c0 [batch][M][N]"""
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    A = torch.randn(batch, M, lda or K, generator=g).cuda()
    Wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).float().cuda()
    b = torch.randn(N, generator=g).cuda()
    c0 = torch.randn(batch, M, N, generator=g).cuda()
    return A, Wt, b, c0


def _run_pair(L, A, Wt, b, c0, K, act_in=ELU, residual=0, act_out=NONE, tm=None, want_tmf=None):
    """ssrhip_gemm on the three planes and ssrhip_codec_gemm_w1 on the one plane, into poisoned buffers with ldc = N + 8 and a pad behind
    them. Returns (three-plane buffer, one-plane buffer, the view [batch][M][N] of the second)."""
    batch, M, lda = A.shape
    N = Wt.shape[0]
    ldc = N + 8
    three, one = _planes(L, Wt)
    base = torch.full((batch * M * ldc + PAD,), POISON, device="cuda")
    if residual:
        base[:batch * M * ldc].view(batch, M, ldc)[:, :, :N] = c0
    outs = []
    n0 = L.ssrhip_codec_w1_launches()
    for planes, entry in ((three, L.ssrhip_gemm), (one, L.ssrhip_codec_gemm_w1)):
        buf = base.clone()
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
        a.W_split = planes.data_ptr()
        rc = entry(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (rc, L.ssrhip_last_error())
        torch.cuda.synchronize()
        outs.append(buf)
    assert L.ssrhip_codec_w1_launches() == n0 + 1                          # the one-plane kernel ran, once
    return outs[0], outs[1], outs[1][:batch * M * ldc].view(batch, M, ldc)[:, :, :N]


def _ref64(A, Wt, b, c0, K, act_in, residual, act_out):
    x = A[..., :K].double()
    ref = (F.elu(x) if act_in == ELU else x) @ Wt.double().t() + b.double()
    if residual:
        ref = c0.double() + ref
    return F.elu(ref) if act_out == ELU else ref


# (M, N, K, the tile rows it is there for)
ELU_SHAPES = [(12300, 520, 72, 128),      # the 128-row DMA tile: 5 x 97 tiles >= 384, ragged M and N tile, K = two tiles + 8
              (300, 200, 64, 64),         # the 64-row tile, ragged
              (77, 1030, 8, 64)]          # K shorter than one tile


@pytest.mark.parametrize("act_out", [NONE, ELU], ids=["store", "elu-on-store"])
@pytest.mark.parametrize("residual", [0, 1], ids=["plain", "residual"])
@pytest.mark.parametrize("M,N,K,bm", ELU_SHAPES, ids=[f"{m}-{n}-{k}" for m, n, k, _ in ELU_SHAPES])
def test_gemm_identity_with_elu_on_load(L, M, N, K, bm, residual, act_out):
    """One launch with act_in = ELU: the same bits as the three-plane launch in the whole poisoned buffer, both within 3e-5 of fp64."""
    assert _form(M, N, K) == bm
    A, Wt, b, c0 = _problem(M, N, K)
    y3, y1, got = _run_pair(L, A, Wt, b, c0, K, ELU, residual, act_out)
    ref = _ref64(A, Wt, b, c0, K, ELU, residual, act_out)
    e3 = float((y3[:M * (N + 8)].view(1, M, N + 8)[:, :, :N].double() - ref).abs().max())
    print(f"M={M} N={N} K={K} res={residual} act_out={act_out} (BM {bm}): max |three planes - fp64| = {e3:.3e}, "
          f"max |one plane - fp64| = {float((got.double() - ref).abs().max()):.3e}, max |one - three| = {float((y1 - y3).abs().max()):.3e}")
    assert torch.equal(y1, y3)                                            # whole buffers: the ldc padding and the pad included
    pad_cols = y1[:M * (N + 8)].view(M, N + 8)[:, N:]
    assert bool((pad_cols == POISON).all()) and bool((y1[M * (N + 8):] == POISON).all())
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref.float(), rtol=TOL, atol=TOL)       # (the three-plane buffer is the same bits)


def test_gemm_identity_batched_strided(L):
    M, N, K, lda = 700, 260, 136, 144
    A, Wt, b, c0 = _problem(M, N, K, batch=3, lda=lda)
    y3, y1, got = _run_pair(L, A, Wt, b, c0, K, ELU, 1, ELU)
    assert torch.equal(y1, y3)
    torch.testing.assert_close(got, _ref64(A, Wt, b, c0, K, ELU, 1, ELU).float(), rtol=TOL, atol=TOL)


def test_gemm_identity_with_the_time_mask(L):
    """tm_c = N (time row = m) on whole 128-row tiles: BOTH launches take the 16-byte epilogue with the mask folded in — the plan
    conditions are asserted for the shape. Same bits, and nothing outside [tm_lo, tm_hi) is written."""
    M, N, K = 12300, 520, 72
    A, Wt, b, c0 = _problem(M, N, K, seed=5)
    lo, hi = 3, M - 5
    y3, y1, got = _run_pair(L, A, Wt, b, c0, K, ELU, 0, NONE, tm=(N, lo, hi), want_tmf=True)
    assert torch.equal(y1, y3)
    assert bool((got[0, :lo] == POISON).all()) and bool((got[0, hi:] == POISON).all())
    torch.testing.assert_close(got[0, lo:hi], _ref64(A, Wt, b, c0, K, ELU, 0, NONE)[0, lo:hi].float(), rtol=TOL, atol=TOL)


@pytest.mark.parametrize("act_in", [NONE, ELU], ids=["raw", "elu-on-load"])
def test_gemm_identity_with_a_transposed_convolutions_time_mask(L, act_in):
    """tm_c = N / 2, two items: an output row holds TWO time rows, as a stride-2 transposed convolution's GEMM does; time rows outside
    [3, 2 M - 5) of either item stay poison."""
    M, N, K, B = 12300, 520, 72, 2
    A, Wt, b, c0 = _problem(M, N, K, batch=B, seed=9)
    lo, hi = 3, 2 * M - 5
    y3, y1, got = _run_pair(L, A, Wt, b, c0, K, act_in, 0, NONE, tm=(N // 2, lo, hi), want_tmf=True)
    assert torch.equal(y1, y3)
    rows = got.contiguous().view(B, 2 * M, N // 2)
    assert bool((rows[:, :lo] == POISON).all()) and bool((rows[:, hi:] == POISON).all())
    ref = _ref64(A, Wt, b, c0, K, act_in, 0, NONE).view(B, 2 * M, N // 2)
    torch.testing.assert_close(rows[:, lo:hi], ref[:, lo:hi].float(), rtol=TOL, atol=TOL)


def test_4wave_forms_in_a_child_process():
    """SSRHIP_GEMM_SPLIT_DMA=0 is read once per process: the 4-wave kernels (both tile shapes, K shorter than a tile) run the three
    shapes of the ELU-on-load identity, plain store, in a fresh child."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                          "test_gemm_identity_with_elu_on_load and plain and store and not elu-on-store"],
                         env=dict(os.environ, SSRHIP_GEMM_SPLIT_DMA="0"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 3, out.stdout[-1500:]


@pytest.mark.parametrize("N,K", [(64, 64), (256, 68)], ids=["N64", "K68"])
def test_a_gemm_that_does_not_qualify_answers_1_and_launches_nothing(L, N, K):
    M = 200
    A, Wt, b, c0 = _problem(M, N, K)
    one = Wt.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
    y = torch.full((M * N + PAD,), POISON, device="cuda")
    a = _lib.GemmArgs()
    a.A, a.W, a.bias, a.C = A.data_ptr(), Wt.data_ptr(), b.data_ptr(), y.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = M, N, K, K, N, ELU
    a.W_split = one.data_ptr()
    n0 = L.ssrhip_codec_w1_launches()
    assert L.ssrhip_codec_gemm_w1(C.byref(a), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all()) and L.ssrhip_codec_w1_launches() == n0
    a.W_split = 0                                                          # what the caller does next: the fp32 chain on the master
    _lib.check(L.ssrhip_gemm(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:M * N].view(M, N), (F.elu(A[0].double()) @ Wt.double().t() + b.double()).float(), rtol=TOL, atol=TOL)
    assert bool((y[M * N:] == POISON).all())


_SPLIT0_CHILD = """
import ctypes as C, torch, ssr_speech_amd
from ssr_speech_amd import _lib
L = _lib.lib()
M, N, K = 200, 256, 64
A, Wt = torch.randn(M, K, device="cuda"), torch.randn(N, K, device="cuda").bfloat16()
y = torch.full((M * N + 64,), -777.25, device="cuda")
a = _lib.GemmArgs()
a.A, a.W, a.C, a.W_split = A.data_ptr(), Wt.float().data_ptr(), y.data_ptr(), Wt.data_ptr()
a.M, a.N, a.K, a.lda, a.ldc, a.act_in = M, N, K, K, N, _lib.ACT_ELU
rc = L.ssrhip_codec_gemm_w1(C.byref(a), _lib.stream_ptr())
torch.cuda.synchronize()
print("answer", rc, "untouched", bool((y == -777.25).all()), "launches", L.ssrhip_codec_w1_launches())
"""


def test_gemm_split_0_answers_1_in_a_child_process():
    """SSRHIP_GEMM_SPLIT=0 (read once per process): a call that would qualify answers 1 with the poisoned buffer untouched."""
    out = subprocess.run([sys.executable, "-c", _SPLIT0_CHILD], env=dict(os.environ, SSRHIP_GEMM_SPLIT="0"), cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "answer 1 untouched True launches 0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_a_null_plane_is_a_contract_error(L):
    a = _lib.GemmArgs()
    a.A, a.W, a.C = 0x1000, 0x2000, 0x3000                                 # never dereferenced: answered before any HIP call
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = 256, 256, 64, 64, 256, ELU
    assert L.ssrhip_codec_gemm_w1(C.byref(a), _lib.stream_ptr()) < 0
    assert b"W_split" in L.ssrhip_last_error()


# ------------------------------------------------------------------------------------------ residual block
def _resblock_case(Cc, T, B=3):
    """seeded block: x [B][T + 2][C] with halo rows, w3 [C/2][3 C] and w1 [C][C/2] rounded to bf16, biases; + the fp64 evaluation"""
    g = torch.Generator().manual_seed(1000 * Cc + T)
    Hh = Cc // 2
    x = torch.randn(B, T + 2, Cc, generator=g)
    w3 = (torch.randn(Hh, 3 * Cc, generator=g) / math.sqrt(3 * Cc)).to(torch.bfloat16).float()
    w1 = (torch.randn(Cc, Hh, generator=g) / math.sqrt(Hh)).to(torch.bfloat16).float()
    b3, b1 = torch.randn(Hh, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1
    xd = x.double()
    win = torch.cat([xd[:, 0:T], xd[:, 1:T + 1], xd[:, 2:T + 2]], dim=2)          # [B][T][3C]: taps t-1, t, t+1
    hmid = F.elu(F.elu(win) @ w3.double().t() + b3.double())
    want = xd[:, 1:T + 1] + hmid @ w1.double().t() + b1.double()
    return x, w3, w1, b3, b1, want


def _resblock_pair(L, Cc, T, out_act, B=3):
    """ssrhip_resblock on three planes and ssrhip_resblock_w1 on one plane each, into poisoned buffers with a pad -> (y3, y1, want, args)"""
    x, w3, w1, b3, b1, want = _resblock_case(Cc, T, B)
    Hh = Cc // 2
    kp = torch.arange(Hh)
    perm = 16 * (kp // 16) + (kp % 8) % 4 + 8 * ((kp % 8) // 4) + 4 * ((kp // 8) % 2)
    dx, dw3, dw1, db3, db1 = x.cuda(), w3.cuda(), w1.cuda(), b3.cuda(), b1.cuda()
    dw1p = w1[:, perm].contiguous().cuda()
    p3 = torch.empty(3, Hh, 3 * Cc, dtype=torch.int16, device="cuda")
    p1 = torch.empty(3, Cc, Hh, dtype=torch.int16, device="cuda")
    _lib.check(L.ssrhip_split_weights(dw3.data_ptr(), p3.data_ptr(), dw3.numel(), _lib.stream_ptr()))
    _lib.check(L.ssrhip_split_weights(dw1p.data_ptr(), p1.data_ptr(), dw1p.numel(), _lib.stream_ptr()))
    o3, o1 = dw3.to(torch.bfloat16).contiguous(), dw1p.to(torch.bfloat16).contiguous()
    torch.cuda.synchronize()
    assert torch.equal(p3[0], o3.view(torch.int16)) and torch.equal(p1[0], o1.view(torch.int16)) and not bool(p3[1:].any()) and not bool(p1[1:].any())
    keep = (dx, dw3, dw1, db3, db1, p3, p1, o3, o1)
    outs = []
    n0 = L.ssrhip_codec_w1_launches()
    for planes, entry in (((p3, p1), L.ssrhip_resblock), ((o3, o1), L.ssrhip_resblock_w1)):
        y = torch.full((B * T * Cc + PAD,), POISON, device="cuda")
        a = _lib.ResblockArgs()
        a.x, a.y, a.w3, a.b3, a.w1, a.b1 = dx.data_ptr(), y.data_ptr(), dw3.data_ptr(), db3.data_ptr(), dw1.data_ptr(), db1.data_ptr()
        a.B, a.T, a.C, a.x_bstride, a.y_bstride, a.out_act = B, T, Cc, (T + 2) * Cc, T * Cc, out_act
        a.w3_split, a.w1_split = planes[0].data_ptr(), planes[1].data_ptr()
        rc = entry(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (rc, L.ssrhip_last_error())
        torch.cuda.synchronize()
        outs.append(y)
    assert L.ssrhip_codec_w1_launches() == n0 + 1
    return outs[0], outs[1], (F.elu(want) if out_act else want), a, keep


@pytest.mark.parametrize("out_act", [NONE, ELU], ids=["store", "elu-on-store"])
@pytest.mark.parametrize("T", [1, 127, 128, 129, 1000])
@pytest.mark.parametrize("Cc", [64, 128])
def test_resblock_identity(L, Cc, T, out_act):
    """The grid of test_resblock_split_dma_kernel_matches_fp64 (B = 3): the one-plane kernel's whole poisoned buffer equals the three-plane
    kernel's, both within 2e-5 of the fp64 evaluation; one plane pointer without the other is a contract error."""
    B = 3
    y3, y1, want, a, keep = _resblock_pair(L, Cc, T, out_act, B)
    got = y1[:B * T * Cc].view(B, T, Cc)
    print(f"C={Cc} T={T} out_act={out_act}: max |one plane - fp64| = {float((got.double().cpu() - want).abs().max()):.3e}, "
          f"max |one - three| = {float((y1 - y3).abs().max()):.3e}")
    assert torch.equal(y1, y3)
    assert bool((y1[B * T * Cc:] == POISON).all()) and torch.isfinite(got).all()
    torch.testing.assert_close(got.double().cpu(), want, rtol=RES_TOL, atol=RES_TOL)
    for drop in ("w3_split", "w1_split"):
        full = getattr(a, drop)
        setattr(a, drop, 0)
        assert L.ssrhip_resblock_w1(C.byref(a), _lib.stream_ptr()) < 0, drop
        setattr(a, drop, full)


def test_resblock_w1_answers_1_at_256_channels_and_writes_nothing(L):
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
    n0 = L.ssrhip_codec_w1_launches()
    assert L.ssrhip_resblock_w1(C.byref(a), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all()) and L.ssrhip_codec_w1_launches() == n0


@pytest.mark.parametrize("ring", ["2", "4"])
def test_resblock_identity_with_either_ring_in_a_child_process(ring):
    """SSRHIP_RESBLOCK_RING is read once per process. Unset, the three-plane kernels take the ring of 2 and the one-plane kernels the
    ring of 4: each value is the non-default ring of one of the two. The tile-boundary lengths of the identity grid in a fresh child."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                          "test_resblock_identity and not child and (129 or 1000) and elu-on-store"],
                         env=dict(os.environ, SSRHIP_RESBLOCK_RING=ring), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 4, out.stdout[-1500:]


# ------------------------------------------------------------------------------------------ the whole codec, full config
SEED = 11


def _matrices(m):
    """name -> every folded weight matrix a model keeps (and what is derived from one by a permutation only)"""
    out = {}
    nets = {"encoder": m.encoder, "decoder": m.decoder, "wmdecoder": m.wmdecoder, "skip_encoder": m.skip_encoder, "wm_encoder": m.wm_encoder}
    for nn, net in nets.items():
        for i, kind, obj, _ in net.nodes:
            if kind in ("conv", "convtr"):
                out[f"{nn}.{i}.W"] = obj.W
                if kind == "conv":
                    out[f"{nn}.{i}.Wraw"] = obj.Wraw
            elif kind == "res":
                out[f"{nn}.{i}.W3"], out[f"{nn}.{i}.W1"] = obj[0].W, obj[1].W
            elif kind == "lstm":
                for l, (wih, whh, _) in enumerate(obj.layers):
                    out[f"{nn}.{i}.wih{l}"], out[f"{nn}.{i}.whh{l}"] = wih, whh
                    if obj.packed[l] is not None:
                        out[f"{nn}.{i}.packed{l}"] = obj.packed[l]
    for j, c in enumerate(m.wm_proj):
        out[f"wm_proj{j}.W"], out[f"wm_cls{j}.Wa"] = c.W, m.wm_cls[j][0]
    out["wm_predictor.W"] = m.wm_predictor.W
    return out


def _fp32_state(m):
    """name -> what stays fp32 whatever the weight_dtype: biases, codebooks, |e|^2, the label table"""
    out = {"codebooks": m.codebooks, "e2": m.e2, "wm_table": m.wm_table, "wm_predictor.b": m.wm_predictor.b}
    nets = {"encoder": m.encoder, "decoder": m.decoder, "wmdecoder": m.wmdecoder, "skip_encoder": m.skip_encoder, "wm_encoder": m.wm_encoder}
    for nn, net in nets.items():
        for i, kind, obj, _ in net.nodes:
            if kind in ("conv", "convtr"):
                out[f"{nn}.{i}.b"] = obj.b
            elif kind == "res":
                out[f"{nn}.{i}.b3"], out[f"{nn}.{i}.b1"] = obj[0].b, obj[1].b
            elif kind == "lstm":
                for l, (_, _, bias) in enumerate(obj.layers):
                    out[f"{nn}.{i}.bias{l}"] = bias
    for j, c in enumerate(m.wm_proj):
        out[f"wm_proj{j}.b"] = c.b
    return out


def _plane_bytes(m):
    n = 0
    for v in m._plane_cache.values():
        for t in (v if isinstance(v, tuple) else (v,)):
            n += t.numel() * t.element_size()
    return n


@pytest.fixture(scope="module")
def trio(L):
    """A: bf16 with the default arm (one plane), B: bf16 with codec_w1 = 0 (three planes), F: fp32, D: built without the keyword; their
    outputs on 1 x 0.3 s and 3 x 0.7 s of seeded noise — computed once, never modified."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=SEED)
    assert "SSRHIP_CODEC_W1" not in os.environ
    torch.cuda.empty_cache()                                               # a cold allocator, as tests/test_gpu_codec.py's sizing test starts from
    A = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
    os.environ["SSRHIP_CODEC_W1"] = "0"
    try:
        B = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
    finally:
        del os.environ["SSRHIP_CODEC_W1"]
    Fm = WMEncodecModel(cfg, sd, "cuda", weight_dtype="fp32")
    D = WMEncodecModel(cfg, sd, "cuda")
    assert (A.weight_dtype, B.weight_dtype, Fm.weight_dtype, D.weight_dtype) == ("bf16", "bf16", "fp32", "fp32")
    assert A.one_plane and not B.one_plane and not Fm.one_plane and not D.one_plane
    g = torch.Generator().manual_seed(SEED)
    sr = cfg.sample_rate
    wavs = {"1x0.3s": (torch.randn(1, 1, int(0.3 * sr), generator=g) * 0.3).cuda(), "3x0.7s": (torch.randn(3, 1, int(0.7 * sr), generator=g) * 0.3).cuda()}
    codes = {t: Fm.encode(w)[0].clone() for t, w in wavs.items()}               # every model decodes the SAME codes
    labels = {t: torch.randint(0, 2, (c.shape[0], c.shape[-1]), generator=g).cuda() for t, c in codes.items()}
    outs, launches = {}, {}
    for name, m in (("A", A), ("B", B), ("F", Fm), ("D", D)):
        n0 = L.ssrhip_codec_w1_launches()
        o, seen = {}, 0

        def note(what):
            nonlocal seen
            if m.mallocs_in_flight != seen:
                print(f"model {name}: {m.mallocs_in_flight - seen} driver allocation(s) in flight during {what}")
                seen = m.mallocs_in_flight

        for t, w in wavs.items():
            c, _, emb = m.encode(w)
            note(f"encode {t}")
            o[f"{t}.codes"], o[f"{t}.emb"] = c.clone(), emb.clone()
            o[f"{t}.decode"] = m.decode(codes[t]).clone()
            note(f"decode {t}")
            wm_wav, mark = m.wmdecode(codes[t], labels[t], w[..., : codes[t].shape[-1] * cfg.hop])
            note(f"wmdecode {t}")
            o[f"{t}.wmdecode"], o[f"{t}.mark"] = wm_wav.clone(), mark.clone()
            o[f"{t}.detect"] = m.detect_watermark(w).clone()
            note(f"detect_watermark {t}")
        rag = [codes["3x0.7s"][0:1, :, :20], codes["3x0.7s"][1:2], codes["1x0.3s"][0:1], codes["3x0.7s"][2:3, :, :7]]
        for i, y in enumerate(m.decode_ragged(rag)):
            o[f"ragged{i}"] = y.clone()
        note("decode_ragged")
        torch.cuda.synchronize()
        outs[name], launches[name] = o, L.ssrhip_codec_w1_launches() - n0
    return dict(cfg=cfg, A=A, B=B, F=Fm, D=D, outs=outs, launches=launches, codes=codes, labels=labels, wavs=wavs)


def test_whole_codec_one_plane_equals_three_planes(trio):
    """Every dense entry point and `decode_ragged`: A (one plane) == B (three planes of the same rounded weights), bit for bit."""
    a, b = trio["outs"]["A"], trio["outs"]["B"]
    assert sorted(a) == sorted(b) and len(a) == 2 * 6 + 4
    for k in sorted(a):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))
        assert torch.isfinite(a[k].double()).all(), k


def test_whole_codec_takes_the_one_plane_path_and_only_where_asked(trio):
    n = trio["launches"]
    print("one-plane launches per model:", n)
    assert n["A"] > 0 and n["B"] == 0 and n["F"] == 0 and n["D"] == 0
    assert 3 * _plane_bytes(trio["A"]) == _plane_bytes(trio["B"]) == _plane_bytes(trio["F"])      # a third of the plane bytes
    assert all(t.dtype == torch.bfloat16 for v in trio["A"]._plane_cache.values() for t in (v if isinstance(v, tuple) else (v,)))
    assert trio["A"].mallocs_in_flight == 0 and trio["B"].mallocs_in_flight == 0


def test_whole_codec_weights_are_rounded_once_and_nothing_else_is(trio):
    ma, mf = _matrices(trio["A"]), _matrices(trio["F"])
    assert sorted(ma) == sorted(mf) and len(ma) > 40
    changed = 0
    for k in ma:
        assert torch.equal(ma[k], mf[k].to(torch.bfloat16).float()), k
        changed += int(not torch.equal(ma[k], mf[k]))
    assert changed == len(ma)                                              # every matrix really was rounded
    mb = _matrices(trio["B"])
    assert all(torch.equal(ma[k], mb[k]) for k in ma)
    sa, sf = _fp32_state(trio["A"]), _fp32_state(trio["F"])
    assert sorted(sa) == sorted(sf)
    for k in sa:
        assert torch.equal(sa[k], sf[k]), k
    # the class biases are DERIVED from the rounded matrix (fp64 product of W_b and ELU(embed), as for fp32), so they follow it
    for j in range(4):
        Wfull, E = trio["A"].wm_proj[j].W.cpu(), trio["A"].wm_table.shape[1]
        want = (F.elu(trio["A"].wm_table.cpu().double()) @ Wfull[:, Wfull.shape[1] - E:].double().t()).float()
        assert torch.equal(trio["A"].wm_cls[j][1].cpu(), want), j


def test_the_default_is_untouched(trio):
    """weight_dtype="fp32" == no keyword at all: same outputs bit for bit, no one-plane launch, three int16 planes per matrix."""
    f, d = trio["outs"]["F"], trio["outs"]["D"]
    for k in sorted(f):
        assert torch.equal(f[k], d[k]), k
    assert all(t.dtype == torch.int16 for v in trio["D"]._plane_cache.values() for t in (v if isinstance(v, tuple) else (v,)))
    assert len(trio["D"]._plane_cache) == len(trio["F"]._plane_cache) and _plane_bytes(trio["D"]) == _plane_bytes(trio["F"])


def test_how_far_the_rounded_codec_is_from_fp32(trio):
    """A report, not a tolerance (synthetic weights; not judged on a real checkpoint): relative rms difference of the waveform decoded
    from the same codes, and the share of RVQ codes that differ on the same audio."""
    a, f = trio["outs"]["A"], trio["outs"]["F"]
    for t in trio["wavs"]:
        for entry in ("decode", "wmdecode"):
            da, df = a[f"{t}.{entry}"].double(), f[f"{t}.{entry}"].double()
            rel = float((da - df).pow(2).mean().sqrt() / df.pow(2).mean().sqrt())
            print(f"{t} {entry}: relative rms difference bf16 vs fp32 = {rel:.4e}")
            assert torch.isfinite(da).all() and rel > 0.0
        ca, cf = a[f"{t}.codes"], f[f"{t}.codes"]
        print(f"{t} encode: {float((ca != cf).double().mean()) * 100:.2f} % of {cf.numel()} RVQ codes differ; first codebook "
              f"{float((ca[:, 0] != cf[:, 0]).double().mean()) * 100:.2f} %")
        assert not torch.equal(a[f"{t}.emb"], f[f"{t}.emb"]) and torch.isfinite(a[f"{t}.emb"]).all()


# ------------------------------------------------------------------------------------------ streams
FRAMES = 24


def test_decode_stream_on_the_one_plane_codec(L, trio):
    """`decode_stream` on A: chunks concatenated == A's one-pass `decode`, bit for bit (as tests/test_gpu_stream.py asserts for fp32), and
    the windows ran one-plane kernels."""
    A, cfg = trio["A"], trio["cfg"]
    codes = trio["codes"]["3x0.7s"][1:2, :, :FRAMES]
    want = A.decode(codes).clone()
    st = A.decode_stream(FRAMES + 3)
    n0 = L.ssrhip_codec_w1_launches()
    chunks = [st.push(codes[..., t: t + 7]) for t in range(0, FRAMES, 7)] + [st.finish()]
    got = torch.cat(chunks, -1)
    assert L.ssrhip_codec_w1_launches() > n0
    assert got.shape == want.shape == (1, 1, FRAMES * cfg.hop) and torch.equal(got, want), float((got - want).abs().max())


def test_wmdecode_stream_on_the_one_plane_codec(L, trio):
    """`wmdecode_stream` on A == A's `wmdecode(..., with_mark=False)`, bit for bit (as tests/test_gpu_wmstream.py asserts for fp32)."""
    A, cfg = trio["A"], trio["cfg"]
    hop = cfg.hop
    codes, labels = trio["codes"]["3x0.7s"][2:3, :, :FRAMES], trio["labels"]["3x0.7s"][2:3, :FRAMES]
    wav = trio["wavs"]["3x0.7s"][2:3, :, : FRAMES * hop]
    want = A.wmdecode(codes, labels, wav, with_mark=False)[0].clone()
    st = A.wmdecode_stream(FRAMES + 3)
    n0 = L.ssrhip_codec_w1_launches()
    chunks = [st.push(codes[..., t: t + 7], labels[0, t: t + 7], wav[..., t * hop: (t + 7) * hop]) for t in range(0, FRAMES, 7)] + [st.finish()]
    got = torch.cat(chunks, -1)
    assert L.ssrhip_codec_w1_launches() > n0
    assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())


def test_decode_stream_batch_on_the_one_plane_codec(L, trio):
    """One `decode_stream_batch` of 2 items on A: per item, A's batch-1 `decode` without the prompt part, within the 2e-5 that
    tests/test_gpu_stream_batch.py holds a batched stream to."""
    A, cfg = trio["A"], trio["cfg"]
    hop = cfg.hop
    prompts, new = (5, 9), (FRAMES - 5, FRAMES - 9)
    codes = [trio["codes"]["3x0.7s"][u: u + 1, :, :FRAMES] for u in range(2)]
    st = A.decode_stream_batch(prompts, max(new) + 2)
    n0 = L.ssrhip_codec_w1_launches()
    st.push_prompts([codes[u][0, :, :prompts[u]] for u in range(2)])
    done, got = [0, 0], [[], []]
    while not all(st.ended):
        take = [min(8, new[u] - done[u]) for u in range(2)]
        ended = [not st.ended[u] and new[u] - done[u] <= 8 for u in range(2)]
        out = st.advance(take, ended, codes=[codes[u][0, :, prompts[u] + done[u]: prompts[u] + done[u] + take[u]] for u in range(2)])
        for u in range(2):
            got[u].append(out[u])
            done[u] += take[u]
    assert L.ssrhip_codec_w1_launches() > n0
    for u in range(2):
        want = A.decode(codes[u])[..., prompts[u] * hop:]
        y = torch.cat(got[u], -1)
        err = float((y - want).abs().max())
        print(f"item {u}: max |stream - batch-1 decode| = {err:.3g}")
        assert y.shape == want.shape == (1, 1, new[u] * hop) and err <= STREAM_TOL, (u, err)
