"""GPU: the one-plane split GEMM (csrc/gemm_split.hip ssrhip_gemm_w1, DESIGN I.13) and everything wired to it.

A weight that IS a bf16 value splits exactly into itself and two planes of zeros. `ssrhip_gemm` on those three planes issues six matrix
products per k block, three of them against zeros; `ssrhip_gemm_w1` on the one plane issues the other three, in the same order, in the same
tiles, through the same epilogues. The claim is IDENTITY: `torch.equal`, on whole poisoned buffers, from one launch up to the tokens of an
830M engine. Every weight here is rounded to bf16 on the host, every activation is finite."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -777.25
PAD = 64                      # poisoned floats behind every output buffer
TOL = 3e-5                    # the bound of tests/test_gpu_kernels.py test_gemm_split_bf16x3_is_as_accurate_as_the_fp32_chain
NONE, RELU, GELU = _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU_ERF


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def _planes(L, Wd):
    """(the three planes of the exact split [3 N K] int16, the one plane [N K] int16) of a bf16-valued fp32 matrix on the device"""
    three = torch.empty(3 * Wd.numel(), dtype=torch.int16, device="cuda")
    _lib.check(L.ssrhip_split_weights(Wd.data_ptr(), three.data_ptr(), Wd.numel(), _lib.stream_ptr()))
    one = Wd.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
    torch.cuda.synchronize()
    assert torch.equal(three[:Wd.numel()], one) and not bool(three[Wd.numel():].any())   # plane 0 = the weight, planes 1 and 2 = zeros
    return three, one


def _form(M, N, K, batch=1):
    """the tile shape csrc/gemm_split.hip plan_gemm_split picks (restated: the test names which form a shape is there for)"""
    tiles128 = ((N + 127) // 128) * ((M + 127) // 128) * batch
    w128, w64 = (M + 127) // 128 * 128 - M, (M + 63) // 64 * 64 - M
    half_empty = w128 - w64 >= 64 and 8 * (w128 - w64) >= M
    return 128 if tiles128 >= 384 and not half_empty else 64


def _problem(M, N, K, batch=1, bias=True, seed=None):
    """seeded operands on the device: A [batch][M][K], W [N][K] rounded to bf16, bias [N], c0 [batch][M][N]"""
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    A = torch.randn(batch, M, K, generator=g).cuda()
    Wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).float().cuda()
    b = torch.randn(N, generator=g).cuda() if bias else None
    c0 = torch.randn(batch, M, N, generator=g).cuda()
    return A, Wt, b, c0


def _run_pair(L, A, Wt, b, c0, act=NONE, residual=0, tm=None):
    """ssrhip_gemm on the three planes and ssrhip_gemm_w1 on the one plane, into poisoned buffers with ldc = N + 8 and a pad behind them.
    Returns (three-plane buffer, one-plane buffer, the view [batch][M][N] of the second)."""
    batch, M, K = A.shape
    N = Wt.shape[0]
    ldc = N + 8
    three, one = _planes(L, Wt)
    base = torch.full((batch * M * ldc + PAD,), POISON, device="cuda")
    if residual:
        base[:batch * M * ldc].view(batch, M, ldc)[:, :, :N] = c0
    outs = []
    for planes, entry in ((three, L.ssrhip_gemm), (one, L.ssrhip_gemm_w1)):
        buf = base.clone()
        a = _lib.GemmArgs()
        a.A, a.W, a.C = A.data_ptr(), Wt.data_ptr(), buf.data_ptr()
        a.bias = b.data_ptr() if b is not None else 0
        a.M, a.N, a.K, a.lda, a.ldc, a.act, a.residual = M, N, K, K, ldc, act, residual
        if batch > 1:
            a.batch, a.strideA, a.strideC = batch, M * K, M * ldc
        if tm is not None:
            a.tm_c, a.tm_lo, a.tm_hi = tm
        a.W_split = planes.data_ptr()
        rc = entry(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (rc, L.ssrhip_last_error())
        torch.cuda.synchronize()
        outs.append(buf)
    return outs[0], outs[1], outs[1][:batch * M * ldc].view(batch, M, ldc)[:, :, :N]


def _ref64(A, Wt, b, c0, act, residual):
    ref = A.double() @ Wt.double().t()
    if b is not None:
        ref = ref + b.double()
    ref = F.relu(ref) if act == RELU else (F.gelu(ref) if act == GELU else ref)
    return c0.double() + ref if residual else ref


def _check_identity(L, M, N, K, act, residual, bm):
    assert _form(M, N, K) == bm
    A, Wt, b, c0 = _problem(M, N, K)
    y3, y1, got = _run_pair(L, A, Wt, b, c0, act, residual)
    ref = _ref64(A, Wt, b, c0, act, residual)
    e3 = float((y3[:M * (N + 8)].view(1, M, N + 8)[:, :, :N].double() - ref).abs().max())
    print(f"M={M} N={N} K={K} act={act} res={residual} (BM {bm}): max |three planes - fp64| = {e3:.3e}, "
          f"max |one plane - fp64| = {float((got.double() - ref).abs().max()):.3e}, max |one - three| = {float((y1 - y3).abs().max()):.3e}")
    assert torch.equal(y1, y3)                                            # whole buffers: the ldc padding and the pad included
    pad_cols = y1[:M * (N + 8)].view(M, N + 8)[:, N:]
    assert bool((pad_cols == POISON).all()) and bool((y1[M * (N + 8):] == POISON).all())
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref.float(), rtol=TOL, atol=TOL)       # (the three-plane buffer is the same bits)


# (M, N, K, act, residual, the tile rows it is there for)
SHAPES = [
    pytest.param(12300, 520, 72, NONE, 0, 128, id="12300-520-72"),        # DMA128: tiles128 = 5 x 97 >= 384, ragged M and N tile, K = two tiles + 8
    pytest.param(300, 200, 64, RELU, 0, 64, id="300-200-64"),             # DMA64, ragged
    pytest.param(77, 1030, 8, GELU, 0, 64, id="77-1030-8"),               # K shorter than one tile
    pytest.param(598, 2048, 8192, NONE, 1, 64, id="598-2048-8192-ffn2"),  # the LM's FFN2 + residual: the longest accumulation
    pytest.param(598, 6144, 2048, NONE, 0, 64, id="598-6144-2048-qkv"),   # the QKV shape, with bias
    # the activation sweep of test_gemm_split_bf16x3_is_as_accurate_as_the_fp32_chain on the two small tile shapes
    pytest.param(12300, 520, 72, GELU, 1, 128, id="sweep-12300-gelu-res"),
    pytest.param(12300, 520, 72, RELU, 0, 128, id="sweep-12300-relu"),
    pytest.param(300, 200, 64, NONE, 1, 64, id="sweep-300-none-res"),
    pytest.param(300, 200, 64, GELU, 0, 64, id="sweep-300-gelu"),
    pytest.param(598, 8192, 2048, RELU, 0, 64, id="sweep-598-8192-2048-ffn1"),
]


@pytest.mark.parametrize("M,N,K,act,residual,bm", SHAPES)
def test_kernel_identity(L, M, N, K, act, residual, bm):
    """One launch: the same bits as the three-plane launch in the whole poisoned buffer, and both within 3e-5 of a torch fp64 product."""
    _check_identity(L, M, N, K, act, residual, bm)


def test_kernel_identity_batched_strided(L):
    M, N, K = 700, 260, 136
    assert _form(M, N, K, 3) == 64
    A, Wt, b, c0 = _problem(M, N, K, batch=3)
    y3, y1, got = _run_pair(L, A, Wt, b, c0, RELU, 1)
    assert torch.equal(y1, y3)
    torch.testing.assert_close(got, _ref64(A, Wt, b, c0, RELU, 1).float(), rtol=TOL, atol=TOL)


def test_kernel_identity_time_masked(L):
    """A time-masked call: the three-plane launch folds the mask into its 16-byte epilogue (128-row tiles, N % tm_c == 0), the one-plane
    launch has no such instantiation and takes the general per-element loop. Same bits, and nothing outside [tm_lo, tm_hi) is written."""
    M, N, K = 12300, 520, 72
    A, Wt, b, c0 = _problem(M, N, K, seed=5)
    lo, hi = 3, M - 5
    y3, y1, got = _run_pair(L, A, Wt, b, c0, NONE, 0, tm=(N, lo, hi))      # tm_c = N: time row u = m
    assert torch.equal(y1, y3)
    assert bool((got[0, :lo] == POISON).all()) and bool((got[0, hi:] == POISON).all())
    torch.testing.assert_close(got[0, lo:hi], _ref64(A, Wt, b, c0, NONE, 0)[0, lo:hi].float(), rtol=TOL, atol=TOL)


def test_kernel_identity_in_plain_tile_order(L, monkeypatch):
    """SSRHIP_GEMM_XCD=0 (read at every launch): the plain blockIdx tile order against the XCD-aware default — four buffers, one result."""
    M, N, K = 12300, 520, 72
    A, Wt, b, c0 = _problem(M, N, K)
    d3, d1, _ = _run_pair(L, A, Wt, b, c0, GELU, 1)
    monkeypatch.setenv("SSRHIP_GEMM_XCD", "0")
    p3, p1, _ = _run_pair(L, A, Wt, b, c0, GELU, 1)
    assert torch.equal(p1, p3) and torch.equal(p1, d1) and torch.equal(d1, d3)


def test_4wave_forms_in_a_child_process():
    """SSRHIP_GEMM_SPLIT_DMA=0 is read once per process: the 4-wave kernels (both tile shapes, K shorter than a tile) run the first three
    identity cases in a fresh child."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                          "test_kernel_identity and (12300-520-72 or 300-200-64 or 77-1030-8) and not sweep"],
                         env=dict(os.environ, SSRHIP_GEMM_SPLIT_DMA="0"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 3, out.stdout[-1500:]


@pytest.mark.parametrize("N,K,act_in", [(64, 64, NONE), (256, 68, NONE), (256, 64, _lib.ACT_ELU)], ids=["N64", "K68", "elu-on-load"])
def test_a_call_that_does_not_qualify_answers_1_and_launches_nothing(L, N, K, act_in):
    M = 200
    A, Wt, b, c0 = _problem(M, N, K)
    one = Wt.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
    y = torch.full((M * N + PAD,), POISON, device="cuda")
    a = _lib.GemmArgs()
    a.A, a.W, a.bias, a.C = A.data_ptr(), Wt.data_ptr(), b.data_ptr(), y.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = M, N, K, K, N, act_in
    a.W_split = one.data_ptr()
    assert L.ssrhip_gemm_w1(C.byref(a), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    a.W_split = 0                                                          # what the caller does next: the fp32 chain on the master
    _lib.check(L.ssrhip_gemm(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    x = F.elu(A[0]) if act_in == _lib.ACT_ELU else A[0]
    torch.testing.assert_close(y[:M * N].view(M, N), (x.double() @ Wt.double().t() + b.double()).float(), rtol=TOL, atol=TOL)
    assert bool((y[M * N:] == POISON).all())


def test_a_null_plane_is_a_contract_error(L):
    a = _lib.GemmArgs()
    a.A, a.W, a.C = 0x1000, 0x2000, 0x3000                                 # never dereferenced: answered before any HIP call
    a.M, a.N, a.K, a.lda, a.ldc = 256, 256, 64, 64, 256
    assert L.ssrhip_gemm_w1(C.byref(a), _lib.stream_ptr()) < 0
    assert b"W_split" in L.ssrhip_last_error()


# ------------------------------------------------------------------------------------------ engine
def _bf16_arena(args, sd, w1):
    """a bf16 arena whose planes were built with the switch SSRHIP_PREFILL_W1 = `w1` in the environment (it is read there and only there)"""
    arena = LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="bf16")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SSRHIP_PREFILL_W1", w1)
        mp.delenv("SSRHIP_PREFILL_SPLIT", raising=False)
        assert arena.ensure_split_planes() and arena.ensure_head_split_planes()
    assert arena.split_planes == (1 if w1 == "1" else 3)
    return arena


@pytest.fixture(scope="module")
def tiny():
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    sd = W.lm_state_dict(args, seed=21, device="cuda")
    return args, sd, {3: _bf16_arena(args, sd, "0"), 1: _bf16_arena(args, sd, "1")}


def _prompt(args, gen, Lt, T, greedy, seed, vocab_text=30):
    x = torch.randint(0, vocab_text, (Lt,), generator=gen).numpy()
    unc = torch.randint(0, vocab_text + 1, (Lt,), generator=gen).numpy()
    y = torch.randint(0, args.audio_vocab_size, (T, 4), generator=gen)
    cated, _, num_task, _ = LY.build_layout(y.T.numpy(), np.asarray([[T, T]]), args)
    kn = DecodeKnobs(top_k=1 if greedy else 40, top_p=1.0 if greedy else 0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2,
                     use_cfg=True, text_len=Lt, n_spans=num_task, seed=seed)
    return [x, unc], cated, kn


def test_the_one_plane_arena_holds_a_third_of_the_bytes(tiny):
    _, _, arenas = tiny
    a3, a1 = arenas[3], arenas[1]
    for l3, l1 in zip(a3.layers, a1.layers):
        for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
            n = l1[name + "_w"].numel()
            assert l1[name + "_ws"].dtype == torch.int16 and l1[name + "_ws"].numel() == n and l3[name + "_ws"].numel() == 3 * n
            assert torch.equal(l1[name + "_ws"], l3[name + "_ws"][:n]) and not bool(l3[name + "_ws"][n:].any())
    assert a1.head1_ws.numel() == a1.head1_w.numel() and a1.head2_ws.numel() == a1.head2_w.numel()
    assert a3.split_plane_bytes() == 3 * a1.split_plane_bytes() > 0


def test_prefill_and_decode_equal_the_three_plane_engine(tiny):
    """2-row engine, a 200-position prompt: the whole (poisoned) KV pool, the prefill's x, the first step's x and the page table after
    `start`, then 24 steps, greedy and sampled."""
    args, _, arenas = tiny
    for greedy in (True, False):
        got = {}
        for np_, arena in arenas.items():
            eng = DecodeEngine(arena, 1, True, 512, 64)
            try:
                assert eng.prefill_planes == np_
                eng.kv_pool.fill_(POISON)
                rows, cated, kn = _prompt(args, torch.Generator().manual_seed(31), 40, 160, greedy, 7)
                n0 = eng.lib.ssrhip_gemm_w1_launches()
                eng.start(rows, [cated], [kn], noise=None)
                torch.cuda.synchronize()
                # every layer GEMM of the one-plane engine's prefill LAUNCHED a one-plane kernel (not the silent fp32-chain fallback)
                assert eng.lib.ssrhip_gemm_w1_launches() - n0 == (4 * arena.L if np_ == 1 else 0)
                after = (eng.kv_pool.clone(), eng._prefill_ws["x"].clone(), eng.x.clone(), eng.page_table.clone())
                eng.decode(24, use_graph=True)
                torch.cuda.synchronize()
                got[np_] = after + (eng.generated[:, :24].clone(), eng.kv_pool.clone())
            finally:
                eng.close()
        assert bool((got[1][0] != POISON).any()) and torch.isfinite(got[1][1]).all()
        for i, what in enumerate(("KV pool after the prefill", "prefill x", "x of the first step", "page table", "tokens", "KV pool after 24 steps")):
            assert torch.equal(got[1][i], got[3][i]), (what, greedy)


@pytest.mark.parametrize("two_phase", ["0", "1"], ids=["blocking-admission", "two-phase-admission"])
def test_run_queue_admission_equals_the_three_plane_engine(tiny, monkeypatch, two_phase):
    """10-row engine (5 utterances with CFG), 6 jobs: the sixth is admitted into a freed slot — by the blocking admission (the default) and,
    under SSRHIP_ADMIT_TWO_PHASE=1 (read by `run_queue`), by the two-phase admission's prefill on the side stream, which runs on the same
    context the one-plane setter was called on."""
    args, _, arenas = tiny
    monkeypatch.setenv("SSRHIP_ADMIT_TWO_PHASE", two_phase)
    outs = {}
    for np_, arena in arenas.items():
        gen = torch.Generator().manual_seed(41)
        jobs = []
        for i in range(6):
            rows, cated, kn = _prompt(args, gen, 8 + i, 150 - 20 * i, True, 50 + i)
            jobs.append(dict(text_rows=rows, audio_cols=cated, gen=None, cap=20 + 12 * i, knobs=kn))
        eng = DecodeEngine(arena, 5, True, 512, 256)
        try:
            n0 = eng.lib.ssrhip_gemm_w1_launches()
            res = eng.run_queue(jobs, chunk=16, sampling=False)
            assert eng.lib.ssrhip_gemm_w1_launches() - n0 == (2 * 4 * arena.L if np_ == 1 else 0)      # the first fill and the one refill
            assert eng.n_admitted == 6 and eng.n_refills >= 1 and eng.prefill_planes == np_
            outs[np_] = [(int(st.done), int(st.n_steps), np.array(tok)) for st, tok in res]
        finally:
            eng.close()
    for (d1, n1, t1), (d3, n3, t3) in zip(outs[1], outs[3]):
        assert (d1, n1) == (d3, n3) and t1.shape[0] > 0 and np.array_equal(t1, t3)


def _collate(items, args):
    x = torch.nn.utils.rnn.pad_sequence([x for x, _ in items], batch_first=True, padding_value=args.text_pad_token)
    y = torch.nn.utils.rnn.pad_sequence([y.transpose(1, 0) for _, y in items], padding_value=args.audio_pad_token).permute(1, 2, 0)
    return dict(x=x, x_lens=torch.LongTensor([len(x) for x, _ in items]), y=y.contiguous(), y_lens=torch.LongTensor([y.shape[1] for _, y in items]))


def test_score_equals_the_three_plane_arena(monkeypatch):
    """`SSR_Speech.score` of a ragged 3-item batch: the arena built under the switch picks ssrhip_lm_score_w1 (layer and head planes)."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    sd = W.lm_state_dict(args, seed=23)
    g = torch.Generator().manual_seed(6)
    items = []
    for i in range(3):
        Lt, T = 9 + 5 * i, 90 + 37 * i
        y = torch.randint(0, args.audio_vocab_size, (args.n_codebooks, T), generator=g)
        y[:, T // 3] = args.mts
        y[:, 0] = args.sos
        items.append((torch.randint(0, args.text_vocab_size, (Lt,), generator=g), y))
    batch = _collate(items, args)
    monkeypatch.delenv("SSRHIP_PREFILL_SPLIT", raising=False)
    out = {}
    for w1 in ("0", "1"):
        monkeypatch.setenv("SSRHIP_PREFILL_W1", w1)
        m = SSR_Speech(args)
        m.load_state_dict(sd)
        m = m.to("cuda").eval()
        m.set_weight_dtype("bf16")
        n0 = _lib.lib().ssrhip_gemm_w1_launches()
        out[w1] = m.score(batch)
        a = m._arena
        # one chunk: four GEMMs per layer, head 1, head 2 of every codebook — all on one-plane kernels, or none
        assert _lib.lib().ssrhip_gemm_w1_launches() - n0 == ((4 * a.L + 1 + a.K) * m.last_score["chunks"] if w1 == "1" else 0)
        assert a.split_planes == (1 if w1 == "1" else 3) and a.head1_ws.numel() == a.split_planes * a.head1_w.numel()
        out[w1]["_nll"], out[w1]["_rank"] = m.last_score["nll"].clone(), m.last_score["rank"].clone()
    assert torch.isfinite(out["1"]["loss"]) and int(out["1"]["ntoken_by_item"].sum()) > 0
    for k in ("loss", "top10acc", "nll_by_item", "ntoken_by_item", "_nll", "_rank"):
        assert torch.equal(out["1"][k], out["0"][k]), k


def test_830m_prefill_and_greedy_steps_equal_the_three_plane_engine():
    """The bench prompt (598 prompt rows of a 2-row engine) at the 830M shape: the KV pool after the prefill, then 12 greedy steps."""
    args = W.lm_args_830m()
    sd = W.lm_state_dict(args, seed=0, device="cuda")
    g = torch.Generator().manual_seed(2024)
    Lt, T = 130, 160
    x = torch.randint(0, 100, (Lt,), generator=g).numpy()
    y = torch.randint(0, 2048, (T, 4), generator=g)
    unc = torch.randint(0, 101, (Lt,), generator=g).numpy()
    cated, _, num_task, _ = LY.build_layout(y.T.numpy(), np.asarray([[T, T]]), args)
    kn = DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, use_cfg=True, text_len=Lt, n_spans=num_task, seed=1)
    got = {}
    for w1 in ("0", "1"):
        arena = _bf16_arena(args, sd, w1)
        eng = DecodeEngine(arena, 1, True, 1024, 256, stream_w16=False)       # (no packed decode copies: this is about the prefill)
        try:
            eng.kv_pool.fill_(POISON)
            n0 = eng.lib.ssrhip_gemm_w1_launches()
            eng.start([x, unc], [cated], [kn], noise=None)
            torch.cuda.synchronize()
            assert eng.lib.ssrhip_gemm_w1_launches() - n0 == (4 * arena.L if w1 == "1" else 0)
            pool = eng.kv_pool.clone()
            eng.decode(12, use_graph=True)
            torch.cuda.synchronize()
            got[w1] = (pool, eng.generated[:, :12].clone(), arena.split_plane_bytes())
        finally:
            eng.close()
        del eng, arena
    assert bool((got["1"][0] != POISON).any())
    assert torch.equal(got["1"][0], got["0"][0])
    assert torch.equal(got["1"][1], got["0"][1])
    assert got["0"][2] == 3 * got["1"][2]
