"""GPU: the bf16 weight stream of the 17..32-row decode step (csrc/gemv_mfma32_w16.hip, DESIGN.md Part I.12).

bf16 -> fp32 is a 16-bit shift and exact, and the bf16-stream kernels run the two-panel fp32 kernels' MFMA sequence on the same launch plan,
so every comparison between the two is `torch.equal`: launch by launch against `ssrhip_gemv` at the same row count on the fp32
streaming-order copy of the rounded master (whole output buffers with a poisoned pad behind them, whole KV pools), step by step between an
engine that streams the packed copies and one that streams the masters, and end to end through the public surface. The launch-level
outputs are also held against a torch fp64 product built from the UNPACKED PACKED BUFFER (a check that does not depend on the fp32 kernel)
with the bound tests/test_gpu_kernels.py::test_gemv_mfma_rows_matches_torch and tests/test_gpu_rows32.py apply to these kernels in fp32
(3e-5); the fp32 launch on the same inputs is held to the same bound in the same test, so a failure of both points at the inputs and not at
the new kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena, from_wt16_order, to_streaming_order, to_wt16_order
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

POISON = -777.25
PAD = 64                      # poisoned floats behind every output buffer: a stray store shows in the whole-buffer comparison
TOL = 3e-5                    # tests/test_gpu_kernels.py::test_gemv_mfma_rows_matches_torch, tests/test_gpu_rows32.py


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


LN, NONE = _lib.PRO_LAYERNORM, _lib.PRO_NONE
# (G, N, K, prologue, activation, epilogue): the shapes of tests/test_gpu_wt16.py that 17..32 rows take (no LayerNorm beyond K = 2048) —
# the smallest that reach each kernel form on 256 CUs, and the step's own
SHAPES = [
    (1, 6144, 2048, LN, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),       # 3 units per workgroup: a full tile + an 8-row duplicate tile, cross-tile refill, KV append
    (1, 8192, 2048, LN, _lib.ACT_RELU, _lib.EPI_STORE),            # FFN1
    (1, 4096, 2048, LN, _lib.ACT_GELU_ERF, _lib.EPI_STORE),        # head-MLP1
    (1, 2048, 2048, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, x in registers
    (1, 2048, 8192, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, streaming
    (4, 2056, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain form without prologue: groups, 4 waves, 257 units
    (2, 52, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # N % 8 = 4: zero-padded unit, partial 4-row store
    (1, 2064, 2112, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain streaming form (258 units > CUs); 132 k-steps: partial / empty wave slices
    (1, 24, 4096, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # the streaming pair form over two 16-step groups per wave
]
H, HD, N_LAYER, LAYER, MAX_PAGES = 16, 128, 2, 1, 2
# both sides of the page edge at 128, in panel 0 (rows 0..15) and in panel 1 (rows 16..31; row 16 is all of panel 1 at B = 17)
KV_POS = [127, 128, 5, 255, 0, 129, 64, 126, 200, 1, 130, 254, 77, 128, 127, 3,
          128, 127, 129, 0, 255, 126, 31, 128, 2, 127, 199, 254, 130, 65, 127, 128]


@functools.lru_cache(maxsize=None)
def _weights(G, N, K):
    """one rounded master per shape, shared by every case of that shape and never modified: (fp32 streaming-order copy, packed bf16 copy,
    the packed copy unpacked again [G][N][K], bias)"""
    seed = N * 7 + K + G
    master = W.make_tensor(f"wt32.{G}.{N}.{K}", (G, N, K), f"lin:{K}", seed, device="cuda").to(torch.bfloat16).float().contiguous()
    packed = to_wt16_order(master)
    unpacked = from_wt16_order(packed, N)
    assert torch.equal(unpacked, master)                                  # the packed buffer holds the rounded master exactly
    bias = torch.randn(G, N, generator=torch.Generator().manual_seed(seed)).cuda()
    return to_streaming_order(master), packed, unpacked, bias


def _to_panels(t):
    """[16 < B <= 32][Kw] -> the paneled tiled layout (include/ssrhip.h SSRHIP_TILED_P): two panels of [Kw/4][16][4], rows >= B poisoned"""
    B, Kw = t.shape
    out = torch.full((2, Kw // 4, 16, 4), POISON, device=t.device)
    for p in range(2):
        rows = t[16 * p:min(B, 16 * p + 16)]
        out[p, :, :rows.shape[0], :] = rows.reshape(rows.shape[0], Kw // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def _from_panels(buf, B, Kw):
    return buf.view(2, Kw // 4, 16, 4).permute(0, 2, 1, 3).reshape(32, Kw)[:B]


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "paneled"])
@pytest.mark.parametrize("B", [17, 27, 32])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_wt32_launch_is_bit_identical_to_the_fp32_launch_on_the_rounded_weights(L, B, G, N, K, pro, act, epi, tiled):
    Wt, packed, Wu, bias = _weights(G, N, K)
    g = torch.Generator().manual_seed(B * 100003 + N * 7 + K + pro)
    qkv = epi == _lib.EPI_QKV_APPEND
    y_tiled = tiled and not qkv                                            # the q output of the QKV launch is always row-major
    x = (torch.randn(B, G * K, generator=g) * 1.5 + 0.3).cuda()
    ny = K if qkv else G * N                                              # floats per row of y (q of the QKV launch)
    yv = (torch.randn(B, ny, generator=g) if epi == _lib.EPI_RESIDUAL else torch.full((B, ny), POISON)).cuda()
    xbuf = _to_panels(x) if tiled else x.reshape(-1).clone()
    y0 = torch.cat([_to_panels(yv) if y_tiled else yv.reshape(-1), torch.full((PAD,), POISON, device="cuda")])
    n_y = y0.numel() - PAD
    pool0 = torch.full((B * MAX_PAGES + 1, N_LAYER, 2, H, _lib.PAGE, HD) if qkv else (1,), POISON, device="cuda")
    table = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES).to(torch.int32).cuda()     # shuffled physical pages
    pos_l = KV_POS[:B]
    pos = torch.tensor(pos_l, dtype=torch.int32).cuda()

    def run(use_wt32):
        y, pool = y0.clone(), pool0.clone()
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = Wt.data_ptr(), bias.data_ptr(), xbuf.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
        a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
        a.x_tiled, a.y_tiled, a.w_tiled = tiled, int(y_tiled), 1
        if qkv:
            a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, N_LAYER, H, HD)
            a.layer, a.kv_pos = LAYER, pos.data_ptr()
        if use_wt32:
            assert L.ssrhip_gemv_wt32_applicable(C.byref(a)) == 1
            rc = L.ssrhip_gemv_wt32(C.byref(a), packed.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (rc, L.ssrhip_last_error())
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y, pool

    y16, pool16 = run(True)
    y32, pool32 = run(False)
    assert torch.equal(y16, y32), float((y16 - y32).abs().max())          # whole buffers, poisoned rows and pad included
    assert torch.equal(pool16, pool32)
    assert torch.equal(y16[n_y:], y0[n_y:])                               # the pad is untouched
    if y_tiled:                                                           # ... and so are the columns >= B of panel 1
        assert bool((y16[:n_y].view(2, ny // 4, 16, 4)[1, :, B - 16:, :] == POISON).all())
    # ---- independent of the fp32 kernel: torch fp64 on the unpacked packed buffer
    xin = x.view(B, G, K).double()
    if pro == LN:
        xin = F.layer_norm(xin, (K,), None, None, 1e-5)
    ref = torch.stack([F.linear(xin[:, k], Wu[k].double(), bias[k].double()) for k in range(G)], 1)          # [B][G][N]
    ref = F.relu(ref) if act == _lib.ACT_RELU else (F.gelu(ref) if act == _lib.ACT_GELU_ERF else ref)
    ref = ref.reshape(B, G * N)
    if epi == _lib.EPI_RESIDUAL:
        ref = ref + yv.double()
    errs = {}
    for name, y, pool in (("wt32", y16, pool16), ("fp32", y32, pool32)):
        got = _from_panels(y[:n_y], B, ny) if y_tiled else y[:n_y].view(B, ny)
        assert torch.isfinite(got).all(), name
        if qkv:
            err = float((got.double() - ref[:, :K]).abs().max())
            untouched = torch.ones_like(pool0, dtype=torch.bool)
            for b in range(B):
                page = int(table[b, pos_l[b] // _lib.PAGE])
                for which in (0, 1):
                    row = pool[page, LAYER, which, :, pos_l[b] % _lib.PAGE, :].reshape(-1)
                    err = max(err, float((row.double() - ref[b, (1 + which) * K:(2 + which) * K]).abs().max()))
                untouched[page, LAYER, :, :, pos_l[b] % _lib.PAGE, :] = False
            assert torch.equal(pool[untouched], pool0[untouched]), name   # nothing but the appended positions was written
        else:
            err = float((got.double() - ref).abs().max())
        errs[name] = err
    print(f"B={B} G={G} N={N} K={K} pro={pro} tiled={tiled}: max |wt32 - fp64| = {errs['wt32']:.3e}, max |fp32 - fp64| = {errs['fp32']:.3e}")
    assert errs["fp32"] < TOL, errs
    assert errs["wt32"] < TOL, errs


def test_wt32_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    B, N, K = 32, 64, 1040                                                # K % 16 == 0 (ssrhip_gemv takes it) but no whole quads
    master = torch.randn(N, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).float().cuda()
    Wt = to_streaming_order(master)
    packed = torch.zeros(N, K, dtype=torch.int16, device="cuda")
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((B * N + PAD,), POISON).cuda()
    a = _lib.GemvArgs()
    a.W, a.x, a.y = Wt.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride, a.w_tiled = B, N, K, 1, K, N, 1
    assert L.ssrhip_gemv_wt32_applicable(C.byref(a)) == 0
    assert L.ssrhip_gemv_wt32(C.byref(a), packed.data_ptr(), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))              # the caller's fallback takes it
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:B * N].view(B, N).cpu(), F.linear(x.cpu(), master.cpu()), rtol=TOL, atol=TOL)
    assert bool((y[B * N:] == POISON).all())


# ------------------------------------------------------------------------------------------ engine level
# the smallest config in which all six families qualify at every row count (tests/test_gpu_wt16.py)
LAYERS, STEPS = 2, 24


@pytest.fixture(scope="module")
def tiny2048():
    args = W.lm_args_tiny(d_model=2048, nhead=16, layers=LAYERS, vocab=2048)
    sd = W.lm_state_dict(args, seed=11, device="cuda")
    return args, sd


@pytest.fixture(scope="module")
def arena16(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="bf16")


def _prompts(args, n_utt, use_cfg, greedy):
    gen = torch.Generator().manual_seed(1000 + n_utt)
    rows, cols, knobs = [], [], []
    for u in range(n_utt):
        Lt, T = 9 + 2 * u, 21 + 3 * u
        x = torch.randint(0, args.text_vocab_size, (Lt,), generator=gen).numpy()
        y = torch.randint(0, args.audio_vocab_size, (T, 4), generator=gen)
        cated, _, num_task, _ = LY.build_layout(y.T.numpy(), np.asarray([[T, T]]), args)
        rows.append(x)
        if use_cfg:
            rows.append(torch.randint(0, args.text_vocab_size + 1, (Lt,), generator=gen).numpy())
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1 if greedy else 40, top_p=1.0 if greedy else 0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5,
                                 cfg_stride=2, use_cfg=use_cfg, text_len=Lt, n_spans=num_task, seed=u))
    return rows, cols, knobs


def _trace(eng, args, n_utt, use_cfg, greedy, use_graph, noise):
    """24 single steps: (per-step post-edit logits [STEPS][n_utt][K][card], generated [n_utt][STEPS][K], device allocations during the steps)"""
    rows, cols, knobs = _prompts(args, n_utt, use_cfg, greedy)
    eng.start(rows, cols, knobs, noise=noise)
    torch.cuda.synchronize()
    allocs0 = torch.cuda.memory_stats()["num_device_alloc"]
    logits = []
    for _ in range(STEPS):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        logits.append(eng.dbg_logits.cpu().clone())
    allocs = torch.cuda.memory_stats()["num_device_alloc"] - allocs0
    return torch.stack(logits), eng.generated[:, :STEPS].cpu().clone(), allocs


@pytest.mark.parametrize("n_utt,use_cfg", [(17, False), (16, True)], ids=["17rows", "32rows"])
def test_wt32_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena16, n_utt, use_cfg):
    args, _ = tiny2048
    mk = lambda **kw: DecodeEngine(arena16, n_utt, use_cfg, 256, 64, debug_logits=True, **kw)
    e16, e32 = mk(stream_wt32=True), mk(stream_wt32=False)
    noise = torch.empty(n_utt, 64, args.n_codebooks, arena16.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        for greedy in (True, False):
            for use_graph in (False, True):
                lg16, tok16, allocs16 = _trace(e16, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise)
                lg32, tok32, _ = _trace(e32, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise)
                assert e16.stream_wt32 and e16.wt32_launches_per_step == 4 * LAYERS + 2 == 10      # not through the fallback
                assert e32.wt32_launches_per_step == 0 and not e32.stream_wt32
                for e in (e16, e32):                                                               # a counter and a switch of its own
                    assert e.wt16_launches_per_step == 0 and e.w16_launches_per_step == 0 and not e.stream_wt16 and not e.stream_w16
                assert torch.isfinite(lg16).all() and allocs16 == 0, allocs16
                for s in range(STEPS):
                    assert torch.equal(lg16[s], lg32[s]), (greedy, use_graph, s, float((lg16[s] - lg32[s]).abs().max()))
                assert torch.equal(tok16, tok32), (greedy, use_graph)
    finally:
        e16.close()
        e32.close()


def test_wt32_engine_contract(tiny2048, arena16, monkeypatch):
    monkeypatch.delenv("SSRHIP_GEMVM_W16", raising=False)
    with pytest.raises(ValueError, match="stream_w16"):
        DecodeEngine(arena16, 2, True, 256, 64, stream_wt32=True)         # 4 rows: that is stream_w16's engine
    with pytest.raises(ValueError, match="stream_wt16"):
        DecodeEngine(arena16, 8, True, 256, 64, stream_wt32=True)         # 16 rows: stream_wt16's
    with pytest.raises(ValueError, match="5..16"):
        DecodeEngine(arena16, 17, False, 256, 64, stream_wt16=True)       # and stream_wt16 keeps refusing 17 rows
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(a32, 17, False, 256, 64, stream_wt32=True)           # an fp32 arena has no rounded masters
    assert DecodeEngine(a32, 17, False, 256, 64).stream_wt32 is False
    assert DecodeEngine(arena16, 17, False, 256, 64).stream_wt32 is False  # the variable unset: WT32_DEFAULT = "0"
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")
    assert DecodeEngine(arena16, 17, False, 256, 64).stream_wt32 is True
    # the C side refuses a 16-row engine and names its setter
    eng = DecodeEngine(arena16, 8, True, 256, 64, stream_wt16=False)
    try:
        assert eng.stream_wt32 is False and eng.stream_wt16 is False
        eng._create_ctx()
        wt16 = arena16.wt16_struct()
        assert eng.lib.ssrhip_lm_set_wt32(eng._ctx, C.byref(wt16)) < 0
        assert b"ssrhip_lm_set_wt16" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
def _utterance(args, seed, Lt=10, T=18):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, args.text_vocab_size, (1, Lt), generator=g)
    y = torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g)
    return x, y, torch.LongTensor([[[T, T]]])


def _same(r1, r2):
    return torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and r1[2] == r2[2] and r1[3] == r2[3]


def test_bf16_model_streams_wt32_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5)
    # 20 ragged utterances on 16 slots: a 32-row engine whose slots are refilled as utterances end
    utts = [dict(x=u[0], y=u[1], mask_interval=u[2]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(20))]
    batch = lambda: m.inference_batch(utts, aug_text=True, group=16, seed=3, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    monkeypatch.delenv("SSRHIP_GEMVM_W16", raising=False)
    r_fp32 = batch()
    assert eng_of().B == 32 and eng_of().stream_wt32 is False and eng_of().wt32_launches_per_step == 0 and m.weight_dtype == "fp32"
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")                           # the switch is read when an engine is built
    m.set_weight_dtype("bf16")
    r_on = batch()
    e = eng_of()
    assert e.B == 32 and e.n_refills >= 2 and e.a.weight_dtype == "bf16"
    assert e.stream_wt32 is True and e.wt32_launches_per_step == 4 * LAYERS + 2
    assert e.stream_wt16 is False and e.wt16_launches_per_step == 0 and e.stream_w16 is False and e.w16_launches_per_step == 0
    assert getattr(m._arena, "_wt16_ready", False)
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "0")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("bf16")
    r_off = batch()
    assert eng_of().B == 32 and eng_of().stream_wt32 is False and eng_of().wt32_launches_per_step == 0 and eng_of().a.weight_dtype == "bf16"
    assert not getattr(m._arena, "_wt16_ready", False)                    # switched off: the packed copies are not built either
    assert len(r_on) == len(r_off) == 20
    for a, b in zip(r_on, r_off):
        assert _same(a, b)                                                # res, marks, masks and intervals
    # back to fp32: the arena (and the packed copies with it) is dropped, today's tokens come back bit for bit
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")
    m.set_weight_dtype("fp32")
    assert m._arena is None and m._engines == {}
    r_back = batch()
    assert eng_of().stream_wt32 is False and eng_of().a.weight_dtype == "fp32" and not getattr(m._arena, "_wt16_ready", False)
    for a, b in zip(r_back, r_fp32):
        assert _same(a, b)
