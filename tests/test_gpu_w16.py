"""GPU: the opt-in bf16 weight stream of the <= 4-row decode step (csrc/gemv_w16.hip, DESIGN.md Part I.10).

bf16 -> fp32 is a 16-bit shift and exact, and the w16 kernels run the fp32 kernels' fmaf sequence in the same order, so every comparison
between the two is `torch.equal`: launch by launch against `ssrhip_gemv` on the rounded weights, step by step between an engine that streams
the packed copies and one that streams the fp32 masters, and end to end through the public surface. The launch-level outputs are also held
against a torch fp64 product built from the UNPACKED PACKED BUFFER (a check that does not depend on the fp32 kernel), with the tolerance the
fp32 launch tests of the same shapes use in tests/test_gpu_kernels.py (3e-5: fp32, summation order only)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena, to_w16_order
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

POISON = -777.25
PAD = 64                      # poisoned floats behind every output buffer: a stray store shows in the whole-buffer comparison
TOL = 3e-5                    # tests/test_gpu_kernels.py: test_gemv_step_shapes_both_kernels / test_gemv_seg_combine_and_qkv_append_at_2048


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def unpack_w16(packed):
    """[.., N, K] int16 in SSRHIP_W16_INDEX order -> fp32 [.., N, K]: the inverse permutation and the 16-bit shift"""
    *lead, N, K = packed.shape
    n = len(lead)
    u = packed.reshape(*lead, N, K // 1024, 2, 64, 2, 4).permute(*range(n), n, n + 1, n + 2, n + 4, n + 3, n + 5).reshape(*lead, N, K)
    return ((u.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)


# (G, N, K, prologue, activation, epilogue): the six launches of the 830M step, a ragged workgroup split, S = 4
SHAPES = [
    (1, 6144, 2048, _lib.PRO_LAYERNORM, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),
    (1, 8192, 2048, _lib.PRO_LAYERNORM, _lib.ACT_RELU, _lib.EPI_STORE),
    (1, 4096, 2048, _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
    (1, 2048, 8192, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    (1, 2048, 2048, _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    (4, 2056, 1024, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_STORE),
    (1, 520, 1024, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_STORE),
    (1, 1024, 4096, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
]
H, HD, N_LAYER, LAYER, MAX_PAGES = 16, 128, 2, 1, 3


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_w16_launch_is_bit_identical_to_the_fp32_launch_on_the_rounded_weights(L, B, G, N, K, pro, act, epi):
    seed = B * 100003 + N * 7 + K + pro
    g = torch.Generator().manual_seed(seed)
    Wr = W.make_tensor(f"w16.{G}.{N}.{K}", (G, N, K), f"lin:{K}", seed, device="cuda").to(torch.bfloat16)
    master, packed = Wr.float().contiguous(), to_w16_order(Wr)
    bias = torch.randn(G, N, generator=g).cuda()
    x = (torch.randn(B, G, K, generator=g) * 1.5 + 0.3).cuda().contiguous()
    ny = K if epi == _lib.EPI_QKV_APPEND else G * N                       # floats per row of y (q of the QKV launch)
    y0 = torch.full((B * ny + PAD,), POISON)
    if epi == _lib.EPI_RESIDUAL:
        y0[:B * ny] = torch.randn(B * ny, generator=g)
    pool0 = torch.full((B * MAX_PAGES + 1, N_LAYER, 2, H, _lib.PAGE, HD) if epi == _lib.EPI_QKV_APPEND else (1,), POISON)
    table = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES).to(torch.int32).cuda()
    pos_l = [130, 7, 383, 256][:B]
    pos = torch.tensor(pos_l, dtype=torch.int32).cuda()
    lens_l = [300, 129, 384, 1][:B]                                       # 3, 2, 3 and 1 pages of partials
    lens = torch.tensor(lens_l, dtype=torch.int32).cuda()
    part_o = torch.randn(B, H, MAX_PAGES, HD, generator=g)
    part_ml = torch.stack([torch.randn(B, H, MAX_PAGES, generator=g) * 2, torch.rand(B, H, MAX_PAGES, generator=g) + 0.5], dim=-1).contiguous()
    for b in range(B):                                                    # beyond a row's pages the buffers hold what the kernel must not use
        n_pg = (lens_l[b] + _lib.PAGE - 1) // _lib.PAGE
        part_o[b, :, n_pg:] = float("nan")
        part_ml[b, :, n_pg:] = float("nan")
    d_po, d_pml = part_o.cuda(), part_ml.cuda()

    def run(use_w16):
        y, pool = y0.clone().cuda(), pool0.clone().cuda()
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = master.data_ptr(), bias.data_ptr(), x.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
        a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
        if epi == _lib.EPI_QKV_APPEND:
            a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, N_LAYER, H, HD)
            a.layer, a.kv_pos = LAYER, pos.data_ptr()
        if pro == _lib.PRO_ATTN_COMBINE:
            a.x = 0
            a.part_o, a.part_ml, a.max_splits, a.row_len = d_po.data_ptr(), d_pml.data_ptr(), MAX_PAGES, lens.data_ptr()
            a.kv = _lib.KV(0, 0, MAX_PAGES, 1, H, HD)
        if use_w16:
            assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 1
            rc = L.ssrhip_gemv_w16(C.byref(a), packed.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (rc, L.ssrhip_last_error())
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y.cpu(), pool.cpu()

    y16, pool16 = run(True)
    y32, pool32 = run(False)
    assert torch.isfinite(y16).all()
    assert torch.equal(y16, y32), float((y16 - y32).abs().max())          # whole buffers, poison tail included
    assert torch.equal(pool16, pool32)
    assert torch.equal(y16[B * ny:], y0[B * ny:])
    # ---- independent of the fp32 kernel: torch fp64 on the unpacked packed buffer
    Wu = unpack_w16(packed).cpu()
    assert torch.equal(Wu, master.cpu())
    xc = x.cpu()
    if pro == _lib.PRO_ATTN_COMBINE:
        xin = torch.zeros(B, 1, K, dtype=torch.float64)
        for b in range(B):
            n_pg = (lens_l[b] + _lib.PAGE - 1) // _lib.PAGE
            m, l_ = part_ml[b, :, :n_pg, 0].double(), part_ml[b, :, :n_pg, 1].double()
            e = torch.exp(m - m.max(dim=1, keepdim=True).values)
            w = e / (e * l_).sum(dim=1, keepdim=True)                                  # [H][pages]
            xin[b, 0] = (w.unsqueeze(-1) * part_o[b, :, :n_pg].double()).sum(dim=1).reshape(-1)
    else:
        xin = (F.layer_norm(xc.double(), (K,), None, None, 1e-5) if pro == _lib.PRO_LAYERNORM else xc.double())
    ref = torch.stack([F.linear(xin[:, k], Wu[k].double(), bias[k].cpu().double()) for k in range(G)], 1)          # [B][G][N]
    ref = F.relu(ref) if act == _lib.ACT_RELU else (F.gelu(ref) if act == _lib.ACT_GELU_ERF else ref)
    ref = ref.reshape(B, G * N)
    if epi == _lib.EPI_RESIDUAL:
        ref = ref + y0[:B * ny].view(B, ny).double()
    if epi == _lib.EPI_QKV_APPEND:
        got_q = y16[:B * K].view(B, K)
        err = float((got_q.double() - ref[:, :K]).abs().max())
        untouched = torch.ones_like(pool0, dtype=torch.bool)
        for b in range(B):
            page = int(table[b, pos_l[b] // _lib.PAGE])
            for which in (0, 1):
                got = pool16[page, LAYER, which, :, pos_l[b] % _lib.PAGE, :].reshape(-1)
                err = max(err, float((got.double() - ref[b, (1 + which) * K:(2 + which) * K]).abs().max()))
            untouched[page, LAYER, :, :, pos_l[b] % _lib.PAGE, :] = False
        assert torch.equal(pool16[untouched], pool0[untouched])           # nothing but the appended position was written
    else:
        err = float((y16[:B * ny].view(B, ny).double() - ref).abs().max())
    print(f"B={B} G={G} N={N} K={K} pro={pro}: max |w16 - fp64| = {err:.3e}")
    if pro == _lib.PRO_ATTN_COMBINE:
        torch.testing.assert_close(y16[:B * ny].view(B, ny), ref.float(), rtol=TOL, atol=TOL)
    else:
        assert err < TOL, err


def test_w16_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    B, N, K = 2, 256, 1536
    master = torch.randn(N, K).to(torch.bfloat16).float().cuda()
    packed = torch.zeros(N, K, dtype=torch.int16, device="cuda")
    x = torch.randn(B, K).cuda()
    y = torch.full((B * N + PAD,), POISON).cuda()
    a = _lib.GemvArgs()
    a.W, a.x, a.y = master.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, N
    assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 0
    assert L.ssrhip_gemv_w16(C.byref(a), packed.data_ptr(), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))              # the caller's fallback takes it
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:B * N].view(B, N).cpu(), F.linear(x.cpu(), master.cpu()), rtol=TOL, atol=TOL)


# ------------------------------------------------------------------------------------------ engine level
# the smallest config in which all six families qualify: out-projection K = 2048, head-MLP2 K = 1024
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
        Lt, T = 9 + 4 * u, 21 + 6 * u
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


@pytest.mark.parametrize("n_utt,use_cfg", [(1, False), (1, True), (2, True)], ids=["1row", "2rows", "4rows"])
def test_w16_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena16, n_utt, use_cfg):
    args, _ = tiny2048
    B = n_utt * (2 if use_cfg else 1)
    mk = lambda **kw: DecodeEngine(arena16, n_utt, use_cfg, 256, 64, debug_logits=True, **kw)
    engines = dict(w16=mk(stream_w16=True), masters=mk(stream_w16=False, pair_mode=1))
    if B == 2:
        engines["paired"] = mk(stream_w16=False, pair_mode=0)
    noise = torch.empty(n_utt, 64, args.n_codebooks, arena16.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        for greedy in (True, False):
            for use_graph in (False, True):
                out = {name: _trace(e, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise) for name, e in engines.items()}
                e16, e32 = engines["w16"], engines["masters"]
                assert e16.stream_w16 and e16.w16_launches_per_step == 4 * LAYERS + 2 == 10        # not through the fallback
                assert e32.w16_launches_per_step == 0 and not e32.stream_w16
                assert e16.pairing is False and "bf16" in e16.pairing_why, e16.pairing_why
                assert e32.pairing is False
                lg16, tok16, allocs16 = out["w16"]
                assert torch.isfinite(lg16).all() and allocs16 == 0, allocs16
                for name in engines:
                    if name == "w16":
                        continue
                    if name == "paired":
                        if not engines[name].pairing:                      # fewer than 256 CUs, a CU mask, the slot taken: nothing to compare
                            continue
                        assert engines[name].w16_launches_per_step == 0
                    lg, tok, _ = out[name]
                    for s in range(STEPS):
                        assert torch.equal(lg16[s], lg[s]), (name, greedy, use_graph, s, float((lg16[s] - lg[s]).abs().max()))
                    assert torch.equal(tok16, tok), (name, greedy, use_graph)
    finally:
        for e in engines.values():
            e.close()


def test_w16_engine_contract(tiny2048, arena16):
    args, sd = tiny2048
    with pytest.raises(ValueError, match="<= 4-row"):
        DecodeEngine(arena16, 5, False, 256, 64, stream_w16=True)         # 5 rows
    # the C side refuses too (an engine of 5 rows exists; the packed copies are not for it)
    eng = DecodeEngine(arena16, 5, False, 256, 64)
    try:
        assert eng.stream_w16 is False
        eng._create_ctx()
        w16 = arena16.w16_struct()
        assert eng.lib.ssrhip_lm_set_w16(eng._ctx, C.byref(w16)) < 0
        assert b"<= 4-row" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(a32, 1, True, 256, 64, stream_w16=True)              # an fp32 arena has no rounded masters
    assert DecodeEngine(a32, 1, True, 256, 64).stream_w16 is False


# ------------------------------------------------------------------------------------------ public surface
def _utterance(args, seed, Lt=10, T=18):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, args.text_vocab_size, (1, Lt), generator=g)
    y = torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g)
    unc = torch.randint(0, args.text_vocab_size + 1, (1, Lt), generator=g)
    return x, y, unc, torch.LongTensor([[[T, T]]])


def _same(r1, r2):
    return torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and r1[2] == r2[2] and r1[3] == r2[3]


def test_set_weight_dtype_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    monkeypatch.delenv("SSRHIP_GEMV_W16", raising=False)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    x, y, unc, mi = _utterance(args, 21)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    call = lambda: m.inference(x.cuda(), torch.LongTensor([x.shape[1]]), x.cuda(), torch.LongTensor([x.shape[1]]), y.cuda(), y.cuda(), mi.cuda(),
                               uncond_x=unc, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    r_fp32 = call()
    assert eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0 and m.weight_dtype == "fp32"
    m.set_weight_dtype("bf16")
    r_w16 = call()
    assert m.weight_dtype == "bf16" and eng_of().stream_w16 is True and eng_of().w16_launches_per_step == 4 * LAYERS + 2
    # the same call with the switch off: the 2-row engine streams the rounded fp32 masters (and may pair) — same res, marks, masks
    monkeypatch.setenv("SSRHIP_GEMV_W16", "0")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("bf16")                                            # the switch is read when an engine is built
    r_masters = call()
    assert eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0 and eng_of().a.weight_dtype == "bf16"
    assert _same(r_w16, r_masters)
    monkeypatch.delenv("SSRHIP_GEMV_W16")
    # a 16-row engine of the bf16 model: the matrix-core step on the rounded masters, no packed stream
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(8))]
    outs = m.inference_batch(utts, aug_text=True, group=8, seed=3, **{k: kw[k] for k in ("top_k", "top_p", "temperature", "stop_repetition", "cfg_coef", "cfg_stride")})
    assert len(outs) == 8 and eng_of().B == 16 and eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0
    # back to fp32: today's tokens, bit for bit
    m.set_weight_dtype("fp32")
    assert _same(call(), r_fp32)
    assert eng_of().a.weight_dtype == "fp32"
    with pytest.raises(ValueError):
        m.set_weight_dtype("fp8")
