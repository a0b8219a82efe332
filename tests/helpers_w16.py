"""Shared by the GPU tests of the three bf16 weight streams (tests/test_gpu_w16.py, test_gpu_wt16.py, test_gpu_wt32.py): the weight
builder, the launch comparison with its fp64 reference, the refusal case, the engine-step comparison and the module fixtures. What differs
between the streams (entry point, tensor-name prefix, activation layout, KV positions, pages, prompt lengths) comes in as a `Stream`;
the seeds and the order of the random draws are those of the three files these pieces came from, so the operands keep their values."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers_conditioning as HC
import helpers_poison as HP
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import (W16_STREAMS, DecodeEngine, DecodeKnobs, LMWeightsArena, from_wt16_order, to_streaming_order, to_w16_order,
                                   to_wt16_order)

POISON = -777.25
PAD = 64                      # poisoned floats behind every output buffer: a stray store shows in the whole-buffer comparison
TOL = 3e-5                    # the bound of the fp32 launch tests of the same shapes in tests/test_gpu_kernels.py (fp32, summation order only)
H, HD, N_LAYER, LAYER = 16, 128, 2, 1
# engine level: the smallest config in which all six families qualify at every row count (out-projection K = 2048, head-MLP2 K = 1024)
LAYERS, STEPS = 2, 24

# name: the entry point is ssrhip_gemv_<name>, the engine's switch stream_<name>; prefix: of the tensor names given to W.make_tensor (it goes
# into the values); layout: (to, from) of the tiled activation buffers and streaming-order weights, None = row-major only (<= 4 rows); kv_pos:
# where row b appends its K / V; hold_fp32: the fp32 launch on the same inputs is printed and held to TOL too
Stream = namedtuple("Stream", "name prefix layout kv_pos max_pages hold_fp32")


def unpack_w16(packed):
    """[.., N, K] int16 in SSRHIP_W16_INDEX order -> fp32 [.., N, K]: the inverse permutation and the 16-bit shift"""
    *lead, N, K = packed.shape
    n = len(lead)
    u = packed.reshape(*lead, N, K // 1024, 2, 64, 2, 4).permute(*range(n), n, n + 1, n + 2, n + 4, n + 3, n + 5).reshape(*lead, N, K)
    return ((u.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)


def rounded_weights(name, G, N, K, seed, order):
    """(rounded fp32 master [G][N][K], its packed bf16 copy in `order`, the packed copy unpacked again)"""
    master = W.make_tensor(f"{name}{G}.{N}.{K}", (G, N, K), f"lin:{K}", seed, device="cuda").to(torch.bfloat16).float().contiguous()
    packed = to_w16_order(master) if order == "w16" else to_wt16_order(master)
    unpacked = unpack_w16(packed) if order == "w16" else from_wt16_order(packed, N)
    assert torch.equal(unpacked, master)                                  # the packed buffer holds the rounded master exactly
    return master, packed, unpacked


def case_weights(prefix, g, seed, G, N, K):
    """<= 4 rows: a master per case (the case's seed), its bias the first draw of the case's generator"""
    return rounded_weights(prefix, G, N, K, seed, "w16") + (torch.randn(G, N, generator=g).cuda(),)


@functools.lru_cache(maxsize=None)
def shape_weights(prefix, G, N, K):
    """5..32 rows: one rounded master per shape, shared by every case of that shape and never modified: (fp32 streaming-order copy, packed
    bf16 copy, the packed copy unpacked again [G][N][K], bias)"""
    seed = N * 7 + K + G
    master, packed, unpacked = rounded_weights(prefix, G, N, K, seed, "wt16")
    return to_streaming_order(master), packed, unpacked, torch.randn(G, N, generator=torch.Generator().manual_seed(seed)).cuda()


def to_tiled(t):
    """[B <= 16][K] -> the 16-column tiled layout (include/ssrhip.h SSRHIP_TILED): [K/4][16][4], rows >= B poisoned"""
    B, K = t.shape
    out = torch.full((K // 4, 16, 4), POISON, device=t.device)
    out[:, :B, :] = t.view(B, K // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def from_tiled(t, B, K):
    return t.view(K // 4, 16, 4)[:, :B, :].permute(1, 0, 2).reshape(B, K)


def to_panels(t):
    """[16 < B <= 32][Kw] -> the paneled tiled layout (include/ssrhip.h SSRHIP_TILED_P): two panels of [Kw/4][16][4], rows >= B poisoned"""
    B, Kw = t.shape
    out = torch.full((2, Kw // 4, 16, 4), POISON, device=t.device)
    for p in range(2):
        rows = t[16 * p:min(B, 16 * p + 16)]
        out[p, :, :rows.shape[0], :] = rows.reshape(rows.shape[0], Kw // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def from_panels(buf, B, Kw):
    return buf.view(2, Kw // 4, 16, 4).permute(0, 2, 1, 3).reshape(32, Kw)[:B]


def kv_pool(B, max_pages, qkv):
    return torch.full((B * max_pages + 1, N_LAYER, 2, H, _lib.PAGE, HD) if qkv else (1,), POISON, device="cuda")


def check_launch(L, st, B, G, N, K, pro, act, epi, tiled=0, x=None, part_ml=None, lens=None, dead=float("nan")):
    """ssrhip_gemv_<st.name> on the packed copy against ssrhip_gemv on the fp32 weights: the same bits in the whole output buffer (poisoned
    rows and pad included) and the whole KV pool, then both against torch fp64 on the UNPACKED PACKED BUFFER, which does not depend on the
    fp32 kernel. The page table is shuffled; a QKV launch may have written nothing but its rows' appended positions.
    x [B, G*K] / part_ml [B, H, max_pages, 2] (CPU) replace the default draws (tests/helpers_conditioning.py: ill-conditioned rows and
    partials); the fp64 bound then follows that file's rule, max(TOL, M * the fp32 reference's own error), the bitwise assertions stay.
    lens (B lengths) / dead (a tests/helpers_poison.py fill) replace the merge prologue's row lengths and what its dead pages hold.
    Returns the packed launch's whole output buffer."""
    x_given, part_ml_given = x, part_ml
    seed = B * 100003 + N * 7 + K + pro
    g = torch.Generator().manual_seed(seed)
    Wf, packed, Wu, bias = shape_weights(st.prefix, G, N, K) if st.layout else case_weights(st.prefix, g, seed, G, N, K)
    to_layout, from_layout = st.layout or (None, None)
    qkv, combine = epi == _lib.EPI_QKV_APPEND, pro == _lib.PRO_ATTN_COMBINE
    y_tiled = tiled and not qkv                                            # the q output of the QKV launch is always row-major
    x = (torch.randn(B, G * K, generator=g) * 1.5 + 0.3).cuda()
    if x_given is not None:
        x = x_given.reshape(B, G * K).cuda()
    ny = K if qkv else G * N                                              # floats per row of y (q of the QKV launch)
    yv = (torch.randn(B, ny, generator=g) if epi == _lib.EPI_RESIDUAL else torch.full((B, ny), POISON)).cuda()
    xbuf = to_layout(x) if tiled else x.reshape(-1).clone()
    y0 = torch.cat([to_layout(yv) if y_tiled else yv.reshape(-1), torch.full((PAD,), POISON, device="cuda")])
    n_y = y0.numel() - PAD
    pool0 = kv_pool(B, st.max_pages, qkv)
    table = torch.randperm(B * st.max_pages, generator=g).view(B, st.max_pages).to(torch.int32).cuda()     # shuffled physical pages
    pos_l = st.kv_pos[:B]
    pos = torch.tensor(pos_l, dtype=torch.int32).cuda()
    if combine:                                                           # the split-KV merge prologue (<= 4 rows): partials instead of x
        lens_l = [300, 129, 384, 1][:B] if lens is None else list(lens)  # 3, 2, 3 and 1 pages of partials
        lens = torch.tensor(lens_l, dtype=torch.int32).cuda()
        part_o = torch.randn(B, H, st.max_pages, HD, generator=g)
        part_ml = torch.stack([torch.randn(B, H, st.max_pages, generator=g) * 2, torch.rand(B, H, st.max_pages, generator=g) + 0.5], dim=-1).contiguous()
        if part_ml_given is not None:
            part_ml = part_ml_given.clone()
        pages = [(n + _lib.PAGE - 1) // _lib.PAGE for n in lens_l]
        HP.fill_dead(part_o, part_ml, lens_l, dead)                       # beyond a row's pages the buffers hold what the kernel must not use
        d_po, d_pml = part_o.cuda(), part_ml.cuda()

    def run(use_packed):
        y, pool = y0.clone(), pool0.clone()
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = Wf.data_ptr(), bias.data_ptr(), xbuf.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
        a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
        a.x_tiled, a.y_tiled, a.w_tiled = tiled, int(y_tiled), int(st.layout is not None)
        if qkv:
            a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), st.max_pages, N_LAYER, H, HD)
            a.layer, a.kv_pos = LAYER, pos.data_ptr()
        if combine:
            a.x = 0
            a.part_o, a.part_ml, a.max_splits, a.row_len = d_po.data_ptr(), d_pml.data_ptr(), st.max_pages, lens.data_ptr()
            a.kv = _lib.KV(0, 0, st.max_pages, 1, H, HD)
        if use_packed:
            assert getattr(L, f"ssrhip_gemv_{st.name}_applicable")(C.byref(a)) == 1
            rc = getattr(L, "ssrhip_gemv_" + st.name)(C.byref(a), packed.data_ptr(), _lib.stream_ptr())
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
    if y_tiled and B > 16:                                                # ... and so are the columns >= B of panel 1
        assert bool((y16[:n_y].view(2, ny // 4, 16, 4)[1, :, B - 16:, :] == POISON).all())
    # ---- independent of the fp32 kernel: torch fp64 on the unpacked packed buffer
    if combine:
        xin = torch.zeros(B, 1, K, dtype=torch.float64)
        for b in range(B):
            m, l_ = part_ml[b, :, :pages[b], 0].double(), part_ml[b, :, :pages[b], 1].double()
            e = torch.exp(m - m.max(dim=1, keepdim=True).values)
            w = e / (e * l_).sum(dim=1, keepdim=True)                                  # [H][pages]
            xin[b, 0] = (w.unsqueeze(-1) * part_o[b, :, :pages[b]].double()).sum(dim=1).reshape(-1)
        xin = xin.cuda()
    else:
        xin = x.view(B, G, K).double()
        if pro == _lib.PRO_LAYERNORM:
            xin = F.layer_norm(xin, (K,), None, None, 1e-5)
    ref = torch.stack([F.linear(xin[:, k], Wu[k].double(), bias[k].double()) for k in range(G)], 1)          # [B][G][N]
    ref = F.relu(ref) if act == _lib.ACT_RELU else (F.gelu(ref) if act == _lib.ACT_GELU_ERF else ref)
    ref = ref.reshape(B, G * N)
    if epi == _lib.EPI_RESIDUAL:
        ref = ref + yv.double()
    tol = TOL
    if x_given is not None or part_ml_given is not None:
        y_res = yv if epi == _lib.EPI_RESIDUAL else None
        if combine:
            tol = HC.gemv_chain_tol(TOL, Wu, bias, act, y_res, part_o=part_o, part_ml=part_ml, lens=lens_l)
        else:
            tol = HC.gemv_chain_tol(TOL, Wu, bias, act, y_res, x=x, ln=pro == _lib.PRO_LAYERNORM)
    errs = {}
    for name, y, pool in ((st.name, y16, pool16), ("fp32", y32, pool32)):
        got = from_layout(y[:n_y], B, ny) if y_tiled else y[:n_y].view(B, ny)
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
    head = f"B={B} G={G} N={N} K={K} pro={pro}" + (f" tiled={tiled}" if st.layout else "")
    if st.hold_fp32:
        print(f"{head}: max |{st.name} - fp64| = {errs[st.name]:.3e}, max |fp32 - fp64| = {errs['fp32']:.3e}")
        assert errs["fp32"] < tol, errs
    else:
        print(f"{head}: max |{st.name} - fp64| = {errs[st.name]:.3e}")
    if combine:
        torch.testing.assert_close(y16[:n_y].view(B, ny), ref.float(), rtol=tol, atol=tol)
    else:
        assert errs[st.name] < tol, errs
    return y16


def check_refusal(L, st, B, N, K):
    """A shape ssrhip_gemv_<st.name> does not take: it answers 1, nothing is launched, and the caller's ssrhip_gemv takes it."""
    master = torch.randn(N, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).float().cuda()
    Wf = to_streaming_order(master) if st.layout else master
    packed = torch.zeros(N, K, dtype=torch.int16, device="cuda")
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((B * N + PAD,), POISON).cuda()
    a = _lib.GemvArgs()
    a.W, a.x, a.y = Wf.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride, a.w_tiled = B, N, K, 1, K, N, int(st.layout is not None)
    assert getattr(L, f"ssrhip_gemv_{st.name}_applicable")(C.byref(a)) == 0
    assert getattr(L, "ssrhip_gemv_" + st.name)(C.byref(a), packed.data_ptr(), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))              # the caller's fallback takes it
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:B * N].view(B, N).cpu(), F.linear(x.cpu(), master.cpu()), rtol=TOL, atol=TOL)
    assert bool((y[B * N:] == POISON).all())


# ------------------------------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


@pytest.fixture(scope="module")
def tiny2048():
    args = W.lm_args_tiny(d_model=2048, nhead=16, layers=LAYERS, vocab=2048)
    sd = W.lm_state_dict(args, seed=11, device="cuda")
    return args, sd


@pytest.fixture(scope="module")
def arena16(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="bf16")


def _prompts(args, n_utt, use_cfg, greedy, grow):
    """utterance u: 9 + grow[0] * u text tokens, 21 + grow[1] * u audio frames"""
    gen = torch.Generator().manual_seed(1000 + n_utt)
    rows, cols, knobs = [], [], []
    for u in range(n_utt):
        Lt, T = 9 + grow[0] * u, 21 + grow[1] * u
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


def _trace(eng, args, n_utt, use_cfg, greedy, use_graph, noise, grow):
    """24 single steps: (per-step post-edit logits [STEPS][n_utt][K][card], generated [n_utt][STEPS][K], device allocations during the steps)"""
    rows, cols, knobs = _prompts(args, n_utt, use_cfg, greedy, grow)
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


def check_engine_steps(stream, args, arena, n_utt, use_cfg, grow, masters_kw={}, unpairs=False):
    """An engine that streams the packed copies (stream_<stream>=True) against one that streams the fp32 masters: the same post-edit logits
    at each of 24 single steps and the same tokens, greedy and sampled, eager and as a graph; every GEMV launch of the packed engine ran a
    kernel of this stream (not the fallback), no other stream's switch or counter moved, and the steps allocate nothing. unpairs (<= 4
    rows): the packed engine steps unpaired and says why; at 2 rows a third engine that may pair is compared too."""
    mk = lambda on, **kw: DecodeEngine(arena, n_utt, use_cfg, 256, 64, debug_logits=True, **{"stream_" + stream: on}, **kw)
    engines = dict(packed=mk(True), masters=mk(False, **masters_kw))
    if unpairs and engines["packed"].B == 2:
        engines["paired"] = mk(False, pair_mode=0)
    noise = torch.empty(n_utt, 64, args.n_codebooks, arena.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        for greedy in (True, False):
            for use_graph in (False, True):
                out = {name: _trace(e, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise, grow) for name, e in engines.items()}
                for name, e in engines.items():                           # a counter and a switch of its own
                    if name == "paired" and not e.pairing:                # fewer than 256 CUs, a CU mask, the slot taken: nothing to compare
                        continue
                    for st in W16_STREAMS:
                        on = name == "packed" and st.name == stream
                        assert getattr(e, "stream_" + st.name) is on, (name, st.name)
                        assert getattr(e, st.name + "_launches_per_step") == (4 * LAYERS + 2 if on else 0), (name, st.name)   # not through the fallback
                if unpairs:
                    assert engines["packed"].pairing is False and "bf16" in engines["packed"].pairing_why, engines["packed"].pairing_why
                    assert engines["masters"].pairing is False
                lg16, tok16, allocs16 = out["packed"]
                assert torch.isfinite(lg16).all() and allocs16 == 0, allocs16
                for name in engines:
                    if name == "packed" or (name == "paired" and not engines[name].pairing):
                        continue
                    lg, tok, _ = out[name]
                    for s in range(STEPS):
                        assert torch.equal(lg16[s], lg[s]), (name, greedy, use_graph, s, float((lg16[s] - lg[s]).abs().max()))
                    assert torch.equal(tok16, tok), (name, greedy, use_graph)
    finally:
        for e in engines.values():
            e.close()


# ------------------------------------------------------------------------------------------ public surface
def _utterance(args, seed, Lt=10, T=18):
    """(x, y, unconditional x, mask_interval)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, args.text_vocab_size, (1, Lt), generator=g)
    y = torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g)
    unc = torch.randint(0, args.text_vocab_size + 1, (1, Lt), generator=g)
    return x, y, unc, torch.LongTensor([[[T, T]]])


def _same(r1, r2):
    return torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and r1[2] == r2[2] and r1[3] == r2[3]


def fake_gemv_args(B, N=512, K=2048, w_tiled=1, pro=_lib.PRO_NONE):
    """launch arguments for the host tests: the pointers are never dereferenced, every call made with them is answered before any launch"""
    a = _lib.GemvArgs()
    a.W, a.y, a.x = 0x1000, 0x2000, 0x3000
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, N
    a.w_tiled, a.pro = w_tiled, pro
    return a
