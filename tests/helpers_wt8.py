"""Shared by the GPU tests of the e4m3 weight stream of the 5..16-row decode step (tests/test_gpu_wt8.py): the quantised weights of a
shape (optionally with a different power of two on every row, so that a misplaced scale cannot hide), the launch comparison with its fp64
reference and the engine-step comparison. Operands, poison, pad, shuffled page table and the fp64 reference are those of
tests/helpers_w16.py; only the weights' rounding and the entry point (codes AND scales) differ."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

import helpers_conditioning as HC
from helpers_w16 import HD, LAYER, LAYERS, N_LAYER, PAD, POISON, STEPS, TOL, H, _trace, from_tiled, kv_pool, to_tiled  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import (W16_STREAMS, DecodeEngine, e4m3_master, from_wt8_order, quantize_e4m3, to_streaming_order, to_wt8_order)

PREFIX = "wt8."


def row_factors(N):
    """2^((5n mod 13) - 9): thirteen different powers of two, 2^-9 .. 2^3, in any sixteen consecutive rows"""
    return torch.ldexp(torch.ones(N), (5 * torch.arange(N)) % 13 - 9)


@functools.lru_cache(maxsize=None)
def shape_weights(G, N, K, spread=False):
    """One quantised matrix per shape, shared by every case of that shape and never modified: (fp32 streaming-order copy of code * scale,
    codes in SSRHIP_WT8_INDEX order, scales [G][N], the PACKED BUFFER unpacked and scaled again [G][N][K], bias [G][N]). spread: row n of
    the raw draw is multiplied by 2^((5n mod 13) - 9) first; every aligned 16-row tile must then hold >= 8 distinct scale exponents."""
    seed = N * 7 + K + G
    raw = W.make_tensor(f"{PREFIX}{G}.{N}.{K}", (G, N, K), f"lin:{K}", seed, device="cuda")
    if spread:
        raw = raw * row_factors(N).cuda().view(1, N, 1)
    codes, scale = quantize_e4m3(raw)
    assert not bool(((codes & 0x7f) == 0x7f).any())
    master = e4m3_master(codes, scale)
    packed = to_wt8_order(codes)
    unpacked = e4m3_master(from_wt8_order(packed, N), scale)
    assert torch.equal(unpacked, master)                                  # the packed buffer times the scales is the master exactly
    if spread:
        exps = torch.frexp(scale)[1].cpu()
        for grp in range(G):
            for n0 in range(0, N - 15, 16):
                assert len(set(exps[grp, n0:n0 + 16].tolist())) >= 8, (grp, n0)
    bias = torch.randn(G, N, generator=torch.Generator().manual_seed(seed)).cuda()
    return to_streaming_order(master), packed, scale.contiguous(), unpacked, bias


def gemv_args(Wf, bias, xbuf, y, B, G, N, K, ny, pro, act, epi, tiled, y_tiled, kv=None):
    a = _lib.GemvArgs()
    a.W, a.bias, a.x, a.y = Wf.data_ptr(), bias.data_ptr(), xbuf.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
    a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
    a.x_tiled, a.y_tiled, a.w_tiled = tiled, int(y_tiled), 1
    if kv is not None:
        pool, table, max_pages, pos = kv
        a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), max_pages, N_LAYER, H, HD)
        a.layer, a.kv_pos = LAYER, pos.data_ptr()
    return a


def check_launch(L, B, G, N, K, pro, act, epi, tiled, kv_pos, max_pages=2, spread=False, x=None):
    """ssrhip_gemv_wt8 on codes + scales against ssrhip_gemv on the fp32 streaming-order copy of code * scale: the same bits in the whole
    output buffer (poisoned rows and pad included) and the whole KV pool; then both against torch fp64 on the UNPACKED PACKED BUFFER TIMES
    THE SCALES, which does not depend on the fp32 kernel, within helpers_w16.TOL. spread: the bound of row n is TOL * max(1, f_n), f_n the
    power of two the row was multiplied by — a power of two scales every product, sum and rounding error of the row's dot product exactly,
    while the roundings of the bias / residual additions stay at the size of the O(1) result (hence not below TOL for f_n < 1).
    x [B, G*K] (CPU): as in helpers_w16.check_launch (ill-conditioned rows; the fp64 bound then follows helpers_conditioning's rule)."""
    x_given = x
    seed = B * 100003 + N * 7 + K + pro
    g = torch.Generator().manual_seed(seed)
    Wf, packed, scale, Wu, bias = shape_weights(G, N, K, spread)
    qkv = epi == _lib.EPI_QKV_APPEND
    y_tiled = tiled and not qkv                                            # the q output of the QKV launch is always row-major
    x = (torch.randn(B, G * K, generator=g) * 1.5 + 0.3).cuda()
    if x_given is not None:
        x = x_given.reshape(B, G * K).cuda()
    ny = K if qkv else G * N
    yv = (torch.randn(B, ny, generator=g) if epi == _lib.EPI_RESIDUAL else torch.full((B, ny), POISON)).cuda()
    xbuf = to_tiled(x) if tiled else x.reshape(-1).clone()
    y0 = torch.cat([to_tiled(yv) if y_tiled else yv.reshape(-1), torch.full((PAD,), POISON, device="cuda")])
    n_y = y0.numel() - PAD
    pool0 = kv_pool(B, max_pages, qkv)
    table = torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32).cuda()     # shuffled physical pages
    pos_l = list(kv_pos[:B])
    pos = torch.tensor(pos_l, dtype=torch.int32).cuda()

    def run(use_packed):
        y, pool = y0.clone(), pool0.clone()
        a = gemv_args(Wf, bias, xbuf, y, B, G, N, K, ny, pro, act, epi, tiled, y_tiled, (pool, table, max_pages, pos) if qkv else None)
        if use_packed:
            assert L.ssrhip_gemv_wt8_applicable(C.byref(a)) == 1
            rc = L.ssrhip_gemv_wt8(C.byref(a), packed.data_ptr(), scale.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (rc, L.ssrhip_last_error())
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y, pool

    y8, pool8 = run(True)
    y32, pool32 = run(False)
    assert torch.equal(y8, y32), float((y8 - y32).abs().max())            # whole buffers, poisoned rows and pad included
    assert torch.equal(pool8, pool32)
    assert torch.equal(y8[n_y:], y0[n_y:])                                # the pad is untouched
    # ---- independent of the fp32 kernel: torch fp64 on the unpacked packed buffer times the scales
    xin = x.view(B, G, K).double()
    if pro == _lib.PRO_LAYERNORM:
        xin = F.layer_norm(xin, (K,), None, None, 1e-5)
    ref = torch.stack([F.linear(xin[:, k], Wu[k].double(), bias[k].double()) for k in range(G)], 1)          # [B][G][N]
    ref = F.relu(ref) if act == _lib.ACT_RELU else (F.gelu(ref) if act == _lib.ACT_GELU_ERF else ref)
    ref = ref.reshape(B, G * N)
    if epi == _lib.EPI_RESIDUAL:
        ref = ref + yv.double()
    bound = (row_factors(N).clamp(min=1.0).repeat(G) if spread else torch.ones(G * N)).double().cuda()       # per output column [G * N]
    errs = {}
    for name, y, pool in (("wt8", y8, pool8), ("fp32", y32, pool32)):
        got = from_tiled(y[:n_y], B, ny) if y_tiled else y[:n_y].view(B, ny)
        assert torch.isfinite(got).all(), name
        if qkv:
            err = float(((got.double() - ref[:, :K]).abs() / bound[:K]).max())
            untouched = torch.ones_like(pool0, dtype=torch.bool)
            for b in range(B):
                page = int(table[b, pos_l[b] // _lib.PAGE])
                for which in (0, 1):
                    row = pool[page, LAYER, which, :, pos_l[b] % _lib.PAGE, :].reshape(-1)
                    cols = slice((1 + which) * K, (2 + which) * K)
                    err = max(err, float(((row.double() - ref[b, cols]).abs() / bound[cols]).max()))
                untouched[page, LAYER, :, :, pos_l[b] % _lib.PAGE, :] = False
            assert torch.equal(pool[untouched], pool0[untouched]), name   # nothing but the appended positions was written
        else:
            err = float(((got.double() - ref).abs() / bound).max())
        errs[name] = err
    print(f"B={B} G={G} N={N} K={K} pro={pro} tiled={tiled} spread={spread}: max |wt8 - fp64| = {errs['wt8']:.3e}, max |fp32 - fp64| = {errs['fp32']:.3e}"
          + (" (relative to max(1, row factor))" if spread else ""))
    tol = TOL
    if x_given is not None:
        tol = HC.gemv_chain_tol(TOL, Wu, bias, act, yv if epi == _lib.EPI_RESIDUAL else None, x=x, ln=pro == _lib.PRO_LAYERNORM)
    assert errs["fp32"] < tol, errs
    assert errs["wt8"] < tol, errs


def check_refusal(L, B, N, K):
    """A launch ssrhip_gemv_wt8 does not take: it answers 1, nothing is launched, and the caller's ssrhip_gemv takes it."""
    codes, scale = quantize_e4m3(torch.randn(N, K, generator=torch.Generator().manual_seed(2)).cuda())
    master = e4m3_master(codes, scale)
    Wf = to_streaming_order(master)
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((B * N + PAD,), POISON).cuda()
    a = _lib.GemvArgs()
    a.W, a.x, a.y = Wf.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride, a.w_tiled = B, N, K, 1, K, N, 1
    assert L.ssrhip_gemv_wt8_applicable(C.byref(a)) == 0
    assert L.ssrhip_gemv_wt8(C.byref(a), codes.data_ptr(), scale.data_ptr(), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    return a, x, y, master


def check_engine_steps(args, arena8, arena16, n_utt, use_cfg, grow):
    """A stream_wt8=True engine against a masters engine (stream_wt8=False, stream_wt16=False) and a stream_wt16=True engine of the same
    e4m3 arena: the same post-edit logits at each of 24 single steps and the same tokens, greedy and sampled, eager and as a graph; every
    GEMV launch of the packed engine ran a kernel of the e4m3 stream (not the fallback), every other stream's switch and counter is off / 0,
    the steps allocate nothing. The greedy eager logits also DIFFER from a bf16 arena's engine on the same prompts."""
    mk = lambda arena, **kw: DecodeEngine(arena, n_utt, use_cfg, 256, 64, debug_logits=True, **kw)
    engines = dict(packed=mk(arena8, stream_wt8=True), masters=mk(arena8, stream_wt8=False, stream_wt16=False),
                   wt16=mk(arena8, stream_wt8=False, stream_wt16=True))
    noise = torch.empty(n_utt, 64, args.n_codebooks, arena8.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        for greedy in (True, False):
            for use_graph in (False, True):
                out = {name: _trace(e, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise, grow) for name, e in engines.items()}
                for name, e in engines.items():
                    assert e.stream_wt8 is (name == "packed") and e.stream_w8 is False, name
                    assert e.wt8_launches_per_step == (4 * LAYERS + 2 if name == "packed" else 0), (name, e.wt8_launches_per_step)   # not the fallback
                    assert e.w8_launches_per_step == 0 and e.w8_pair_launches_per_step == 0 and e.w16_pair_launches_per_step == 0, name
                    for st in W16_STREAMS:
                        on = name == "wt16" and st.name == "wt16"
                        assert getattr(e, "stream_" + st.name) is on, (name, st.name)
                        assert getattr(e, st.name + "_launches_per_step") == (4 * LAYERS + 2 if on else 0), (name, st.name)
                lg8, tok8, allocs8 = out["packed"]
                assert torch.isfinite(lg8).all() and allocs8 == 0, allocs8
                for name in ("masters", "wt16"):
                    lg, tok, _ = out[name]
                    for s in range(STEPS):
                        assert torch.equal(lg8[s], lg[s]), (name, greedy, use_graph, s, float((lg8[s] - lg[s]).abs().max()))
                    assert torch.equal(tok8, tok), (name, greedy, use_graph)
                if greedy and not use_graph:                              # not silently a bf16 model
                    e16 = mk(arena16, stream_wt16=False)
                    try:
                        lg16, _, _ = _trace(e16, args, n_utt, use_cfg, True, False, None, grow)
                    finally:
                        e16.close()
                    assert not torch.equal(lg8[0], lg16[0])
    finally:
        for e in engines.values():
            e.close()
