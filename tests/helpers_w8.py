"""Shared by the tests of the e4m3 weight stream (tests/test_w8_host.py, tests/test_gpu_w8.py): a quantiser written independently of
torch's float8 cast (a table of the 254 finite e4m3 values, nearest with ties to the even code), SSRHIP_W8_INDEX evaluated in Python, the
launch comparison with its fp64 reference and the engine-step comparison. The launch operands are those of tests/helpers_w16.py
(the same `W.make_tensor` draws, seeds, poison, pad, shuffled page table); only the weights' rounding and the entry point differ."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

import helpers_conditioning as HC
import helpers_poison as HP
from helpers_w16 import LAYER, N_LAYER, PAD, POISON, STEPS, TOL, H, HD, LAYERS, _trace, kv_pool  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import W16_STREAMS, DecodeEngine, e4m3_master, from_w8_order, quantize_e4m3, to_w8_order


def e4m3_value(code: int) -> float:
    """The value of OCP e4m3 code `code` (1 sign, 4 exponent bits with bias 7, 3 mantissa bits; 0x7f / 0xff are NaN), from the definition."""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    assert not (e == 15 and m == 7), "NaN code"
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


FINITE_CODES = [c for c in range(256) if c not in (0x7f, 0xff)]          # 254 of them, both zeros included
assert len(FINITE_CODES) == 254


def table_quantize(Wm: torch.Tensor):
    """[N][K] fp32 (CPU) -> (codes uint8 [N][K], scale fp32 [N], exponent list): the issue's rule, written without torch's float8 cast.
    e from math.frexp of the row's amax; each element takes the nearest of the non-negative table values in fp64 (exact: every candidate
    and every w * 2^-e is a double), a tie goes to the even code; the sign bit is the weight's."""
    pos = torch.tensor([e4m3_value(c) for c in range(0x7f)], dtype=torch.float64)      # codes 0 .. 0x7e ascending
    mids = (pos[1:] + pos[:-1]) / 2
    Wd = Wm.double()
    codes = torch.empty(Wm.shape, dtype=torch.uint8)
    scale, exps = torch.empty(Wm.shape[0]), []
    for n in range(Wm.shape[0]):
        amax = float(Wd[n].abs().max())
        if amax == 0.0:
            e = 0
        else:
            m, x = math.frexp(amax)
            e = x - 9 if m <= 0.875 else x - 8
        e = max(-100, min(100, e))
        exps.append(e)
        scale[n] = 2.0 ** e
        v = Wd[n].abs() * 2.0 ** -e
        assert float(v.max()) <= 448.0
        lo = torch.searchsorted(mids, v, right=False)                     # v <= mids[lo]: the nearest is lo, or lo / lo + 1 on a tie
        tie = (lo < mids.numel()) & (v == mids[lo.clamp(max=mids.numel() - 1)])
        lo = torch.where(tie & (lo % 2 == 1), lo + 1, lo)                 # ties to the even code
        sign = torch.signbit(Wm[n]).to(torch.int64) << 7
        codes[n] = (lo | sign).to(torch.uint8)
    return codes, scale, exps


def w8_index(n, k, K):
    """include/ssrhip.h SSRHIP_W8_INDEX"""
    return (n * (K // 1024) + k // 1024) * 1024 + ((k % 1024 % 256) // 4) * 16 + ((k % 1024) // 256) * 4 + k % 4


def quantized_weights(name, G, N, K, seed):
    """(fp32 master [G][N][K] = codes * scale, packed codes, scales [G][N], the packed buffer unpacked and scaled again) on the GPU, from
    the draws tests/helpers_w16.py rounds to bf16"""
    raw = W.make_tensor(f"{name}{G}.{N}.{K}", (G, N, K), f"lin:{K}", seed, device="cuda")
    codes, scale = quantize_e4m3(raw)
    master = e4m3_master(codes, scale)
    packed = to_w8_order(codes)
    unpacked = e4m3_master(from_w8_order(packed), scale)
    assert torch.equal(unpacked, master) and not bool(((codes & 0x7f) == 0x7f).any())
    return master, packed, scale.contiguous(), unpacked


def check_launch(L, B, G, N, K, pro, act, epi, kv_pos=(130, 7, 383, 256), max_pages=3, x=None, part_ml=None, lens=None, dead=float("nan")):
    """ssrhip_gemv_w8 on codes + scales against ssrhip_gemv on the master: the same bits in the whole output buffer (pad included) and the
    whole KV pool, then against torch fp64 on the UNPACKED PACKED BUFFER times the scales, which does not depend on the fp32 kernel.
    x / part_ml: as in helpers_w16.check_launch (ill-conditioned draws; the fp64 bound then follows helpers_conditioning's rule).
    lens / dead: as there (the merge prologue's row lengths, the fill of its dead pages). Returns the packed launch's whole output buffer."""
    x_given, part_ml_given = x, part_ml
    seed = B * 100003 + N * 7 + K + pro
    g = torch.Generator().manual_seed(seed)
    Wf, packed, scale, Wu = quantized_weights("w16.", G, N, K, seed)
    bias = torch.randn(G, N, generator=g).cuda()
    qkv, combine = epi == _lib.EPI_QKV_APPEND, pro == _lib.PRO_ATTN_COMBINE
    x = (torch.randn(B, G * K, generator=g) * 1.5 + 0.3).cuda()
    if x_given is not None:
        x = x_given.reshape(B, G * K).cuda()
    ny = K if qkv else G * N
    yv = (torch.randn(B, ny, generator=g) if epi == _lib.EPI_RESIDUAL else torch.full((B, ny), POISON)).cuda()
    xbuf = x.reshape(-1).clone()
    y0 = torch.cat([yv.reshape(-1), torch.full((PAD,), POISON, device="cuda")])
    n_y = y0.numel() - PAD
    pool0 = kv_pool(B, max_pages, qkv)
    table = torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32).cuda()
    pos_l = list(kv_pos[:B])
    pos = torch.tensor(pos_l, dtype=torch.int32).cuda()
    if combine:
        lens_l = [300, 129, 384, 1][:B] if lens is None else list(lens)
        lens = torch.tensor(lens_l, dtype=torch.int32).cuda()
        part_o = torch.randn(B, H, max_pages, HD, generator=g)
        part_ml = torch.stack([torch.randn(B, H, max_pages, generator=g) * 2, torch.rand(B, H, max_pages, generator=g) + 0.5], dim=-1).contiguous()
        if part_ml_given is not None:
            part_ml = part_ml_given.clone()
        pages = [(n + _lib.PAGE - 1) // _lib.PAGE for n in lens_l]
        HP.fill_dead(part_o, part_ml, lens_l, dead)
        d_po, d_pml = part_o.cuda(), part_ml.cuda()

    def run(use_packed):
        y, pool = y0.clone(), pool0.clone()
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = Wf.data_ptr(), bias.data_ptr(), xbuf.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
        a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
        if qkv:
            a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), max_pages, N_LAYER, H, HD)
            a.layer, a.kv_pos = LAYER, pos.data_ptr()
        if combine:
            a.x = 0
            a.part_o, a.part_ml, a.max_splits, a.row_len = d_po.data_ptr(), d_pml.data_ptr(), max_pages, lens.data_ptr()
            a.kv = _lib.KV(0, 0, max_pages, 1, H, HD)
        if use_packed:
            assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 1
            rc = L.ssrhip_gemv_w8(C.byref(a), packed.data_ptr(), scale.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (rc, L.ssrhip_last_error())
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y, pool

    y8, pool8 = run(True)
    y32, pool32 = run(False)
    assert torch.equal(y8, y32), float((y8 - y32).abs().max())            # whole buffers, pad included
    assert torch.equal(pool8, pool32)
    assert torch.equal(y8[n_y:], y0[n_y:])
    if combine:
        xin = torch.zeros(B, 1, K, dtype=torch.float64)
        for b in range(B):
            m, l_ = part_ml[b, :, :pages[b], 0].double(), part_ml[b, :, :pages[b], 1].double()
            e = torch.exp(m - m.max(dim=1, keepdim=True).values)
            w = e / (e * l_).sum(dim=1, keepdim=True)
            xin[b, 0] = (w.unsqueeze(-1) * part_o[b, :, :pages[b]].double()).sum(dim=1).reshape(-1)
        xin = xin.cuda()
    else:
        xin = x.view(B, G, K).double()
        if pro == _lib.PRO_LAYERNORM:
            xin = F.layer_norm(xin, (K,), None, None, 1e-5)
    ref = torch.stack([F.linear(xin[:, k], Wu[k].double(), bias[k].double()) for k in range(G)], 1)
    ref = F.relu(ref) if act == _lib.ACT_RELU else (F.gelu(ref) if act == _lib.ACT_GELU_ERF else ref)
    ref = ref.reshape(B, G * N)
    if epi == _lib.EPI_RESIDUAL:
        ref = ref + yv.double()
    got = y8[:n_y].view(B, ny)
    assert torch.isfinite(got).all()
    if qkv:
        err = float((got.double() - ref[:, :K]).abs().max())
        untouched = torch.ones_like(pool0, dtype=torch.bool)
        for b in range(B):
            page = int(table[b, pos_l[b] // _lib.PAGE])
            for which in (0, 1):
                row = pool8[page, LAYER, which, :, pos_l[b] % _lib.PAGE, :].reshape(-1)
                err = max(err, float((row.double() - ref[b, (1 + which) * K:(2 + which) * K]).abs().max()))
            untouched[page, LAYER, :, :, pos_l[b] % _lib.PAGE, :] = False
        assert torch.equal(pool8[untouched], pool0[untouched])            # nothing but the appended positions was written
    else:
        err = float((got.double() - ref).abs().max())
    print(f"B={B} G={G} N={N} K={K} pro={pro}: max |w8 - fp64| = {err:.3e}")
    tol = TOL
    if x_given is not None or part_ml_given is not None:
        y_res = yv if epi == _lib.EPI_RESIDUAL else None
        if combine:
            tol = HC.gemv_chain_tol(TOL, Wu, bias, act, y_res, part_o=part_o, part_ml=part_ml, lens=lens_l)
        else:
            tol = HC.gemv_chain_tol(TOL, Wu, bias, act, y_res, x=x, ln=pro == _lib.PRO_LAYERNORM)
    if combine:
        torch.testing.assert_close(got, ref.float(), rtol=tol, atol=tol)
    else:
        assert err < tol, err
    return y8


def check_refusal(L, B, N, K):
    """A shape ssrhip_gemv_w8 does not take: it answers 1, nothing is launched, and the caller's ssrhip_gemv takes it."""
    codes, scale = quantize_e4m3(torch.randn(N, K, generator=torch.Generator().manual_seed(2)).cuda())
    master = e4m3_master(codes, scale)
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((B * N + PAD,), POISON).cuda()
    a = _lib.GemvArgs()
    a.W, a.x, a.y = master.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, N
    assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 0
    assert L.ssrhip_gemv_w8(C.byref(a), codes.data_ptr(), scale.data_ptr(), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:B * N].view(B, N).cpu(), F.linear(x.cpu(), master.cpu()), rtol=TOL, atol=TOL)
    assert bool((y[B * N:] == POISON).all())


def check_engine_steps(args, arena8, arena16, n_utt, use_cfg, grow):
    """A stream_w8=True engine against a stream_w8=False engine of the same e4m3 arena: the same post-edit logits at each of 24 single steps
    and the same tokens, greedy and sampled, eager and as a graph (at 2 rows also against an engine that may pair); every GEMV launch of
    the packed engine ran an e4m3-stream kernel, the other streams' switches and counters stay off / 0, the steps allocate nothing, the
    packed engine steps unpaired and names the stream. The greedy eager logits also DIFFER from a bf16 arena's engine on the same prompts."""
    mk = lambda arena, **kw: DecodeEngine(arena, n_utt, use_cfg, 256, 64, debug_logits=True, **kw)
    engines = dict(packed=mk(arena8, stream_w8=True), masters=mk(arena8, stream_w8=False, pair_mode=1))
    if engines["packed"].B == 2:
        engines["paired"] = mk(arena8, stream_w8=False, pair_mode=0)
    noise = torch.empty(n_utt, 64, args.n_codebooks, arena8.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        for greedy in (True, False):
            for use_graph in (False, True):
                out = {name: _trace(e, args, n_utt, use_cfg, greedy, use_graph, None if greedy else noise, grow) for name, e in engines.items()}
                for name, e in engines.items():
                    if name == "paired" and not e.pairing:
                        continue
                    assert e.stream_w8 is (name == "packed"), name
                    assert e.w8_launches_per_step == (4 * LAYERS + 2 if name == "packed" else 0), (name, e.w8_launches_per_step)
                    for st in W16_STREAMS:
                        assert getattr(e, "stream_" + st.name) is False and getattr(e, st.name + "_launches_per_step") == 0, (name, st.name)
                assert engines["packed"].pairing is False and "e4m3" in engines["packed"].pairing_why, engines["packed"].pairing_why
                assert engines["masters"].pairing is False
                lg8, tok8, allocs8 = out["packed"]
                assert torch.isfinite(lg8).all() and allocs8 == 0, allocs8
                for name in engines:
                    if name == "packed" or (name == "paired" and not engines[name].pairing):
                        continue
                    lg, tok, _ = out[name]
                    for s in range(STEPS):
                        assert torch.equal(lg8[s], lg[s]), (name, greedy, use_graph, s, float((lg8[s] - lg[s]).abs().max()))
                    assert torch.equal(tok8, tok), (name, greedy, use_graph)
                if greedy and not use_graph:                              # not silently a bf16 model
                    e16 = mk(arena16, pair_mode=1)                # (never asks for the pairing slot the third engine may hold)
                    try:
                        lg16, _, _ = _trace(e16, args, n_utt, use_cfg, True, False, None, grow)
                    finally:
                        e16.close()
                    assert not torch.equal(lg8[0], lg16[0])
    finally:
        for e in engines.values():
            e.close()
