"""GPU: the opt-in bf16 KV cache of the 5..32-row decode step (DESIGN.md Part I.14).

A cache entry is the upper half of an fp32 value rounded to nearest even; every writer rounds (the QKV append of the step, the prefill's
scatter), every reader widens with a 16-bit shift, which is exact, and runs the fp32 kernel's arithmetic in its order and with its lane
map. So every launch-level comparison is `torch.equal` against the existing fp32 entry point on the widened pool (whole poisoned output
buffers, pads included), and the writers are held bit for bit to `.to(torch.bfloat16)`. At engine level the per-step logits are held to the
oracle whose attention sees bf16-valued K / V (tests/helpers_kv16.py; tests/test_kv16_host.py shows that an fp32 cache cannot pass) within
the 2e-4 that tests/test_gpu_lm.py holds the fp32 engine to."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_kv16 as HK
from helpers_w16 import L, arena16, tiny2048  # noqa: F401  (module-scoped fixtures)
from helpers_w16 import PAD, POISON, _trace, from_panels, shape_weights, to_panels, to_tiled
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

PAGE = _lib.PAGE
N_LAYER, LAYER = 2, 1
POISON16 = 0x7B7B                       # int16 pattern of an untouched 2-byte entry (a large finite bf16)
LENS = [1, 127, 128, 129, 257, 385]     # one page, a page edge, an odd page count (the clamped second buffer), four pages


def _poisoned_out(n):
    return torch.full((n + PAD,), POISON, device="cuda")


def _filled_pool(g, n_pages, Hh, hd, seq_pages, seq_len):
    """bf16 pool [n_pages + 1][N_LAYER][2][Hh][PAGE][hd] as int16: random bf16 values at the positions < seq_len[s] of layer LAYER in the
    pages seq_pages[s] of sequence s, POISON16 everywhere else (the other layer, the tails of pages, unused pages, the spare page)"""
    vals = HK.bf16_bits(torch.randn(n_pages + 1, 2, Hh, PAGE, hd, generator=g))
    pool = torch.full((n_pages + 1, N_LAYER, 2, Hh, PAGE, hd), POISON16, dtype=torch.int16)
    for pages, n in zip(seq_pages, seq_len):
        for p in range((n + PAGE - 1) // PAGE):
            k = min(PAGE, n - p * PAGE)
            pool[pages[p], LAYER, :, :, :k] = vals[pages[p], :, :, :k]
    return pool.cuda()


def _attn_args(q, pool, table, max_pages, Hh, hd, row_seq, row_len, R, out_tiled=0):
    a = _lib.AttnArgs()
    a.q, a.q_stride = q.data_ptr(), 0
    a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), max_pages, N_LAYER, Hh, hd)
    a.layer, a.row_seq, a.row_len = LAYER, _lib.ptr(row_seq), _lib.ptr(row_len)
    a.R, a.max_splits, a.scale, a.out_tiled = R, max_pages, 1.0 / math.sqrt(hd), out_tiled
    return a


# ------------------------------------------------------------------------------------------ launch level: the readers
@functools.lru_cache(maxsize=None)
def _rows_case(hd, R):
    """The operands of one (head_dim, R) case, built once and never modified: row lengths cycling through LENS, a `row_seq` that is not
    the identity, a permuted page table, the poisoned 2-byte pool and its widened fp32 twin"""
    Hh, max_pages = 2, 4
    g = torch.Generator().manual_seed(R * 1000 + hd)
    lens = [LENS[(r + R) % len(LENS)] for r in range(R)]
    row_seq = torch.randperm(R, generator=g)                                  # row r reads sequence row_seq[r]
    assert not torch.equal(row_seq, torch.arange(R))
    n_pages = R * max_pages
    perm = torch.randperm(n_pages, generator=g).view(R, max_pages)            # entries past a sequence's pages: the spare page
    seq_len = [0] * R
    for r in range(R):
        seq_len[int(row_seq[r])] = lens[r]
    table = torch.full((R, max_pages), n_pages, dtype=torch.int32)
    for s in range(R):
        npg = (seq_len[s] + PAGE - 1) // PAGE
        table[s, :npg] = perm[s, :npg].to(torch.int32)
    pool16 = _filled_pool(g, n_pages, Hh, hd, [table[s].tolist() for s in range(R)], seq_len)
    q = torch.randn(R, Hh * hd, generator=g).cuda()
    return lens, row_seq, table, pool16, HK.widen(pool16), q, table.cuda(), row_seq.to(torch.int32).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


@pytest.mark.parametrize("depth", ["2", "4"])
@pytest.mark.parametrize("out_tiled", [0, 1])
@pytest.mark.parametrize("R", [5, 16, 17, 32])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_rows_kv16_equals_attn_rows_on_the_widened_pool(L, monkeypatch, hd, R, out_tiled, depth):
    Hh, max_pages = 2, 4
    D = Hh * hd
    lens, row_seq, table, pool16, pool32, q, d_table, d_seq, d_len = _rows_case(hd, R)
    n_out = (16 * ((R + 15) // 16) if out_tiled else R) * D
    out16, out32 = _poisoned_out(n_out), _poisoned_out(n_out)
    monkeypatch.setenv("SSRHIP_ATTN_KV16_DEPTH", depth)                       # read at every launch
    a16 = _attn_args(q, pool16, d_table, max_pages, Hh, hd, d_seq, d_len, R, out_tiled)
    a32 = _attn_args(q, pool32, d_table, max_pages, Hh, hd, d_seq, d_len, R, out_tiled)
    _lib.check(L.ssrhip_attn_rows_kv16(C.byref(a16), out16.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_rows_kv16")
    _lib.check(L.ssrhip_attn_rows(C.byref(a32), out32.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_rows")
    torch.cuda.synchronize()
    assert torch.equal(out16, out32), float((out16 - out32).abs().max())      # the whole poisoned buffer and the pad
    assert torch.equal(out16[n_out:], torch.full((PAD,), POISON, device="cuda"))
    rows = (from_panels(out16[:32 * D], R, D) if R > 16 else out16[:n_out].view(D // 4, 16, 4)[:, :R].permute(1, 0, 2).reshape(R, D)) if out_tiled \
        else out16[:n_out].view(R, D)
    assert torch.isfinite(rows).all()                                         # no poisoned entry was folded in
    r1 = lens.index(1)                                                        # a row of length 1 returns its only value row
    v0 = pool32[int(table[int(row_seq[r1]), 0]), LAYER, 1, :, 0, :].reshape(-1)
    assert torch.equal(rows[r1], v0)


@pytest.mark.parametrize("hd", [64, 128])
def test_attn_prefill_kv16_equals_attn_prefill_on_the_widened_pool(L, hd):
    Hh, max_pages = 2, 3
    D = Hh * hd
    g = torch.Generator().manual_seed(hd)
    seg_len = [1, 129, 300]
    seg_seq = [2, 0, 1]                                                       # segment i fills sequence seg_seq[i] (row_seq set)
    R = sum(seg_len)
    n_pages = 3 * max_pages
    table = torch.randperm(n_pages, generator=g).view(3, max_pages).to(torch.int32)
    seq_len = [0, 0, 0]
    for n, s in zip(seg_len, seg_seq):
        seq_len[s] = n
    pool16 = _filled_pool(g, n_pages, Hh, hd, [table[s].tolist() for s in range(3)], seq_len)
    pool32 = HK.widen(pool16)
    q = torch.randn(R, D, generator=g).cuda()
    seq_start = torch.tensor(np.concatenate([[0], np.cumsum(seg_len)]), dtype=torch.int32).cuda()
    row_seq = torch.tensor(sum(([s] * n for n, s in zip(seg_len, seg_seq)), []), dtype=torch.int32).cuda()
    d_table = table.cuda()
    out16, out32 = _poisoned_out(R * D), _poisoned_out(R * D)
    a16 = _attn_args(q, pool16, d_table, max_pages, Hh, hd, row_seq, None, R)
    a32 = _attn_args(q, pool32, d_table, max_pages, Hh, hd, row_seq, None, R)
    _lib.check(L.ssrhip_attn_prefill_kv16(C.byref(a16), seq_start.data_ptr(), 3, max(seg_len), out16.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_prefill_kv16")
    _lib.check(L.ssrhip_attn_prefill(C.byref(a32), seq_start.data_ptr(), 3, max(seg_len), out32.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_prefill")
    torch.cuda.synchronize()
    assert torch.equal(out16, out32), float((out16 - out32).abs().max())
    assert torch.isfinite(out16[:R * D]).all() and bool((out16[R * D:] == POISON).all())
    v0 = pool32[int(table[2, 0]), LAYER, 1, :, 0, :].reshape(-1)              # the one-row sequence: its query sees key 0 only
    assert torch.equal(out16[:D], v0)


# ------------------------------------------------------------------------------------------ launch level: the writers
def test_kv_scatter16_rounds_like_torch_and_writes_nothing_else(L):
    Hh, hd, max_pages = 2, 64, 2
    D = Hh * hd
    g = torch.Generator().manual_seed(7)
    pos = [126, 127, 128, 129, 0, 1, 2]                                       # sequence 0 crosses the page edge
    seq = [0, 0, 0, 0, 1, 1, 1]
    R = len(pos)
    qkv = torch.randn(R, 3 * D, generator=g) * 3
    sp = HK.special_values()
    qkv[1, D + 5:D + 5 + sp.numel()] = sp                                     # ties, +-0, denormals, overflow, +-inf: in K ...
    qkv[5, 2 * D + 64:2 * D + 64 + sp.numel()] = sp.flip(0)                   # ... and in V
    table = torch.tensor([[3, 1], [0, 2]], dtype=torch.int32)
    pool0 = torch.full((4 + 1, N_LAYER, 2, Hh, PAGE, hd), POISON16, dtype=torch.int16)
    expect = pool0.clone()
    bits = qkv.to(torch.bfloat16).view(torch.int16)                           # torch's own conversion (CPU)
    for r in range(R):
        page = int(table[seq[r], pos[r] // PAGE])
        for which in (0, 1):
            expect[page, LAYER, which, :, pos[r] % PAGE, :] = bits[r, (1 + which) * D:(2 + which) * D].view(Hh, hd)
    pool, d_qkv, d_table = pool0.cuda(), qkv.cuda(), table.cuda()
    d_seq, d_pos = torch.tensor(seq, dtype=torch.int32).cuda(), torch.tensor(pos, dtype=torch.int32).cuda()
    kv = _lib.KV(pool.data_ptr(), d_table.data_ptr(), max_pages, N_LAYER, Hh, hd)
    _lib.check(L.ssrhip_kv_scatter16(d_qkv.data_ptr(), C.byref(kv), LAYER, d_seq.data_ptr(), d_pos.data_ptr(), R, _lib.stream_ptr()), "ssrhip_kv_scatter16")
    torch.cuda.synchronize()
    assert torch.equal(pool.cpu(), expect)                                    # the touched entries bit for bit, every other entry unchanged
    assert int((expect != POISON16).sum()) == R * 2 * D


@functools.lru_cache(maxsize=None)
def _append_weights(K):
    return shape_weights("kv16.", 1, 3 * K, K)


def _append_case(L, B, K, Hh, hd, path, pro):
    """The QKV launch with EPI_QKV_APPEND on an fp32 pool and with EPI_QKV_APPEND16 on a 2-byte pool, through `path`"""
    N, max_pages = 3 * K, 2
    Wt, packed, Wrm, bias = _append_weights(K)
    g = torch.Generator().manual_seed(B * 31 + K)
    x = (torch.randn(B, K, generator=g) * 1.5 + 0.3).cuda()
    tiled = path != "rowmajor"
    xbuf = (to_panels(x) if B > 16 else to_tiled(x)) if tiled else x.reshape(-1).clone()
    pos_l = [[127, 128, 0][b % 3] for b in range(B)]
    table = torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32)
    spare_row = 4 % B
    table[spare_row] = B * max_pages                                           # a row whose table points at the spare page
    d_table, d_pos = table.cuda(), torch.tensor(pos_l, dtype=torch.int32).cuda()
    shape = (B * max_pages + 1, N_LAYER, 2, Hh, PAGE, hd)
    pool32_0 = torch.full(shape, POISON, device="cuda")
    pool16_0 = torch.full(shape, POISON16, dtype=torch.int16, device="cuda")

    def run(epi, pool):
        y = _poisoned_out(B * K)
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = (Wt if tiled else Wrm).data_ptr(), bias.data_ptr(), xbuf.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, K
        a.pro, a.act, a.epi, a.ln_eps = pro, _lib.ACT_NONE, epi, 1e-5
        a.x_tiled, a.y_tiled, a.w_tiled = int(tiled), 0, int(tiled)
        a.kv = _lib.KV(pool.data_ptr(), d_table.data_ptr(), max_pages, N_LAYER, Hh, hd)
        a.layer, a.kv_pos = LAYER, d_pos.data_ptr()
        if path == "packed":
            name = "ssrhip_gemv_wt16" if B <= 16 else "ssrhip_gemv_wt32"
            rc = getattr(L, name)(C.byref(a), packed.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (name, rc, L.ssrhip_last_error())                  # it took the launch (1 would be "does not qualify")
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()), "ssrhip_gemv")
        torch.cuda.synchronize()
        return y

    p32, p16 = pool32_0.clone(), pool16_0.clone()
    y32, y16 = run(_lib.EPI_QKV_APPEND, p32), run(_lib.EPI_QKV_APPEND16, p16)
    assert torch.equal(y16, y32)                                              # q bit for bit, pad included
    written = torch.zeros(shape, dtype=torch.bool, device="cuda")
    for b in range(B):
        written[int(table[b, pos_l[b] // PAGE]), LAYER, :, :, pos_l[b] % PAGE, :] = True
    assert bool((p32[written] != POISON).all()) and torch.equal(p32[~written], pool32_0[~written])
    expect = pool16_0.clone()
    expect[written] = p32[written].to(torch.bfloat16).view(torch.int16)
    assert torch.equal(p16, expect)                                           # the appended entries are .to(bfloat16) of the fp32 launch's; nothing else moved


@pytest.mark.parametrize("pro", [_lib.PRO_LAYERNORM, _lib.PRO_NONE], ids=["ln", "plain"])
@pytest.mark.parametrize("path", ["rowmajor", "wtiled", "packed"])
@pytest.mark.parametrize("B", [5, 16, 17, 32])
@pytest.mark.parametrize("K,Hh,hd", [(128, 2, 64), (2048, 16, 128)])
def test_qkv_append16_rounds_the_fp32_launchs_entries(L, K, Hh, hd, B, path, pro):
    _append_case(L, B, K, Hh, hd, path, pro)


@pytest.mark.parametrize("B", [1, 2, 4])
def test_qkv_append16_is_refused_at_four_rows_and_below(L, B):
    K, Hh, hd = 128, 2, 64
    _, _, Wrm, bias = _append_weights(K)
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(B)).cuda()
    y = _poisoned_out(B * K)
    pool = torch.full((B * 2 + 1, N_LAYER, 2, Hh, PAGE, hd), POISON16, dtype=torch.int16, device="cuda")
    table = torch.arange(B * 2, dtype=torch.int32).view(B, 2).cuda()
    pos = torch.zeros(B, dtype=torch.int32).cuda()
    a = _lib.GemvArgs()
    a.W, a.bias, a.x, a.y = Wrm.data_ptr(), bias.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, 3 * K, K, 1, K, K
    a.pro, a.epi, a.ln_eps = _lib.PRO_LAYERNORM, _lib.EPI_QKV_APPEND16, 1e-5
    a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), 2, N_LAYER, Hh, hd)
    a.layer, a.kv_pos = LAYER, pos.data_ptr()
    assert L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert bool((pool == POISON16).all()) and bool((y == POISON).all())


# ------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _arena(cfg):
    args, sd = HK.model_cpu(cfg)
    return args, LMWeightsArena(args, {k: v.cuda() for k, v in sd.items()}, torch.device("cuda"))


def _steps(eng, args, seeds, use_graph):
    """24 single steps from a fresh start: (logits [STEPS][n_utt][K][card], tokens [n_utt][STEPS][K], device allocations during the steps)"""
    rows, cols, knobs = HK.engine_inputs(args, seeds)
    eng.start(rows, cols, knobs, noise=None)
    torch.cuda.synchronize()
    allocs0 = torch.cuda.memory_stats()["num_device_alloc"]
    logits = []
    for _ in range(HK.STEPS):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        logits.append(eng.dbg_logits.cpu().numpy().copy())
    return np.stack(logits), eng.generated[:, :HK.STEPS].cpu().numpy(), torch.cuda.memory_stats()["num_device_alloc"] - allocs0


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cfg,n_utt", [("d128", 3), ("d1024", 8), ("d1024", 16)])
def test_kv16_engine_matches_the_oracle_with_bf16_valued_kv(monkeypatch, cfg, n_utt, use_graph):
    args, arena = _arena(cfg)
    seeds = list(range(1, n_utt + 1))
    eng = DecodeEngine(arena, n_utt, True, 256, 64, debug_logits=True, kv_dtype="bf16")
    try:
        assert eng.kv_dtype == "bf16" and eng.kv_pool.dtype == torch.bfloat16 and eng.kv_pool_bytes == 2 * eng.kv_pool.numel()
        lg, tok, allocs = _steps(eng, args, seeds, use_graph)
        assert eng.kv16_launches_per_step == args.num_decoder_layers          # every attention launch read the 2-byte cache: no fallback
        assert allocs == 0, allocs
    finally:
        eng.close()
    worst = 0.0
    for u, seed in enumerate(seeds):
        ref_lg, ref_tok = HK.oracle_trace(monkeypatch, cfg, seed, True)
        n = ref_lg.shape[0]                                                   # STEPS, or fewer if the utterance ended earlier
        assert n >= 8 and np.array_equal(tok[u, :n], ref_tok), (u, tok[u], ref_tok)
        finite = np.isfinite(ref_lg)
        assert np.array_equal(np.isfinite(lg[:n, u]), finite)
        err = np.abs(np.where(finite, lg[:n, u] - ref_lg, 0.0)).max()
        worst = max(worst, float(err))
        assert err <= HK.LOGIT_ATOL, (u, err)
    print(f"{cfg} {2 * n_utt} rows {'graph' if use_graph else 'eager'}: max |logit - shimmed oracle| over {HK.STEPS} steps = {worst:.2e}")


@pytest.mark.parametrize("cfg,n_utt", [("d128", 3), ("d1024", 8)])
def test_prefill_writes_the_rounded_layer0_entries_of_the_fp32_engine(cfg, n_utt):
    """Layer 0's K / V do not depend on attention: after start() they are `.to(bfloat16)` of the fp32 engine's, bit for bit"""
    args, arena = _arena(cfg)
    rows, cols, knobs = HK.engine_inputs(args, list(range(1, n_utt + 1)))
    pools = {}
    for dt in ("fp32", "bf16"):
        eng = DecodeEngine(arena, n_utt, True, 256, 64, kv_dtype=dt)
        try:
            eng.start(rows, cols, knobs, noise=None)
            torch.cuda.synchronize()
            shape = (-1, arena.L, 2, arena.H, PAGE, eng.hd)
            pools[dt] = (eng.kv_pool.view(shape)[:, 0].clone(), [list(p) for p in eng._row_pages], list(eng._kv0))
        finally:
            eng.close()
    (p32, pages32, len32), (p16, pages16, len16) = pools["fp32"], pools["bf16"]
    assert pages32 == pages16 and len32 == len16 and min(len32) > 0
    assert p16.dtype == torch.bfloat16 and p16.numel() == p32.numel()
    for b, n in enumerate(len32):
        for p in range((n + PAGE - 1) // PAGE):
            k = min(PAGE, n - p * PAGE)
            want = p32[pages32[b][p], :, :, :k].to(torch.bfloat16).view(torch.int16)
            assert torch.equal(p16[pages16[b][p], :, :, :k].view(torch.int16), want), (b, p)


@pytest.mark.parametrize("n_utt,stream", [(8, "wt16"), (16, "wt32")])
def test_kv16_is_independent_of_the_weight_stream(tiny2048, arena16, n_utt, stream):
    args, _ = tiny2048
    out = {}
    for on in (True, False):
        eng = DecodeEngine(arena16, n_utt, True, 256, 64, debug_logits=True, kv_dtype="bf16", **{"stream_" + stream: on})
        try:
            out[on] = _trace(eng, args, n_utt, True, True, True, None, (2, 3))
            assert eng.kv16_launches_per_step == args.num_decoder_layers
            assert getattr(eng, stream + "_launches_per_step") == (4 * args.num_decoder_layers + 2 if on else 0)
        finally:
            eng.close()
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert torch.isfinite(out[True][0]).all() and out[True][2] == 0


def _queue_utts(n):
    g = torch.Generator().manual_seed(14)
    utts = []
    for i in range(n):
        Lt, T = int(torch.randint(6, 15, (1,), generator=g)), int(torch.randint(5, 40, (1,), generator=g))
        utts.append(dict(x=torch.randint(0, 30, (1, Lt), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g), mask_interval=torch.LongTensor([[[T, T]]])))
    return utts


def _model(cfg):
    args, sd = HK.model_cpu(cfg)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


QUEUE_KW = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)


def test_run_queue_with_refill_under_kv16(monkeypatch):
    """10 utterances through 3 slots x CFG: blocking admission and two-phase admission give the same tokens, and both match the same
    engine decoding the utterances in fixed groups of three (no refill) — every prefill path rounds, every attention widens"""
    m = _model("d128")
    m.set_kv_dtype("bf16")
    utts = _queue_utts(10)
    res = {}
    for two_phase in ("0", "1"):
        monkeypatch.setenv("SSRHIP_ADMIT_TWO_PHASE", two_phase)
        res[two_phase] = m.inference_batch(utts, seed=40, group=3, **QUEUE_KW)
        eng = next(iter(m._engines.values()))
        assert eng.kv_dtype == "bf16" and eng.B == 6 and eng.n_admitted == 10 and eng.n_refills == 7
        assert eng.kv16_launches_per_step == m.args.num_decoder_layers
    monkeypatch.delenv("SSRHIP_ADMIT_TWO_PHASE")
    fixed = m.inference_batch(utts[:9], seed=40, group=3, refill=False, **QUEUE_KW) + m.inference_batch(utts[6:], seed=46, group=4, refill=False, **QUEUE_KW)[3:]
    assert next(iter(m._engines.values())).kv_dtype == "bf16"
    for i in range(10):
        for other in (res["1"], fixed):
            assert torch.equal(res["0"][i][0], other[i][0]) and torch.equal(res["0"][i][1], other[i][1]) and res["0"][i][2] == other[i][2], i


def test_public_surface(monkeypatch):
    cfg = "d128"
    args, arena = _arena(cfg)
    m = _model(cfg)
    utts = _queue_utts(8)
    fp32 = m.inference_batch(utts, seed=9, **QUEUE_KW)
    assert next(iter(m._engines.values())).kv_dtype == "fp32" and next(iter(m._engines.values())).kv16_launches_per_step == 0
    m.set_kv_dtype("bf16")
    assert m.kv_dtype == "bf16" and not m._engines
    bf16 = m.inference_batch(utts, seed=9, **QUEUE_KW)
    eng = next(iter(m._engines.values()))
    assert eng.kv_dtype == "bf16" and eng.B == 16 and eng.kv16_launches_per_step == args.num_decoder_layers
    # the engine-level run of the same utterances: the kv16 engine decoding them as one fixed group gives these tokens
    again = m.inference_batch(utts, seed=9, refill=False, **QUEUE_KW)
    for i in range(8):
        assert torch.equal(bf16[i][0], again[i][0]) and bf16[i][2] == again[i][2], i
    # the 2-row path keeps fp32 K / V under the switch
    u = utts[0]
    Lt = u["x"].shape[1]
    torch.manual_seed(9)
    one16 = m.inference(u["x"].cuda(), torch.LongTensor([Lt]), u["x"].cuda(), torch.LongTensor([Lt]), u["y"].cuda(), u["y"].cuda(), u["mask_interval"].cuda(), kvcache=1, **QUEUE_KW)
    assert next(iter(m._engines.values())).kv_dtype == "fp32"
    m.set_kv_dtype("fp32")
    assert not m._engines
    back = m.inference_batch(utts, seed=9, **QUEUE_KW)
    for i in range(8):
        assert torch.equal(back[i][0], fp32[i][0]) and torch.equal(back[i][1], fp32[i][1]) and back[i][2] == fp32[i][2] and back[i][3] == fp32[i][3], i
    assert torch.equal(one16[0], fp32[0][0])                                  # ... so it equals the fp32 batch row (the batch-1 parity contract)
    with pytest.raises(ValueError, match="5..32 rows"):
        DecodeEngine(arena, 1, True, 256, 64, kv_dtype="bf16")
    with pytest.raises(ValueError, match="256 pages"):
        DecodeEngine(arena, 3, True, 257 * PAGE, 64, kv_dtype="bf16")
