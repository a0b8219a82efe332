"""GPU: the opt-in bf16 KV cache of the 1/2/4-row decode step (DESIGN.md Part I.23).

The QKV launch of such an engine is the fp32 engine's launch with another destination: it appends fp32 K / V into a small landing cache.
`ssrhip_attn_decode_kv16` reads the pool as 2-byte entries, takes the position this step appended from the landing cache, rounds it to
nearest even once, uses the ROUNDED values and stores them into the pool. Widening is exact and the arithmetic behind it is
`ssrhip_attn_decode`'s in its order, so the launch-level comparisons are bit for bit (on the raw bits: some inputs are infinite on purpose)
against the fp32 entry point on the widened pool that holds `round_bf16(landing)` at the appended position. At engine level the per-step
logits are held to the oracle whose attention sees bf16-valued K / V within the 2e-4 the fp32 engine is held to against its oracle
(tests/test_kv16_small_host.py shows on the CPU that an fp32 cache misses that bound on these inputs)."""
import ctypes as C
import functools
import gc
import math

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_kv16 as HK
import helpers_kv16_small as HS
from helpers_w16 import LAYERS, PAD, POISON, STEPS, L, _trace, _utterance, arena16, tiny2048  # noqa: F401  (module-scoped fixtures)
from oracle import lm as O
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

PAGE = _lib.PAGE
N_LAYER, LAYER, HEADS, MAX_PAGES = 3, 1, 2, 4
POISON16 = 0x7B7B                       # int16 pattern of an untouched 2-byte entry (a large finite bf16)
NAN16 = 0x7FC1                          # what the pool holds at the appended position before the launch: a NaN, never to be used
LENS = [1, 2, 127, 128, 129, 200, 257]  # the first position, a page edge from both sides, the second page's first key, three pages


def _bits(t):
    return t.contiguous().view(torch.int32)


def _len_sets(R):
    """row lengths of the launches at R rows: windows of LENS, so that every length occurs at every R, mixed within a launch"""
    return [[LENS[(i * R + k) % len(LENS)] for k in range(R)] for i in range((len(LENS) + R - 1) // R)]


@functools.lru_cache(maxsize=None)
def _launch_case(hd, R, which_set):
    """Operands of one launch, built once and never modified by the tests (launches work on clones): a shuffled page table, the 2-byte pool
    with random bf16 values below len - 1, NaN bits AT len - 1 and poison elsewhere, the landing cache (random everywhere, the special values of
    the rounding tests among layer LAYER's entries), and the fp32 twin of the pool with round_bf16(landing) at len - 1."""
    lens = _len_sets(R)[which_set]
    g = torch.Generator().manual_seed(hd * 100 + R * 10 + which_set)
    n_pages = R * MAX_PAGES
    perm = torch.randperm(n_pages, generator=g).view(R, MAX_PAGES)
    table = torch.full((R, MAX_PAGES), n_pages, dtype=torch.int32)            # entries past a row's pages: the spare page
    vals = HK.bf16_bits(torch.randn(n_pages + 1, 2, HEADS, PAGE, hd, generator=g))
    pool16 = torch.full((n_pages + 1, N_LAYER, 2, HEADS, PAGE, hd), POISON16, dtype=torch.int16)
    land = torch.randn(R, 1, 2, HEADS, PAGE, hd, generator=g)
    sp = HK.special_values()
    finite = sp[HK.round_bf16(sp).abs() < 4]                                  # ties, zeros, denormals: no product with them overflows
    land[0, 0, 0, 0, LAYER, 3:3 + sp.numel()] = sp                            # row 0, head 0: every special value, the infinite ones too, in K ...
    land[0, 0, 1, 0, LAYER, 7:7 + sp.numel()] = sp.flip(0)                    # ... and in V
    for r in range(1, R):
        land[r, 0, 0, 1, LAYER, 1:1 + finite.numel()] = finite
        land[r, 0, 1, 1, LAYER, 2:2 + finite.numel()] = finite.flip(0)
    last = []                                                                 # (page, position) of len - 1 per row
    for r, n in enumerate(lens):
        npg = (n + PAGE - 1) // PAGE
        table[r, :npg] = perm[r, :npg].to(torch.int32)
        for p in range(npg):
            k = min(PAGE, n - p * PAGE)
            pool16[perm[r, p], LAYER, :, :, :k] = vals[perm[r, p], :, :, :k]
        last.append((int(perm[r, (n - 1) // PAGE]), (n - 1) % PAGE))
        pool16[last[-1][0], LAYER, :, :, last[-1][1]] = NAN16
    pool32 = HK.widen(pool16)
    want16 = pool16.clone()
    for r, (page, j) in enumerate(last):
        pool32[page, LAYER, :, :, j] = HK.round_bf16(land[r, 0, :, :, LAYER])
        want16[page, LAYER, :, :, j] = HK.bf16_bits(land[r, 0, :, :, LAYER])
    q = torch.randn(R, HEADS * hd, generator=g)
    prefetch = torch.randn(256 * 1024, generator=g)
    dev = lambda t: t.cuda()
    return dict(lens=lens, last=last, table=dev(table), pool16=dev(pool16), pool32=dev(pool32), want16=dev(want16), land=dev(land), q=dev(q),
                row_len=dev(torch.tensor(lens, dtype=torch.int32)), prefetch=dev(prefetch))


def _attn_args(c, pool, hd, R, part_o, part_ml, prefetch):
    a = _lib.AttnArgs()
    a.q, a.q_stride = c["q"].data_ptr(), 0
    a.kv = _lib.KV(pool.data_ptr(), c["table"].data_ptr(), MAX_PAGES, N_LAYER, HEADS, hd)
    a.layer, a.row_seq, a.row_len = LAYER, 0, c["row_len"].data_ptr()
    a.R, a.max_splits, a.scale = R, MAX_PAGES, 1.0 / math.sqrt(hd)
    a.part_o, a.part_ml = part_o.data_ptr(), part_ml.data_ptr()
    if prefetch:
        a.prefetch, a.prefetch_floats = c["prefetch"].data_ptr(), 1024
    return a


# ------------------------------------------------------------------------------------------ launch level
@pytest.mark.parametrize("prefetch", [False, True], ids=["", "prefetch"])
@pytest.mark.parametrize("head_fastest", [None, "0"], ids=["headfast", "pagefast"])
@pytest.mark.parametrize("vat", [None, "-1"], ids=["vat8", "vatfree"])
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_kv16_equals_attn_decode_on_the_widened_pool_and_promotes(L, monkeypatch, hd, R, vat, head_fastest, prefetch):
    for name, v in (("SSRHIP_ATTN_VAT", vat), ("SSRHIP_ATTN_HEAD_FASTEST", head_fastest)):    # read at every launch
        monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
    n_o, n_ml = R * HEADS * MAX_PAGES * hd, R * HEADS * MAX_PAGES * 2
    for which_set in range(len(_len_sets(R))):
        c = _launch_case(hd, R, which_set)
        pool16, pool32, land = c["pool16"].clone(), c["pool32"].clone(), c["land"].clone()
        po16, po32 = torch.full((n_o + PAD,), POISON, device="cuda"), torch.full((n_o + PAD,), POISON, device="cuda")
        ml16, ml32 = torch.full((n_ml + PAD,), POISON, device="cuda"), torch.full((n_ml + PAD,), POISON, device="cuda")
        a16 = _attn_args(c, pool16, hd, R, po16, ml16, prefetch)
        a32 = _attn_args(c, pool32, hd, R, po32, ml32, False)                      # (the touch changes no result: the reference runs without)
        _lib.check(L.ssrhip_attn_decode_kv16(C.byref(a16), land.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_decode_kv16")
        _lib.check(L.ssrhip_attn_decode(C.byref(a32), _lib.stream_ptr()), "ssrhip_attn_decode")
        torch.cuda.synchronize()
        what = (hd, R, c["lens"])
        # the partials, whole poisoned buffers and pads, bit for bit (row 0 / head 0 holds infinities: raw bits)
        assert torch.equal(_bits(po16), _bits(po32)), what
        assert torch.equal(_bits(ml16), _bits(ml32)), what
        assert bool((po16[n_o:] == POISON).all()) and bool((ml16[n_ml:] == POISON).all())
        o = po16[:n_o].view(R, HEADS, MAX_PAGES, hd)
        for r, n in enumerate(c["lens"]):
            npg = (n + PAGE - 1) // PAGE
            assert bool((o[r, :, npg:] == POISON).all()), what                    # pages past the row's length: not written
            assert torch.isfinite(o[r, 1 if r == 0 else 0:, :npg]).all(), what    # (row, head)s without infinite inputs: the NaN at len - 1 never got in
            if n == 1:                                                            # one key: its page's partial is the rounded landing V itself
                h0 = 1 if r == 0 else 0
                assert torch.equal(o[r, h0:, 0], HK.round_bf16(c["land"][r, 0, 1, h0:, LAYER])), what
        # the pool: position len - 1 of every (row, head, K and V) now holds the rounded landing entry, every other entry is untouched
        assert torch.equal(pool16, c["want16"]), what
        assert int((pool16 != c["pool16"]).sum()) == R * 2 * HEADS * hd           # (NaN bits before, so every promoted entry differs)
        assert torch.equal(_bits(land), _bits(c["land"])), what                   # the landing cache is read only
        assert torch.equal(pool32, c["pool32"])


# ------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _arena(cfg):
    args, sd = HS.model_cpu(cfg)
    return args, LMWeightsArena(args, {k: v.cuda() for k, v in sd.items()}, torch.device("cuda"))


def _steps(eng, args, seeds, use_cfg, use_graph):
    """24 single steps from a fresh start: (logits [STEPS][n_utt][K][card], tokens [n_utt][STEPS][K], device allocations during the steps)"""
    rows, cols, knobs = HS.engine_inputs(args, seeds, use_cfg)
    eng.start(rows, cols, knobs, noise=None)
    torch.cuda.synchronize()
    allocs0 = torch.cuda.memory_stats()["num_device_alloc"]
    logits = []
    for _ in range(HS.STEPS):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        logits.append(eng.dbg_logits.cpu().numpy().copy())
    return np.stack(logits), eng.generated[:, :HS.STEPS].cpu().numpy(), torch.cuda.memory_stats()["num_device_alloc"] - allocs0


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("cfg", sorted(HS.CONFIGS))
def test_engine_matches_the_oracle_with_bf16_valued_kv(monkeypatch, cfg, rows, use_graph):
    monkeypatch.delenv("SSRHIP_ATTN_KV16_SMALL", raising=False)
    args, arena = _arena(cfg)
    n_utt, use_cfg = HS.ROWS[rows]
    seeds = HS.seeds_of(cfg, rows)
    eng = DecodeEngine(arena, n_utt, use_cfg, 256, 64, debug_logits=True, kv_dtype="bf16", kv16_small=True, pair_mode=1)
    try:
        assert eng.B == rows and eng.kv16_small is True and eng.kv_dtype == "bf16" and eng.kv_pool.dtype == torch.bfloat16
        entries = (eng.pages.n_pages + 1) * arena.L * 2 * arena.D * PAGE
        assert eng.kv_pool.numel() == entries and eng.kv_pool_bytes == 2 * entries            # half the fp32 pool's 4 bytes per entry
        assert eng.kv_landing_bytes == rows * 2 * arena.D * PAGE * 4
        assert eng.kv_land_table.tolist() == list(range(rows))
        assert eng.kv_land_pos.tolist() == [l for l in range(arena.L) for _ in range(rows)]
        lg, tok, allocs = _steps(eng, args, seeds, use_cfg, use_graph)
        assert eng.kv16_launches_per_step == args.num_decoder_layers           # every attention launch read the 2-byte cache: no fallback
        assert allocs == 0, allocs
        if use_graph:                                                          # the refusal after capture
            assert eng.lib.ssrhip_lm_set_kv16_small(eng._ctx, None, None, None) < 0 and b"already captured" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    worst = 0.0
    for u, seed in enumerate(seeds):
        ref_lg, ref_tok = HS.oracle_trace(monkeypatch, cfg, seed, True, use_cfg)
        n = ref_lg.shape[0]
        assert n == HS.STEPS and np.array_equal(tok[u, :n], ref_tok), (u, tok[u], ref_tok)
        finite = np.isfinite(ref_lg)
        assert np.array_equal(np.isfinite(lg[:n, u]), finite)
        err = float(np.abs(np.where(finite, lg[:n, u] - ref_lg, 0.0)).max())
        worst = max(worst, err)
        print(f"{cfg} {rows} rows {'graph' if use_graph else 'eager'} utterance {u}: max |logit - rounding oracle| over {n} steps = {err:.2e}")
        assert err <= HS.LOGIT_ATOL, (u, err)


def test_switch_unset_changes_nothing(monkeypatch):
    monkeypatch.delenv("SSRHIP_ATTN_KV16_SMALL", raising=False)
    args, arena = _arena("d128")
    with pytest.raises(ValueError, match="5..32 rows"):
        DecodeEngine(arena, 1, True, 256, 64, kv_dtype="bf16")
    with pytest.raises(ValueError, match="1/2/4-row decode step only"):
        DecodeEngine(arena, 3, True, 256, 64, kv_dtype="bf16", kv16_small=True)
    with pytest.raises(ValueError, match="kv16_small needs the bf16 cache type"):
        DecodeEngine(arena, 1, True, 256, 64, kv16_small=True)
    eng = DecodeEngine(arena, 1, True, 256, 64)
    try:
        assert eng.kv16_small is False and eng.kv_dtype == "fp32" and eng.kv_pool.dtype == torch.float32
        assert eng.kv_landing_bytes == 0 and eng.kv_land is None and eng.kv16_launches_per_step == 0
    finally:
        eng.close()
    monkeypatch.setenv("SSRHIP_ATTN_KV16_SMALL", "1")                          # the switch alone, without the cache type, changes nothing either
    eng = DecodeEngine(arena, 1, True, 256, 64)
    try:
        assert eng.kv16_small is False and eng.kv_dtype == "fp32" and eng.kv_landing_bytes == 0
    finally:
        eng.close()
    eng = DecodeEngine(arena, 1, True, 256, 64, kv_dtype="bf16")               # ... and with it, the bf16 cache exists at 2 rows
    try:
        assert eng.kv16_small is True and eng.kv_dtype == "bf16"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ weight streams and pair forms
@pytest.fixture(scope="module")
def arenas2048(tiny2048, arena16):
    args, sd = tiny2048
    dev = torch.device("cuda")
    return dict(fp32=LMWeightsArena(args, sd, dev), bf16=arena16, e4m3=LMWeightsArena(args, sd, dev, weight_dtype="e4m3"))


@pytest.mark.parametrize("weights", ["fp32", "bf16", "e4m3"])
def test_kv16_small_is_independent_of_the_weight_stream_and_the_launch_form(tiny2048, arenas2048, monkeypatch, weights):
    """One utterance under CFG on the 2048-wide model, where the 2-row step pairs: the engine whose QKV launch runs inside the FFN2 | QKV
    pair launch and the one whose QKV launch is a single (segment) launch give the same logits at each of 24 steps and the same tokens, bit
    for bit, over fp32, bf16 and e4m3 weights — the landing descriptor is all a writer sees."""
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip("the pair launches need 256 CUs")
    gc.collect()                                                              # engines of earlier tests give their pairing slot back
    args, _ = tiny2048
    for name in ("SSRHIP_ATTN_KV16_SMALL", "SSRHIP_GEMV_W16", "SSRHIP_GEMV_W8", "SSRHIP_GEMV_W16_PAIR", "SSRHIP_GEMV_W8_PAIR"):
        monkeypatch.delenv(name, raising=False)
    arena = arenas2048[weights]
    stream = dict(fp32={}, bf16=dict(stream_w16=True), e4m3=dict(stream_w8=True))[weights]
    pair_kw = dict(fp32={}, bf16=dict(pair_w16=True), e4m3=dict(pair_w8=True))[weights]
    out = {}
    for paired in (True, False):
        kw = dict(stream, **pair_kw) if paired else dict(stream, pair_mode=1)
        eng = DecodeEngine(arena, 1, True, 256, 64, debug_logits=True, kv_dtype="bf16", kv16_small=True, **kw)
        try:
            out[paired] = _trace(eng, args, 1, True, True, True, None, (2, 3))
            assert eng.kv16_launches_per_step == LAYERS and eng.kv16_small is True
            assert eng.pairing is paired, eng.pairing_why
            if weights == "bf16":
                assert eng.w16_pair_launches_per_step == (2 * LAYERS if paired else 0) and eng.w16_launches_per_step == (2 if paired else 4 * LAYERS + 2)
            if weights == "e4m3":
                assert eng.w8_pair_launches_per_step == (2 * LAYERS if paired else 0) and eng.w8_launches_per_step == (2 if paired else 4 * LAYERS + 2)
            eng.check_pairs()
        finally:
            eng.close()
        del eng
        gc.collect()
    (lg_p, tok_p, allocs_p), (lg_s, tok_s, _) = out[True], out[False]
    assert torch.isfinite(lg_p).all() and allocs_p == 0
    for s in range(STEPS):
        assert torch.equal(lg_p[s], lg_s[s]), (weights, s, float((lg_p[s] - lg_s[s]).abs().max()))
    assert torch.equal(tok_p, tok_s)


# ------------------------------------------------------------------------------------------ queues and the public surface
def _queue_utts(n):
    g = torch.Generator().manual_seed(14)
    utts = []
    for i in range(n):
        Lt, T = int(torch.randint(6, 15, (1,), generator=g)), int(torch.randint(5, 40, (1,), generator=g))
        utts.append(dict(x=torch.randint(0, 30, (1, Lt), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g), mask_interval=torch.LongTensor([[[T, T]]])))
    return utts


def _model(cfg):
    args, sd = HS.model_cpu(cfg)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


QUEUE_KW = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)


@pytest.mark.parametrize("group", [1, 2])
def test_run_queue_with_refill_under_kv16_small(monkeypatch, group):
    """5 utterances through `group` slots x CFG (2 and 4 rows): blocking admission and two-phase admission give the same results, and both
    equal the same engine decoding the utterances in fixed groups without refill — every prefill path rounds, every attention widens"""
    monkeypatch.setenv("SSRHIP_ATTN_KV16_SMALL", "1")
    m = _model("d128")
    m.set_kv_dtype("bf16")
    utts = _queue_utts(5)
    res = {}
    for two_phase in ("0", "1"):
        monkeypatch.setenv("SSRHIP_ADMIT_TWO_PHASE", two_phase)
        res[two_phase] = m.inference_batch(utts, seed=40, group=group, **QUEUE_KW)
        eng = next(iter(m._engines.values()))
        assert eng.kv16_small is True and eng.kv_dtype == "bf16" and eng.B == 2 * group
        assert eng.n_admitted == 5 and eng.n_refills == 5 - group
        assert eng.kv16_launches_per_step == m.args.num_decoder_layers
    monkeypatch.delenv("SSRHIP_ADMIT_TWO_PHASE")
    fixed = m.inference_batch(utts, seed=40, group=group, refill=False, **QUEUE_KW)
    assert next(iter(m._engines.values())).kv16_small is True
    for i in range(5):
        for other in (res["1"], fixed):
            assert torch.equal(res["0"][i][0], other[i][0]) and torch.equal(res["0"][i][1], other[i][1]) and res["0"][i][2] == other[i][2], (group, i)
    for e in m._engines.values():
        e.close()


def test_public_surface(monkeypatch):
    """`inference` and `inference_stream` under the switch and set_kv_dtype("bf16") run a bf16 engine and return what the oracle with
    bf16-valued K / V returns; with the switch unset the engine is the fp32 one; flipping the switch rebuilds the engine."""
    monkeypatch.delenv("SSRHIP_ATTN_KV16_SMALL", raising=False)
    cfg = "d128"
    args, sd = HS.model_cpu(cfg)
    m = _model(cfg)
    x, y, unc, mi = _utterance(args, HS.SEEDS[cfg]["cfg"][0])
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=2, aug_text=True)
    Lt = torch.LongTensor([x.shape[1]])
    call = lambda: m.inference(x.cuda(), Lt, x.cuda(), Lt, y.cuda(), y.cuda(), mi.cuda(), uncond_x=unc, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    m.set_kv_dtype("bf16")
    r_off = call()                                                             # the switch is unset: the 2-row path keeps fp32 K / V
    e_off = eng_of()
    assert e_off.kv16_small is False and e_off.kv_dtype == "fp32" and e_off.kv16_launches_per_step == 0
    ref32 = O.inference(O.reference_params(sd), args, x, y, mi, uncond_x=unc, **kw)
    assert np.array_equal(r_off[0].cpu().numpy(), ref32[0].numpy())
    monkeypatch.setenv("SSRHIP_ATTN_KV16_SMALL", "1")
    r_on = call()                                                              # the switch is part of the engine key: a new engine is built
    e_on = eng_of()
    assert e_on is not e_off and len(m._engines) == 1
    assert e_on.kv16_small is True and e_on.kv_dtype == "bf16" and e_on.kv_pool.dtype == torch.bfloat16 and e_on.B == 2
    assert e_on.kv16_launches_per_step == args.num_decoder_layers
    with monkeypatch.context() as mp:
        mp.setattr(O, "F", HK.kv16_functional())
        ref16 = O.inference(O.reference_params(sd), args, x, y, mi, uncond_x=unc, **kw)
    assert np.array_equal(r_on[0].cpu().numpy(), ref16[0].numpy())             # what the rounding oracle predicts, and nothing else
    assert np.array_equal(r_on[1].numpy(), ref16[1].numpy()) and r_on[2] == ref16[2] and r_on[3] == ref16[3]
    stream = m.inference_stream(x.cuda(), Lt, x.cuda(), Lt, y.cuda(), y.cuda(), mi.cuda(), uncond_x=unc, **kw)
    for _ in stream:
        pass
    assert eng_of().kv16_small is True and eng_of().kv16_launches_per_step == args.num_decoder_layers
    assert torch.equal(stream.result[0], r_on[0])
    m.set_kv_dtype("fp32")                                                     # the switch alone does nothing
    assert not m._engines
    r_fp32 = call()
    assert eng_of().kv16_small is False and eng_of().kv_dtype == "fp32" and torch.equal(r_fp32[0], r_off[0])
    m.set_kv_dtype("bf16")
    monkeypatch.delenv("SSRHIP_ATTN_KV16_SMALL")
    r_back = call()
    assert eng_of().kv16_small is False and eng_of().kv_dtype == "fp32" and torch.equal(r_back[0], r_off[0])
    arena = _arena(cfg)[1]
    with pytest.raises(ValueError, match="5..32 rows"):
        DecodeEngine(arena, 1, True, 256, 64, kv_dtype="bf16")
    for e in m._engines.values():
        e.close()
