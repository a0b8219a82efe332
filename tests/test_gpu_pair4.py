"""GPU: the opt-in pair launches of the 4-row decode step (csrc/gemv_pair4.hip; DESIGN.md Part I.24).

Each phase of a 4-row pair kernel runs the fmaf sequence of the `gemv_seg_kernel<4, ..>` launch it replaces and the edge publishes and
gathers the same fp32 values, so `ssrhip_gemv_pair4` and two `ssrhip_gemv` launches at B = 4 give the SAME BITS. Every comparison here is
`np.array_equal` / `torch.equal` on whole buffers (poisoned pads and the whole KV pool included); no tolerance.

Launch level: B = 4, D = 2048, F = 8192, 2 layers of pool, a shuffled page table. Engine level: helpers_w16's `tiny2048` model (d_model
2048, 2 layers), two utterances under CFG and four without. No test here provokes a give-up or keeps CUs busy."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as HC
import helpers_poison as HP
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import PAIR4_WS_BYTES, DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

from helpers_w16 import LAYERS, PAD, POISON, L, _prompts, tiny2048  # noqa: F401

pytestmark = pytest.mark.gpu

B, D, F = 4, 2048, 8192
H, HD, N_LAYER, MAX_PAGES = 16, 128, 2, 4
STEPS = 12
FORMS = ("pair4", "two")


@pytest.fixture(scope="module", autouse=True)
def _needs_256_cus():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip("the pair launches need 256 CUs")
    gc.collect()                                                 # engines of earlier test modules give their slot back when they are collected


@pytest.fixture(scope="module")
def weights():
    """The matrices of every launch-level case, drawn once and never modified: two alternating FFN2 / out-projection / consumer matrices."""
    g = torch.Generator(device="cuda").manual_seed(24)
    mk = lambda shape, scale: (torch.randn(*shape, generator=g, device="cuda") * scale).contiguous()
    w = dict(ffn2=[mk((D, F), F ** -0.5) for _ in range(2)], out=[mk((D, D), D ** -0.5) for _ in range(2)])
    for N in (4096, 6144, 8192):
        w[N] = [mk((N, D), D ** -0.5) for _ in range(2)]
    w["b2"], w["bn"] = torch.randn(D, generator=g, device="cuda"), torch.randn(8192, generator=g, device="cuda")
    return w


def _buf(i, n):
    return 1 if (i == n - 1 and n % 3 == 1) else i % 3           # ssrhip_pair_buffer


def _padded(rows, n, fill=None):
    """[rows * n + PAD] floats: the rows (poison, or the given values), then the poisoned pad"""
    t = torch.full((rows * n + PAD,), POISON, device="cuda")
    if fill is not None:
        t[:rows * n] = fill.reshape(-1)
    return t


def _launch(lib, form, a, b, wa, wb, ws, i, n):
    """one (a, b) of a chain: the pair launch on its granule buffers, or the two launches it replaces"""
    a.W, b.W = wa.data_ptr(), wb.data_ptr()
    s = _lib.stream_ptr()
    if form == "two":
        for args in (a, b):
            rc = lib.ssrhip_gemv(C.byref(args), s)
            assert rc == 0, (rc, lib.ssrhip_last_error())
    else:
        assert lib.ssrhip_gemv_pair4_applicable(C.byref(a), C.byref(b)) == 1
        rc = lib.ssrhip_gemv_pair4(C.byref(a), C.byref(b), ws.data_ptr(), _buf(i, n), _buf((i + 1) % n, n), s)
        assert rc == 0, (rc, lib.ssrhip_last_error())


def _compare(res, what):
    for k, (got, ref) in enumerate(zip(res["pair4"], res["two"])):
        assert np.isfinite(ref[ref != POISON]).all(), (what, k)
        assert np.array_equal(got, ref), (what, k, float(np.nanmax(np.abs(got - ref))))


def _ffn2_args(weights, h, x, y, N, ny, act, epi):
    a, b = _lib.GemvArgs(), _lib.GemvArgs()
    a.bias, a.x, a.y = weights["b2"].data_ptr(), h.data_ptr(), x.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, D, F, 1, F, D
    a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
    b.bias, b.x, b.y = weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()
    b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = B, N, D, 1, D, ny
    b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, act, epi, 1e-5
    return a, b


def _ffn2_chain(L, weights, N, act, epi, n_pairs, reps, seed, x=None):
    """FFN2 + residual | LN + consumer, n_pairs pairs on the cycled granule buffers, replayed `reps` times, both forms;
    x [B, D] (CPU) replaces today's draw of the residual stream the chain starts from"""
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(B, F, generator=g) * 0.7).cuda()
    x0 = (torch.randn(B, D, generator=g) * 1.5 + 0.3).cuda()
    if x is not None:
        x0 = x.cuda()
    table = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES).to(torch.int32).cuda()      # shuffled physical pages
    # one row on the last slot of a page, one on the first slot of a page, two mid-page
    pos = torch.tensor([_lib.PAGE - 1, 2 * _lib.PAGE, 130, 300], dtype=torch.int32, device="cuda")
    qkv = epi == _lib.EPI_QKV_APPEND
    ny = D if qkv else N
    res = {}
    for form in FORMS:
        ws = torch.zeros(PAIR4_WS_BYTES // 4, dtype=torch.int32, device="cuda")
        x, y = _padded(B, D, x0), _padded(B, ny)
        pool = torch.full((B * MAX_PAGES + 1, N_LAYER, 2, H, _lib.PAGE, HD) if qkv else (1,), POISON, device="cuda")
        for rep in range(reps):
            for i in range(n_pairs):
                a, b = _ffn2_args(weights, h, x, y, N, ny, act, epi)
                if qkv:
                    b.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, N_LAYER, H, HD)
                    b.layer, b.kv_pos = i % 2, pos.data_ptr()
                _launch(L, form, a, b, weights["ffn2"][i % 2], weights[N][i % 2], ws, i, n_pairs)
        torch.cuda.synchronize()
        if form == "pair4":
            assert L.ssrhip_gemv_pair4_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * ny:] == POISON).all()), form            # the pads are still poison
        res[form] = (x.cpu().numpy(), y.cpu().numpy(), pool.cpu().numpy())
    return res, qkv


# ------------------------------------------------------------------------------------------ launch level
@pytest.mark.parametrize("name,N,act,epi", [("qkv", 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND), ("head1", 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
                                            ("ffn1", 8192, _lib.ACT_RELU, _lib.EPI_STORE)])
def test_ffn2_form_is_bit_identical_to_the_two_launches(L, weights, name, N, act, epi):
    """7 pairs on the cycled granule buffers (the n % 3 == 1 case), replayed twice (stale tags would show). Residual stream, consumer
    output (pads included) and the whole KV pool."""
    res, qkv = _ffn2_chain(L, weights, N, act, epi, 7, 2, N)
    _compare(res, name)
    if qkv:
        assert int((res["pair4"][2] != POISON).sum()) == 2 * B * N_LAYER * D                             # the appends landed, and nothing else


def test_the_smallest_cycle_of_two_pairs_replayed_three_times(L, weights):
    res, _ = _ffn2_chain(L, weights, 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND, 2, 3, 77)
    _compare(res, "n=2")
    assert int((res["pair4"][2] != POISON).sum()) == 2 * B * N_LAYER * D


@pytest.mark.parametrize("MS,lens", [(8, [1000, 129, 300, 640]), (7, [7 * _lib.PAGE, 1, 2 * _lib.PAGE, 2 * _lib.PAGE + 1])])
def test_merge_form_is_bit_identical_to_the_two_launches(L, weights, MS, lens):
    """split-KV merge + out-projection + residual | LN + FFN1 + ReLU. Rows of <= 2 pages (the two prefetched pages alone), of more (the
    late loads), a length of 1, an odd max_splits; NaN beyond each row's pages; 5 pairs replayed twice. (The form has no early units.)"""
    _merge_both_forms(L, weights, MS, lens)


def _merge_both_forms(L, weights, MS, lens, part_ml=None, dead=float("nan")):
    """the chain of the test above; part_ml [B, H, MS, 2] (CPU, NaN beyond each row's pages) replaces today's draw of the partials;
    dead: the tests/helpers_poison.py fill of the pages beyond each row. Returns the forms' whole output buffers."""
    part_ml_given = part_ml
    g = torch.Generator().manual_seed(MS + lens[0])
    part_o = torch.randn(B, H, MS, HD, generator=g)
    part_ml = torch.stack([torch.randn(B, H, MS, generator=g) * 2, torch.rand(B, H, MS, generator=g) + 0.5], dim=-1).contiguous()
    if part_ml_given is not None:
        part_ml = part_ml_given.clone()
    HP.fill_dead(part_o, part_ml, lens, dead)                    # beyond the row's pages the buffers hold what the kernel must not use
    part_o, part_ml = part_o.cuda(), part_ml.cuda()
    dlen = torch.tensor(lens, dtype=torch.int32, device="cuda")
    x0 = (torch.randn(B, D, generator=g) * 1.5 + 0.3).cuda()
    n_pairs, res = 5, {}
    for form in FORMS:
        ws = torch.zeros(PAIR4_WS_BYTES // 4, dtype=torch.int32, device="cuda")
        x, y = _padded(B, D, x0), _padded(B, F)
        for rep in range(2):
            for i in range(n_pairs):
                a, b = _lib.GemvArgs(), _lib.GemvArgs()
                a.bias, a.y = weights["b2"].data_ptr(), x.data_ptr()
                a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, D, D, 1, D, D
                a.pro, a.act, a.epi = _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
                a.part_o, a.part_ml, a.max_splits, a.row_len = part_o.data_ptr(), part_ml.data_ptr(), MS, dlen.data_ptr()
                a.kv = _lib.KV(0, 0, MS, 1, H, HD)
                b.bias, b.x, b.y = weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()
                b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = B, F, D, 1, D, F
                b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, _lib.ACT_RELU, _lib.EPI_STORE, 1e-5
                _launch(L, form, a, b, weights["out"][i % 2], weights[8192][i % 2], ws, i, n_pairs)
        torch.cuda.synchronize()
        if form == "pair4":
            assert L.ssrhip_gemv_pair4_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * F:] == POISON).all()), form
        res[form] = (x.cpu().numpy(), y.cpu().numpy())
    _compare(res, ("merge", MS, lens))
    return res


@pytest.mark.parametrize("rows", ["offset", "step"])
def test_ffn2_form_is_bit_identical_on_ill_conditioned_rows(L, weights, rows):
    """FFN2 + residual | LN + head-MLP1 + GELU with the residual stream starting at rows with a large common offset / a step between
    the LayerNorm's slices (tests/helpers_conditioning.py): the same bitwise comparison with the two launches"""
    res, _ = _ffn2_chain(L, weights, 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE, 7, 2, 4096, x=HC.ln_rows(B, D, 4096)[rows])
    _compare(res, "head1/" + rows)


@pytest.mark.parametrize("partials", ["wide", "late_peak"])
def test_merge_form_is_bit_identical_on_wide_partials(L, weights, partials):
    """the merge form with partial maxima spread over +-180 / a peak of 150 on each row's last page; 8, 2, 3 and 5 pages"""
    MS, lens = 8, [1000, 129, 300, 640]
    _merge_both_forms(L, weights, MS, lens, part_ml=HC.ml_cases(B, H, MS, lens, 8)[partials])


@pytest.mark.parametrize("case", ["B=2", "N=5120", "SSRHIP_GEMV_PAIR=0", "tiled"])
def test_refusals_launch_nothing(L, weights, monkeypatch, case):
    """returns 1, says it is not applicable, and every output is still poison"""
    rows, N = (2, 4096) if case == "B=2" else (4, 5120 if case == "N=5120" else 4096)
    if case == "SSRHIP_GEMV_PAIR=0":
        monkeypatch.setenv("SSRHIP_GEMV_PAIR", "0")
    h = torch.zeros(rows, F, device="cuda")
    x, y = _padded(rows, D), _padded(rows, N)
    ws = torch.zeros(PAIR4_WS_BYTES // 4, dtype=torch.int32, device="cuda")
    a, b = _lib.GemvArgs(), _lib.GemvArgs()
    a.W, a.bias, a.x, a.y = weights["ffn2"][0].data_ptr(), weights["b2"].data_ptr(), h.data_ptr(), x.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = rows, D, F, 1, F, D
    a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
    b.W, b.bias, b.x, b.y = weights[6144][0].data_ptr(), weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()       # 6144 rows cover N = 5120
    b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = rows, N, D, 1, D, N
    b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE, 1e-5
    if case == "tiled":
        a.x_tiled = 1
    assert L.ssrhip_gemv_pair4_applicable(C.byref(a), C.byref(b)) == 0
    rc = L.ssrhip_gemv_pair4(C.byref(a), C.byref(b), ws.data_ptr(), 0, 1, _lib.stream_ptr())
    assert rc == 1, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all())
    assert int(ws.abs().sum()) == 0                              # not even the granules were touched
    if case == "SSRHIP_GEMV_PAIR=0":                             # the switch is read at every call: the same pair qualifies without it
        monkeypatch.delenv("SSRHIP_GEMV_PAIR")
        assert L.ssrhip_gemv_pair4_applicable(C.byref(a), C.byref(b)) == 1
    if case == "tiled":                                          # the 2-byte KV append is a contract error, and nothing was launched either
        a.x_tiled, b.epi = 0, _lib.EPI_QKV_APPEND16
        assert L.ssrhip_gemv_pair4(C.byref(a), C.byref(b), ws.data_ptr(), 0, 1, _lib.stream_ptr()) < 0
        assert b"EPI_QKV_APPEND16" in L.ssrhip_last_error()
        torch.cuda.synchronize()
        assert bool((x == POISON).all()) and bool((y == POISON).all()) and int(ws.abs().sum()) == 0


def test_the_two_row_entries_keep_refusing_four_rows(L, weights):
    h = torch.zeros(B, F, device="cuda")
    x, y = _padded(B, D), _padded(B, 4096)
    a, b = _ffn2_args(weights, h, x, y, 4096, 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE)
    a.W, b.W = weights["ffn2"][0].data_ptr(), weights[4096][0].data_ptr()
    assert L.ssrhip_gemv_pair4_applicable(C.byref(a), C.byref(b)) == 1 and L.ssrhip_gemv_pair_applicable(C.byref(a), C.byref(b)) == 0
    ws = torch.zeros(PAIR4_WS_BYTES // 4, dtype=torch.int32, device="cuda")
    assert L.ssrhip_gemv_pair(C.byref(a), C.byref(b), ws.data_ptr(), 0, 1, _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all()) and int(ws.abs().sum()) == 0


# ------------------------------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def arena32(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"))


def _steps(eng, args, n_utt, use_cfg, use_graph):
    """STEPS single greedy steps from poisoned KV memory: (post-edit logits per step, generated tokens, sampler states, the whole KV pool)"""
    eng.kv_pool.fill_(POISON)
    rows, cols, knobs = _prompts(args, n_utt, use_cfg, True, (2, 3))
    eng.start(rows, cols, knobs, noise=None)
    logits = []
    for _ in range(STEPS):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        logits.append(eng.dbg_logits.cpu().clone())
    eng.check_pairs()                                            # the give-up flag is clear (raises otherwise)
    return torch.stack(logits), eng.generated[:, :STEPS].cpu().clone(), eng.state_dev.cpu().clone(), eng.kv_pool.cpu().clone()


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("n_utt,use_cfg", [(2, True), (4, False)])
def test_engine_steps_equal_the_unpaired_four_row_engine(tiny2048, arena32, monkeypatch, n_utt, use_cfg, kv16):
    """Two utterances under CFG, four without; fp32 cache and the bf16 cache behind the landing cache: logits at each of 12 steps, tokens,
    sampler states and the whole KV pool of the pair4 engine equal those of the unpaired 4-row engine, eager and as a graph."""
    args, _ = tiny2048
    for name in ("SSRHIP_GEMV_PAIR4", "SSRHIP_GEMV_PAIR", "SSRHIP_ATTN_KV16_SMALL"):
        monkeypatch.delenv(name, raising=False)
    if kv16:
        monkeypatch.setenv("SSRHIP_ATTN_KV16_SMALL", "1")
    kv = dict(kv_dtype="bf16") if kv16 else {}
    mk = lambda **kw: DecodeEngine(arena32, n_utt, use_cfg, 256, 64, debug_logits=True, **kv, **kw)
    engines = dict(pair4=mk(pair4=True), plain=mk())
    try:
        assert engines["pair4"].B == 4 and engines["pair4"].pair4 is True and engines["plain"].pair4 is False
        assert engines["pair4"].kv16_small is kv16 and engines["plain"].kv16_small is kv16
        for use_graph in (False, True):
            out = {name: _steps(e, args, n_utt, use_cfg, use_graph) for name, e in engines.items()}
            ep, en = engines["pair4"], engines["plain"]
            assert ep.pairing is True and "4-row pair launches" in ep.pairing_why, ep.pairing_why
            assert ep.pair4_launches_per_step == 2 * LAYERS
            assert en.pairing is False and en.pair4_launches_per_step == 0
            assert ep.kv16_launches_per_step == (LAYERS if kv16 else 0)
            lg, tok, st, pool = out["pair4"]
            lg2, tok2, st2, pool2 = out["plain"]
            assert torch.isfinite(lg).all()
            for s in range(STEPS):
                assert torch.equal(lg[s], lg2[s]), (use_graph, s, float((lg[s] - lg2[s]).abs().max()))
            assert torch.equal(tok, tok2) and torch.equal(st, st2), use_graph
            assert torch.equal(pool.view(torch.int16 if kv16 else torch.int32), pool2.view(torch.int16 if kv16 else torch.int32)), use_graph
    finally:
        for e in engines.values():
            e.close()


def test_a_pair4_engine_without_the_slot_steps_unpaired_and_equal(tiny2048, arena32, monkeypatch):
    """While a paired 2-row engine lives, a pair4=True engine gets no slot: it reports 0 with the reason and computes the same tokens."""
    args, _ = tiny2048
    for name in ("SSRHIP_GEMV_PAIR4", "SSRHIP_GEMV_PAIR"):
        monkeypatch.delenv(name, raising=False)
    gc.collect()
    two = DecodeEngine(arena32, 1, True, 256, 64)
    engines = [two]
    try:
        two._create_ctx()
        assert two.pairing is True, two.pairing_why
        late, plain = DecodeEngine(arena32, 2, True, 256, 64, debug_logits=True, pair4=True), DecodeEngine(arena32, 2, True, 256, 64, debug_logits=True)
        engines += [late, plain]
        _, tok_late, _, _ = _steps(late, args, 2, True, True)
        _, tok_plain, _, _ = _steps(plain, args, 2, True, True)
        assert late.pair4 is True and late.pairing is False and "another decode engine of this process" in late.pairing_why, late.pairing_why
        assert late.pair4_launches_per_step == 0 and two.pairing is True
        assert torch.equal(tok_late, tok_plain)
    finally:
        for e in engines:
            e.close()


def test_pair4_contract(arena32):
    with pytest.raises(ValueError, match="4-row decode step only"):
        DecodeEngine(arena32, 1, True, 256, 64, pair4=True)                               # 2 rows
    with pytest.raises(ValueError, match="pair_mode=1"):
        DecodeEngine(arena32, 2, True, 256, 64, pair4=True, pair_mode=1)
    eng = DecodeEngine(arena32, 1, True, 256, 64, pair_mode=1)                            # the C side refuses 2 rows too
    try:
        eng._create_ctx()
        assert eng.lib.ssrhip_lm_set_pair4(eng._ctx, 1) < 0 and b"4-row step only" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
def test_inference_batch_of_two_under_the_switch_equals_the_run_without(tiny2048, monkeypatch):
    args, sd = tiny2048
    for name in ("SSRHIP_GEMV_PAIR4", "SSRHIP_GEMV_PAIR"):
        monkeypatch.delenv(name, raising=False)
    gc.collect()
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    g = torch.Generator().manual_seed(31)
    utts = []
    for Lt, T in ((10, 18), (13, 25)):
        utts.append(dict(x=torch.randint(0, args.text_vocab_size, (1, Lt), generator=g), y=torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True, seed=9, group=2)
    eng_of = lambda: next(iter(m._engines.values()))
    try:
        r_off = m.inference_batch(utts, **kw)
        e_off = eng_of()
        assert e_off.B == 4 and e_off.pair4 is False and e_off.pairing is False and e_off.pair4_launches_per_step == 0
        monkeypatch.setenv("SSRHIP_GEMV_PAIR4", "1")
        r_on = m.inference_batch(utts, **kw)                     # the switch is part of the engine key: a new engine is built
        e_on = eng_of()
        assert e_on is not e_off and len(m._engines) == 1
        assert e_on.B == 4 and e_on.pair4 is True and e_on.pairing is True, e_on.pairing_why
        assert e_on.pair4_launches_per_step == 2 * LAYERS
        assert len(r_on) == len(r_off) == 2
        for got, ref in zip(r_on, r_off):
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2]
    finally:
        for e in m._engines.values():
            e.close()
