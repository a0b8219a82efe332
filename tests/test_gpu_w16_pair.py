"""GPU: the opt-in pair launches over the bf16 weight stream (csrc/gemv_pair_w16.hip; DESIGN.md Part I.19).

Widening a bf16 weight is a shift or a mask and exact, each phase of a pair kernel runs the fmaf sequence of the `w16` kernel it mirrors,
and the edge publishes and gathers the same fp32 values — so `ssrhip_gemv_pair_w16`, two `ssrhip_gemv_w16` launches and `ssrhip_gemv_pair`
on the rounded masters give the SAME BITS. Every comparison here is `np.array_equal` / `torch.equal` on whole buffers (poisoned pads and
the whole KV pool included); no tolerance.

Launch level: the shapes, chains and merge cases of tests/test_gpu_kernels.py
test_gemv_pair_launch_is_bit_identical_to_the_two_launches. Engine level: helpers_w16's `tiny2048` model, one utterance under CFG.
No test here provokes a give-up or keeps CUs busy."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as HC
import helpers_poison as HP
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import DecodeEngine, to_w16_order
from ssr_speech_amd.models.ssr import SSR_Speech

from helpers_w16 import LAYERS, PAD, POISON, STEPS, L, _same, _trace, _utterance, arena16, tiny2048  # noqa: F401

pytestmark = pytest.mark.gpu

B, D, F = 2, 2048, 8192
H, HD, N_LAYER, MAX_PAGES = 16, 128, 2, 4
WS_BYTES = 3 * 4096 * 8 + 64                                     # include/ssrhip.h SSRHIP_PAIR_WS_BYTES
FORMS = ("pair_w16", "two_w16", "pair_fp32")


@pytest.fixture(scope="module", autouse=True)
def _needs_256_cus():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip("the pair launches need 256 CUs")
    gc.collect()                                                 # engines of earlier test modules give their slot back when they are collected


def _rounded(shape, scale, g):
    """(bf16-rounded fp32 master, its packed copy in SSRHIP_W16_INDEX order)"""
    master = (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16).float().contiguous()
    return master, to_w16_order(master)


@pytest.fixture(scope="module")
def weights():
    """The matrices of every launch-level case, drawn once and never modified: two alternating FFN2 / out-projection / consumer matrices."""
    g = torch.Generator(device="cuda").manual_seed(19)
    w = dict(ffn2=[_rounded((D, F), F ** -0.5, g) for _ in range(2)], out=[_rounded((D, D), D ** -0.5, g) for _ in range(2)])
    for N in (4096, 6144, 8192):
        w[N] = [_rounded((N, D), D ** -0.5, g) for _ in range(2)]
    w["b2"], w["bn"] = torch.randn(D, generator=g, device="cuda"), torch.randn(8192, generator=g, device="cuda")
    return w


def _buf(i, n):
    return 1 if (i == n - 1 and n % 3 == 1) else i % 3           # ssrhip_pair_buffer


def _padded(rows, n, fill=None, g=None):
    """[rows * n + PAD] floats: the rows (poison, or random), then the poisoned pad"""
    t = torch.full((rows * n + PAD,), POISON, device="cuda")
    if fill is not None:
        t[:rows * n] = fill.reshape(-1)
    return t


def _launch(lib, form, a, b, wa, wb, ws, i, n):
    """one (a, b) of a chain in the given form; wa / wb = (master, packed)"""
    a.W, b.W = wa[0].data_ptr(), wb[0].data_ptr()
    s = _lib.stream_ptr()
    if form == "two_w16":
        for args, w in ((a, wa), (b, wb)):
            rc = lib.ssrhip_gemv_w16(C.byref(args), w[1].data_ptr(), s)
            assert rc == 0, (rc, lib.ssrhip_last_error())
    elif form == "pair_fp32":
        rc = lib.ssrhip_gemv_pair(C.byref(a), C.byref(b), ws.data_ptr(), _buf(i, n), _buf((i + 1) % n, n), s)
        assert rc == 0, (rc, lib.ssrhip_last_error())
    else:
        assert lib.ssrhip_gemv_pair_w16_applicable(C.byref(a), C.byref(b)) == 1
        rc = lib.ssrhip_gemv_pair_w16(C.byref(a), C.byref(b), wa[1].data_ptr(), wb[1].data_ptr(), ws.data_ptr(), _buf(i, n), _buf((i + 1) % n, n), s)
        assert rc == 0, (rc, lib.ssrhip_last_error())


def _compare(res, what):
    want = res["two_w16"]
    for k, t in enumerate(want):
        assert np.isfinite(t[t != POISON]).all(), (what, k)
    for form in ("pair_w16", "pair_fp32"):
        for k, (got, ref) in enumerate(zip(res[form], want)):
            assert np.array_equal(got, ref), (what, form, k, float(np.nanmax(np.abs(got - ref))))


# ------------------------------------------------------------------------------------------ launch level
@pytest.mark.parametrize("name,N,act,epi", [("qkv", 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND), ("head1", 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
                                            ("ffn1", 8192, _lib.ACT_RELU, _lib.EPI_STORE)])
def test_ffn2_form_is_bit_identical_three_ways(L, weights, name, N, act, epi):
    """FFN2 + residual | LN + consumer: 7 pairs on the cycled granule buffers, replayed twice (stale tags would show). Residual stream,
    consumer output (pads included) and the whole KV pool: pair_w16 == two w16 launches == the fp32 pair on the masters."""
    _ffn2_three_ways(L, weights, name, N, act, epi)


def _ffn2_three_ways(L, weights, name, N, act, epi, x=None):
    """the chain of the test above; x [B, D] (CPU) replaces today's draw of the residual stream the chain starts from"""
    g = torch.Generator().manual_seed(N)
    h = (torch.randn(B, F, generator=g) * 0.7).cuda()
    x0 = (torch.randn(B, D, generator=g) * 1.5 + 0.3).cuda()
    if x is not None:
        x0 = x.cuda()
    table = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES).to(torch.int32).cuda()      # shuffled physical pages
    pos = torch.tensor([130, 300], dtype=torch.int32, device="cuda")
    qkv = epi == _lib.EPI_QKV_APPEND
    ny = D if qkv else N
    n_pairs, res = 7, {}
    for form in FORMS:
        ws = torch.zeros(WS_BYTES // 4, dtype=torch.int32, device="cuda")
        x, y = _padded(B, D, x0), _padded(B, ny)
        pool = torch.full((B * MAX_PAGES + 1, N_LAYER, 2, H, _lib.PAGE, HD) if qkv else (1,), POISON, device="cuda")
        for rep in range(2):
            for i in range(n_pairs):
                a, b = _lib.GemvArgs(), _lib.GemvArgs()
                a.bias, a.x, a.y = weights["b2"].data_ptr(), h.data_ptr(), x.data_ptr()
                a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, D, F, 1, F, D
                a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
                b.bias, b.x, b.y = weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()
                b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = B, N, D, 1, D, ny
                b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, act, epi, 1e-5
                if qkv:
                    b.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, N_LAYER, H, HD)
                    b.layer, b.kv_pos = i % 2, pos.data_ptr()
                _launch(L, form, a, b, weights["ffn2"][i % 2], weights[N][i % 2], ws, i, n_pairs)
        torch.cuda.synchronize()
        if form != "two_w16":
            assert L.ssrhip_gemv_pair_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * ny:] == POISON).all()), form            # the pads are still poison
        res[form] = (x.cpu().numpy(), y.cpu().numpy(), pool.cpu().numpy())
    _compare(res, name)
    if qkv:
        assert int((res["two_w16"][2] != POISON).sum()) == 2 * B * N_LAYER * D                          # the appends landed, and nothing else


@pytest.mark.parametrize("early", [None, "0"])
@pytest.mark.parametrize("MS,lens", [(8, [1000, 129]), (8, [300, 640]), (7, [7 * _lib.PAGE, 1])])
def test_merge_form_is_bit_identical_three_ways(L, weights, monkeypatch, MS, lens, early):
    """split-KV merge + out-projection + residual | LN + FFN1 + ReLU: contexts of 8 / 2 pages (beyond the 6 prefetched ones / short),
    3 / 5 pages, an odd max_splits; NaN beyond each row's pages; 5 pairs replayed twice; with B's early units and without."""
    _merge_three_ways(L, weights, monkeypatch, MS, lens, early)


def _merge_three_ways(L, weights, monkeypatch, MS, lens, early, part_ml=None, dead=float("nan")):
    """the chain of the test above; part_ml [B, H, MS, 2] (CPU, NaN beyond each row's pages) replaces today's draw of the partials;
    dead: the tests/helpers_poison.py fill of the pages beyond each row. Returns the forms' whole output buffers."""
    part_ml_given = part_ml
    if early is None:
        monkeypatch.delenv("SSRHIP_GEMV_PAIR_EARLY", raising=False)
    else:
        monkeypatch.setenv("SSRHIP_GEMV_PAIR_EARLY", early)
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
        ws = torch.zeros(WS_BYTES // 4, dtype=torch.int32, device="cuda")
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
        if form != "two_w16":
            assert L.ssrhip_gemv_pair_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * F:] == POISON).all()), form
        res[form] = (x.cpu().numpy(), y.cpu().numpy())
    _compare(res, ("merge", MS, lens, early))
    return res


@pytest.mark.parametrize("rows", ["offset", "step"])
def test_ffn2_form_is_bit_identical_on_ill_conditioned_rows(L, weights, rows):
    """FFN2 + residual | LN + head-MLP1 + GELU with the residual stream starting at rows with a large common offset / a step between
    the LayerNorm's slices (tests/helpers_conditioning.py): the same three-way bitwise comparison"""
    _ffn2_three_ways(L, weights, "head1/" + rows, 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE, x=HC.ln_rows(B, D, 4096)[rows])


@pytest.mark.parametrize("partials", ["wide", "late_peak"])
def test_merge_form_is_bit_identical_on_wide_partials(L, weights, monkeypatch, partials):
    """the merge form with partial maxima spread over +-180 / a peak of 150 on each row's last page, 8 and 2 pages"""
    MS, lens = 8, [1000, 129]
    _merge_three_ways(L, weights, monkeypatch, MS, lens, None, part_ml=HC.ml_cases(B, H, MS, lens, 8)[partials])


@pytest.mark.parametrize("case", ["B=4", "N=5120", "SSRHIP_GEMV_PAIR=0"])
def test_refusals_launch_nothing(L, weights, monkeypatch, case):
    """returns 1, says it is not applicable, and every output is still poison"""
    rows, N = (4, 4096) if case == "B=4" else (2, 5120 if case == "N=5120" else 4096)
    if case == "SSRHIP_GEMV_PAIR=0":
        monkeypatch.setenv("SSRHIP_GEMV_PAIR", "0")
    h = torch.zeros(rows, F, device="cuda")
    x, y = _padded(rows, D), _padded(rows, N)
    ws = torch.zeros(WS_BYTES // 4, dtype=torch.int32, device="cuda")
    a, b = _lib.GemvArgs(), _lib.GemvArgs()
    a.W, a.bias, a.x, a.y = weights["ffn2"][0][0].data_ptr(), weights["b2"].data_ptr(), h.data_ptr(), x.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = rows, D, F, 1, F, D
    a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
    b.W, b.bias, b.x, b.y = weights[6144][0][0].data_ptr(), weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()       # 6144 rows cover N = 5120
    b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = rows, N, D, 1, D, N
    b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE, 1e-5
    assert L.ssrhip_gemv_pair_w16_applicable(C.byref(a), C.byref(b)) == 0
    rc = L.ssrhip_gemv_pair_w16(C.byref(a), C.byref(b), weights["ffn2"][0][1].data_ptr(), weights[6144][0][1].data_ptr(), ws.data_ptr(), 0, 1, _lib.stream_ptr())
    assert rc == 1, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all())
    assert int(ws.abs().sum()) == 0                              # not even the granules were touched
    if case == "SSRHIP_GEMV_PAIR=0":                             # the switch is read at every call: the same pair qualifies without it
        monkeypatch.delenv("SSRHIP_GEMV_PAIR")
        assert L.ssrhip_gemv_pair_w16_applicable(C.byref(a), C.byref(b)) == 1


# ------------------------------------------------------------------------------------------ engine level
def test_engine_steps_equal_the_unpaired_stream_and_the_masters(tiny2048, arena16, monkeypatch):
    """One utterance under CFG: an engine that pairs its bf16 stream, one that streams w16 unpaired and a masters engine with pair_mode 1 —
    the same post-edit logits at each of 24 single steps and the same tokens, greedy and sampled, eager and as a graph. The pairing engine
    ran 2 * layers bf16 pair launches and 2 single w16 launches per step, its give-up flag stayed clear and its steps allocated nothing.
    A second pair_w16 engine built while the first lives does not get the slot, steps unpaired, says why, and gives equal tokens."""
    args, _ = tiny2048
    monkeypatch.delenv("SSRHIP_GEMV_W16_PAIR", raising=False)    # the default is off: only pair_w16=True pairs
    mk = lambda **kw: DecodeEngine(arena16, 1, True, 256, 64, debug_logits=True, **kw)
    engines = dict(pair=mk(stream_w16=True, pair_w16=True), w16=mk(stream_w16=True), masters=mk(stream_w16=False, pair_mode=1))
    noise = torch.empty(1, 64, args.n_codebooks, arena16.card).exponential_(1, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        assert engines["pair"].pair_w16 is True and engines["w16"].pair_w16 is False and engines["masters"].pair_w16 is False
        for greedy in (True, False):
            for use_graph in (False, True):
                out = {name: _trace(e, args, 1, True, greedy, use_graph, None if greedy else noise, (2, 3)) for name, e in engines.items()}
                ep = engines["pair"]
                assert ep.pairing is True and "bf16 pair launches" in ep.pairing_why, ep.pairing_why
                assert ep.w16_pair_launches_per_step == 2 * LAYERS and ep.w16_launches_per_step == 2
                ep.check_pairs()                                 # the give-up flag is clear (raises otherwise)
                assert engines["w16"].pairing is False and engines["w16"].w16_pair_launches_per_step == 0
                assert engines["w16"].w16_launches_per_step == 4 * LAYERS + 2
                assert engines["masters"].pairing is False and engines["masters"].w16_launches_per_step == 0
                lg, tok, allocs = out["pair"]
                assert torch.isfinite(lg).all() and allocs == 0, allocs
                for name in ("w16", "masters"):
                    lg2, tok2, _ = out[name]
                    for s in range(STEPS):
                        assert torch.equal(lg[s], lg2[s]), (name, greedy, use_graph, s, float((lg[s] - lg2[s]).abs().max()))
                    assert torch.equal(tok, tok2), (name, greedy, use_graph)
        # the slot is taken: a second engine of the same kind steps unpaired and computes the same
        second = mk(stream_w16=True, pair_w16=True)
        engines["second"] = second
        _, tok_first, _ = _trace(engines["pair"], args, 1, True, True, True, None, (2, 3))
        _, tok_second, _ = _trace(second, args, 1, True, True, True, None, (2, 3))
        assert second.pair_w16 is True and second.pairing is False and "another decode engine of this process" in second.pairing_why, second.pairing_why
        assert second.w16_pair_launches_per_step == 0 and second.w16_launches_per_step == 4 * LAYERS + 2
        assert engines["pair"].pairing is True
        assert torch.equal(tok_first, tok_second)
    finally:
        for e in engines.values():
            e.close()


def test_pair_w16_contract(arena16):
    with pytest.raises(ValueError, match="2-row decode step only"):
        DecodeEngine(arena16, 2, True, 256, 64, stream_w16=True, pair_w16=True)          # 4 rows
    with pytest.raises(ValueError, match="stream_w16"):
        DecodeEngine(arena16, 1, True, 256, 64, stream_w16=False, pair_w16=True)
    with pytest.raises(ValueError, match="pair_mode=1"):
        DecodeEngine(arena16, 1, True, 256, 64, stream_w16=True, pair_w16=True, pair_mode=1)
    eng = DecodeEngine(arena16, 2, True, 256, 64, stream_w16=True)                       # the C side refuses 4 rows too
    try:
        eng._create_ctx()
        assert eng.lib.ssrhip_lm_set_w16_pair(eng._ctx, 1) < 0 and b"2-row step only" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
def test_a_bf16_model_pairs_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    monkeypatch.delenv("SSRHIP_GEMV_W16", raising=False)
    monkeypatch.delenv("SSRHIP_GEMV_W16_PAIR", raising=False)
    gc.collect()
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    m.set_weight_dtype("bf16")
    x, y, unc, mi = _utterance(args, 21)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    call = lambda: m.inference(x.cuda(), torch.LongTensor([x.shape[1]]), x.cuda(), torch.LongTensor([x.shape[1]]), y.cuda(), y.cuda(), mi.cuda(),
                               uncond_x=unc, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    r_off = call()
    e_off = eng_of()
    assert e_off.stream_w16 is True and e_off.pair_w16 is False and e_off.pairing is False and e_off.w16_pair_launches_per_step == 0
    monkeypatch.setenv("SSRHIP_GEMV_W16_PAIR", "1")
    r_on = call()                                                # the switch is part of the engine key: a new engine is built
    e_on = eng_of()
    assert e_on is not e_off and len(m._engines) == 1
    assert e_on.pair_w16 is True and e_on.pairing is True, e_on.pairing_why
    assert e_on.w16_pair_launches_per_step == 2 * LAYERS and e_on.w16_launches_per_step == 2
    assert _same(r_on, r_off)
    monkeypatch.delenv("SSRHIP_GEMV_W16_PAIR")
    assert _same(call(), r_off) and eng_of().pairing is False
