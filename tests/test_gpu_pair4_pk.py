"""GPU: the opt-in pair launches of the 4-row decode step over the packed weight streams (csrc/gemv_pair4_pk.hip; DESIGN.md Part I.26).

bf16 -> fp32 and e4m3 -> fp32 are exact, a multiplication by a row's 2^e commutes with every fp32 rounding (nothing here is subnormal or
overflows), each phase of a pair kernel runs the fmaf / wave_sum sequence of the packed single launch it replaces (e4m3: with the scale
applied where the partial sum is parked), and the edge publishes and gathers the same fp32 values. So `ssrhip_gemv_pair4_w16` /
`ssrhip_gemv_pair4_w8`, two `ssrhip_gemv_w16` / `ssrhip_gemv_w8` launches at B = 4 and `ssrhip_gemv_pair4` on the equivalent fp32 masters
give the SAME BITS. Every comparison here is `np.array_equal` / `torch.equal` on whole buffers (poisoned pads and the whole KV pool
included); no tolerance.

Launch level: B = 4, D = 2048, F = 8192 (the kernels' fixed shapes), weights from helpers_w16.rounded_weights / helpers_w8.quantized_weights,
2 layers of pool, a shuffled page table. One more e4m3 case gives every row another scale than its neighbours' (tests/test_gpu_w8_pair.py's
`quantised`), so that a kernel applying another row's scale fails. Engine level: helpers_w16's `tiny2048` model on arenas of both dtypes,
two utterances under CFG and four without. No test here provokes a give-up or keeps CUs busy."""
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

from helpers_w16 import LAYERS, PAD, POISON, L, _prompts, arena16, rounded_weights, tiny2048  # noqa: F401
from helpers_w8 import quantized_weights
from test_gpu_w8_pair import quantised

pytestmark = pytest.mark.gpu

B, D, F = 4, 2048, 8192
H, HD, N_LAYER, MAX_PAGES = 16, 128, 2, 4
STEPS = 12
STREAMS = ("w16", "w8")
FORMS = ("pk", "two", "fp32")                                    # the pair launch over the packed stream, the two packed launches, ssrhip_gemv_pair4 on the masters
FMT = {"w16": "bf16", "w8": "e4m3"}


@pytest.fixture(scope="module", autouse=True)
def _needs_256_cus():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip("the pair launches need 256 CUs")
    gc.collect()                                                 # engines of earlier test modules give their slot back when they are collected


def _matrix(stream, name, N, K, seed):
    """(fp32 master [N][K], packed copy, scales or None) of one matrix in the stream's format"""
    if stream == "w16":
        master, packed, _ = rounded_weights(name, 1, N, K, seed, "w16")
        return master[0].contiguous(), packed[0].contiguous(), None
    master, packed, scale, _ = quantized_weights(name, 1, N, K, seed)
    return master[0].contiguous(), packed[0].contiguous(), scale[0].contiguous()


_WEIGHTS = {}


def _weights(stream):
    """The matrices of every launch-level case of a stream, built once and never modified: two alternating FFN2 / out-projection / consumer
    matrices. Key "w8s": e4m3 with row-dependent scales."""
    if stream not in _WEIGHTS:
        g = torch.Generator(device="cuda").manual_seed(26)
        if stream == "w8s":
            mk = lambda name, N, K, i: quantised((N, K), K ** -0.5, g)
        else:
            mk = lambda name, N, K, i: _matrix(stream, f"p4pk.{name}{i}.", N, K, 260 + 7 * i + N // 1024)
        w = dict(ffn2=[mk("ffn2", D, F, i) for i in range(2)], out=[mk("out", D, D, i) for i in range(2)])
        for N in (4096, 6144, 8192):
            w[N] = [mk("b", N, D, i) for i in range(2)]
        w["b2"], w["bn"] = torch.randn(D, generator=g, device="cuda"), torch.randn(8192, generator=g, device="cuda")
        _WEIGHTS[stream] = w
    return _WEIGHTS[stream]


def _buf(i, n):
    return 1 if (i == n - 1 and n % 3 == 1) else i % 3           # ssrhip_pair_buffer


def _padded(rows, n, fill=None):
    """[rows * n + PAD] floats: the rows (poison, or the given values), then the poisoned pad"""
    t = torch.full((rows * n + PAD,), POISON, device="cuda")
    if fill is not None:
        t[:rows * n] = fill.reshape(-1)
    return t


def _pk_call(lib, stream, a, b, wa, wb, ws, buf, nxt):
    s = _lib.stream_ptr()
    if stream == "w16":
        return lib.ssrhip_gemv_pair4_w16(C.byref(a), C.byref(b), wa[1].data_ptr(), wb[1].data_ptr(), ws.data_ptr(), buf, nxt, s)
    return lib.ssrhip_gemv_pair4_w8(C.byref(a), C.byref(b), wa[1].data_ptr(), wa[2].data_ptr(), wb[1].data_ptr(), wb[2].data_ptr(), ws.data_ptr(), buf, nxt, s)


def _pk_applicable(lib, stream, a, b):
    return getattr(lib, f"ssrhip_gemv_pair4_{stream}_applicable")(C.byref(a), C.byref(b))


def _launch(lib, stream, form, a, b, wa, wb, ws, i, n):
    """one (a, b) of a chain in the given form; wa / wb = (master, packed, scales or None)"""
    a.W, b.W = wa[0].data_ptr(), wb[0].data_ptr()
    s = _lib.stream_ptr()
    if form == "two":
        for args, w in ((a, wa), (b, wb)):
            if stream == "w16":
                rc = lib.ssrhip_gemv_w16(C.byref(args), w[1].data_ptr(), s)
            else:
                rc = lib.ssrhip_gemv_w8(C.byref(args), w[1].data_ptr(), w[2].data_ptr(), s)
            assert rc == 0, (rc, lib.ssrhip_last_error())
    elif form == "fp32":
        rc = lib.ssrhip_gemv_pair4(C.byref(a), C.byref(b), ws.data_ptr(), _buf(i, n), _buf((i + 1) % n, n), s)
        assert rc == 0, (rc, lib.ssrhip_last_error())
    else:
        assert _pk_applicable(lib, stream, a, b) == 1
        rc = _pk_call(lib, stream, a, b, wa, wb, ws, _buf(i, n), _buf((i + 1) % n, n))
        assert rc == 0, (rc, lib.ssrhip_last_error())


def _compare(res, what):
    want = res["two"]
    for k, t in enumerate(want):
        assert np.isfinite(t[t != POISON]).all(), (what, k)
    for form in ("pk", "fp32"):
        for k, (got, ref) in enumerate(zip(res[form], want)):
            assert np.array_equal(got, ref), (what, form, k, float(np.nanmax(np.abs(got - ref))))


def _ffn2_args(weights, rows, h, x, y, N, ny, act, epi):
    a, b = _lib.GemvArgs(), _lib.GemvArgs()
    a.bias, a.x, a.y = weights["b2"].data_ptr(), h.data_ptr(), x.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = rows, D, F, 1, F, D
    a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
    b.bias, b.x, b.y = weights["bn"].data_ptr(), x.data_ptr(), y.data_ptr()
    b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = rows, N, D, 1, D, ny
    b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, act, epi, 1e-5
    return a, b


def _ffn2_chain(lib, stream, N, act, epi, n_pairs, reps, seed, x=None, wkey=None):
    """FFN2 + residual | LN + consumer, n_pairs pairs on the cycled granule buffers, replayed `reps` times, all three forms;
    x [B, D] (CPU) replaces today's draw of the residual stream the chain starts from"""
    weights = _weights(wkey or stream)
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
                a, b = _ffn2_args(weights, B, h, x, y, N, ny, act, epi)
                if qkv:
                    b.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, N_LAYER, H, HD)
                    b.layer, b.kv_pos = i % 2, pos.data_ptr()
                _launch(lib, stream, form, a, b, weights["ffn2"][i % 2], weights[N][i % 2], ws, i, n_pairs)
        torch.cuda.synchronize()
        if form != "two":
            assert lib.ssrhip_gemv_pair4_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * ny:] == POISON).all()), form            # the pads are still poison
        res[form] = (x.cpu().numpy(), y.cpu().numpy(), pool.cpu().numpy())
    return res, qkv


# ------------------------------------------------------------------------------------------ launch level
@pytest.mark.parametrize("name,N,act,epi", [("qkv", 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND), ("head1", 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
                                            ("ffn1", 8192, _lib.ACT_RELU, _lib.EPI_STORE)])
@pytest.mark.parametrize("stream", STREAMS)
def test_ffn2_form_is_bit_identical_three_ways(L, stream, name, N, act, epi):
    """7 pairs on the cycled granule buffers (the n % 3 == 1 case), replayed twice (stale tags would show). Residual stream, consumer
    output (pads included) and the whole KV pool: the packed pair == two packed launches == the fp32 4-row pair on the masters."""
    res, qkv = _ffn2_chain(L, stream, N, act, epi, 7, 2, N)
    _compare(res, (stream, name))
    if qkv:
        assert int((res["pk"][2] != POISON).sum()) == 2 * B * N_LAYER * D                                # the appends landed, and nothing else


@pytest.mark.parametrize("stream", STREAMS)
def test_the_smallest_cycle_of_two_pairs_replayed_three_times(L, stream):
    res, _ = _ffn2_chain(L, stream, 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND, 2, 3, 77)
    _compare(res, (stream, "n=2"))
    assert int((res["pk"][2] != POISON).sum()) == 2 * B * N_LAYER * D


def _merge_three_ways(lib, stream, monkeypatch, MS, lens, early, part_ml=None, wkey=None, dead=float("nan")):
    """split-KV merge + out-projection + residual | LN + FFN1 + ReLU, 5 pairs replayed twice, all three forms; part_ml [B, H, MS, 2] (CPU,
    NaN beyond each row's pages) replaces today's draw of the partials;
    dead: the tests/helpers_poison.py fill of the pages beyond each row. Returns the forms' whole output buffers."""
    weights = _weights(wkey or stream)
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
                _launch(lib, stream, form, a, b, weights["out"][i % 2], weights[8192][i % 2], ws, i, n_pairs)
        torch.cuda.synchronize()
        if form != "two":
            assert lib.ssrhip_gemv_pair4_status(ws.data_ptr(), _lib.stream_ptr()) == 0
        assert bool((x[B * D:] == POISON).all()) and bool((y[B * F:] == POISON).all()), form
        res[form] = (x.cpu().numpy(), y.cpu().numpy())
    _compare(res, (stream, "merge", MS, lens, early))
    return res


@pytest.mark.parametrize("early", [None, "0"])
@pytest.mark.parametrize("MS,lens", [(8, [1000, 129, 300, 640]), (7, [7 * _lib.PAGE, 1, 2 * _lib.PAGE, 2 * _lib.PAGE + 1])])
@pytest.mark.parametrize("stream", STREAMS)
def test_merge_form_is_bit_identical_three_ways(L, monkeypatch, stream, MS, lens, early):
    """Rows of 8, 2, 3, 5 and of 7, 1, 2, 3 pages (the two prefetched pages alone, and the late loads), a length of 1, an odd max_splits;
    NaN beyond each row's pages; with B's early units (SSRHIP_GEMV_PAIR_EARLY unset) and without (=0): both forms ship for both streams."""
    _merge_three_ways(L, stream, monkeypatch, MS, lens, early)


def test_e4m3_rows_with_different_scales(L, monkeypatch):
    """Both forms once more over e4m3 matrices whose neighbouring rows (and rows 8 apart) carry different scales: a kernel that applies
    another row's scale fails here instead of passing by coincidence."""
    res, _ = _ffn2_chain(L, "w8", 6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND, 7, 2, 61, wkey="w8s")
    _compare(res, "w8s/qkv")
    _merge_three_ways(L, "w8", monkeypatch, 8, [1000, 129, 300, 640], None, wkey="w8s")


@pytest.mark.parametrize("rows", ["offset", "step"])
@pytest.mark.parametrize("stream", STREAMS)
def test_ffn2_form_is_bit_identical_on_ill_conditioned_rows(L, stream, rows):
    """FFN2 + residual | LN + head-MLP1 + GELU with the residual stream starting at rows with a large common offset / a step between
    the LayerNorm's slices (tests/helpers_conditioning.py): the same three-way bitwise comparison"""
    res, _ = _ffn2_chain(L, stream, 4096, _lib.ACT_GELU_ERF, _lib.EPI_STORE, 7, 2, 4096, x=HC.ln_rows(B, D, 4096)[rows])
    _compare(res, (stream, "head1/" + rows))


@pytest.mark.parametrize("partials", ["wide", "late_peak"])
@pytest.mark.parametrize("stream", STREAMS)
def test_merge_form_is_bit_identical_on_wide_partials(L, monkeypatch, stream, partials):
    """the merge form with partial maxima spread over +-180 / a peak of 150 on each row's last page; 8, 2, 3 and 5 pages"""
    MS, lens = 8, [1000, 129, 300, 640]
    _merge_three_ways(L, stream, monkeypatch, MS, lens, None, part_ml=HC.ml_cases(B, H, MS, lens, 8)[partials])


@pytest.mark.parametrize("case", ["B=2", "N=5120", "SSRHIP_GEMV_PAIR=0", "SSRHIP_GEMV_SEG=0", "tiled"])
@pytest.mark.parametrize("stream", STREAMS)
def test_refusals_launch_nothing(L, monkeypatch, stream, case):
    """returns 1, says it is not applicable, every output is still poison and the workspace still zero; the 2-row packed entry and
    ssrhip_gemv_pair4_applicable answer for these descriptors what they answered before"""
    weights = _weights(stream)
    rows, N = (2, 4096) if case == "B=2" else (4, 5120 if case == "N=5120" else 4096)
    switch = case.split("=")[0] if case.startswith("SSRHIP") else None
    if switch:
        monkeypatch.setenv(switch, "0")
    h = torch.zeros(rows, F, device="cuda")
    x, y = _padded(rows, D), _padded(rows, N)
    ws = torch.zeros(PAIR4_WS_BYTES // 4, dtype=torch.int32, device="cuda")
    wa, wb = weights["ffn2"][0], weights[6144][0]                # 6144 rows cover N = 5120
    a, b = _ffn2_args(weights, rows, h, x, y, N, N, _lib.ACT_GELU_ERF, _lib.EPI_STORE)
    a.W, b.W = wa[0].data_ptr(), wb[0].data_ptr()
    if case == "tiled":
        a.x_tiled = 1
    two_row = getattr(L, f"ssrhip_gemv_pair_{stream}_applicable")
    assert _pk_applicable(L, stream, a, b) == 0
    rc = _pk_call(L, stream, a, b, wa, wb, ws, 0, 1)
    assert rc == 1, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all())
    assert int(ws.abs().sum()) == 0                              # not even the granules were touched
    # the older questions on the same descriptors: the fp32 4-row form does not read SSRHIP_GEMV_SEG, the 2-row packed form takes 2 rows only
    assert L.ssrhip_gemv_pair4_applicable(C.byref(a), C.byref(b)) == (1 if case == "SSRHIP_GEMV_SEG=0" else 0)
    assert two_row(C.byref(a), C.byref(b)) == (1 if case == "B=2" else 0)
    if switch:                                                   # the switches are read at every call: the same pair qualifies without them
        monkeypatch.delenv(switch)
        assert _pk_applicable(L, stream, a, b) == 1 and two_row(C.byref(a), C.byref(b)) == 0
    if case == "tiled":                                          # the 2-byte KV append is a contract error, and nothing was launched either
        a.x_tiled, b.epi = 0, _lib.EPI_QKV_APPEND16
        assert _pk_call(L, stream, a, b, wa, wb, ws, 0, 1) < 0
        assert b"EPI_QKV_APPEND16" in L.ssrhip_last_error()
        torch.cuda.synchronize()
        assert bool((x == POISON).all()) and bool((y == POISON).all()) and int(ws.abs().sum()) == 0


# ------------------------------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def arena8(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="e4m3")


@pytest.fixture(scope="module")
def arena32(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"))


@pytest.fixture
def arena_of(arena16, arena8):
    return {"w16": arena16, "w8": arena8}


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


def _clear_switches(monkeypatch):
    for name in ("SSRHIP_GEMV_PAIR4_PK", "SSRHIP_GEMV_PAIR4", "SSRHIP_GEMV_PAIR", "SSRHIP_GEMV_SEG", "SSRHIP_GEMV_W16", "SSRHIP_GEMV_W8", "SSRHIP_GEMV_W16_PAIR",
                 "SSRHIP_GEMV_W8_PAIR", "SSRHIP_GEMV_PAIR_EARLY", "SSRHIP_ATTN_KV16_SMALL"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("n_utt,use_cfg", [(2, True), (4, False)])
@pytest.mark.parametrize("stream", STREAMS)
def test_engine_steps_equal_the_unpaired_packed_engine(tiny2048, arena_of, monkeypatch, stream, n_utt, use_cfg, kv16):
    """Two utterances under CFG, four without; fp32 cache and the bf16 cache behind the landing cache: logits at each of 12 steps, tokens,
    sampler states and the whole poisoned KV pool of the pair4_pk engine equal those of the unpaired packed 4-row engine, eager and as a
    graph. The paired engine ran 2 * layers pair launches and 2 single packed launches per step."""
    args, _ = tiny2048
    _clear_switches(monkeypatch)
    if kv16:
        monkeypatch.setenv("SSRHIP_ATTN_KV16_SMALL", "1")
    kv = dict(kv_dtype="bf16") if kv16 else {}
    mk = lambda **kw: DecodeEngine(arena_of[stream], n_utt, use_cfg, 256, 64, debug_logits=True, **kv, **kw)
    engines = dict(pk=mk(pair4_pk=True), plain=mk())
    singles = lambda e: getattr(e, stream + "_launches_per_step")
    try:
        ep, en = engines["pk"], engines["plain"]
        assert ep.B == 4 and ep.pair4_pk is True and en.pair4_pk is False
        assert getattr(ep, "stream_" + stream) is True and getattr(en, "stream_" + stream) is True
        assert ep.kv16_small is kv16 and en.kv16_small is kv16
        for use_graph in (False, True):
            out = {name: _steps(e, args, n_utt, use_cfg, use_graph) for name, e in engines.items()}
            assert ep.pairing is True and f"4-row {FMT[stream]} pair launches (ssrhip_gemv_pair4_{stream})" in ep.pairing_why, ep.pairing_why
            assert ep.pair4_pk_launches_per_step == 2 * LAYERS and singles(ep) == 2
            assert ep.pair4_launches_per_step == 0 and ep.w16_pair_launches_per_step == 0 and ep.w8_pair_launches_per_step == 0
            assert en.pairing is False and en.pair4_pk_launches_per_step == 0 and singles(en) == 4 * LAYERS + 2
            assert ep.kv16_launches_per_step == (LAYERS if kv16 else 0)
            lg, tok, st, pool = out["pk"]
            lg2, tok2, st2, pool2 = out["plain"]
            assert torch.isfinite(lg).all()
            for s in range(STEPS):
                assert torch.equal(lg[s], lg2[s]), (use_graph, s, float((lg[s] - lg2[s]).abs().max()))
            assert torch.equal(tok, tok2) and torch.equal(st, st2), use_graph
            assert torch.equal(pool.view(torch.int16 if kv16 else torch.int32), pool2.view(torch.int16 if kv16 else torch.int32)), use_graph
    finally:
        for e in engines.values():
            e.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_a_pair4_pk_engine_without_the_slot_steps_unpaired_and_equal(tiny2048, arena_of, monkeypatch, stream):
    """While a paired 2-row engine lives, a pair4_pk=True engine gets no slot: it reports 0 launches with the reason and computes the same tokens."""
    args, _ = tiny2048
    _clear_switches(monkeypatch)
    gc.collect()
    arena = arena_of[stream]
    two = DecodeEngine(arena, 1, True, 256, 64, **{"pair_" + stream: True})
    engines = [two]
    try:
        two._create_ctx()
        assert two.pairing is True, two.pairing_why
        late, plain = DecodeEngine(arena, 2, True, 256, 64, debug_logits=True, pair4_pk=True), DecodeEngine(arena, 2, True, 256, 64, debug_logits=True)
        engines += [late, plain]
        _, tok_late, _, _ = _steps(late, args, 2, True, True)
        _, tok_plain, _, _ = _steps(plain, args, 2, True, True)
        assert late.pair4_pk is True and late.pairing is False and "another decode engine of this process" in late.pairing_why, late.pairing_why
        assert late.pair4_pk_launches_per_step == 0 and getattr(late, stream + "_launches_per_step") == 4 * LAYERS + 2 and two.pairing is True
        assert torch.equal(tok_late, tok_plain)
    finally:
        for e in engines:
            e.close()


def test_pair4_pk_contract(arena16, arena32, monkeypatch):
    _clear_switches(monkeypatch)
    with pytest.raises(ValueError, match="4-row decode step only"):
        DecodeEngine(arena16, 1, True, 256, 64, pair4_pk=True)                            # 2 rows
    with pytest.raises(ValueError, match="streams packed weights"):
        DecodeEngine(arena32, 2, True, 256, 64, pair4_pk=True)                            # an fp32 arena has no packed stream
    with pytest.raises(ValueError, match="pair_mode=1"):
        DecodeEngine(arena16, 2, True, 256, 64, pair4_pk=True, pair_mode=1)
    why = C.create_string_buffer(256)
    for arena, n_utt, want in ((arena16, 1, b"4-row step only"), (arena32, 2, b"streams no packed weights")):       # the C side refuses the same
        eng = DecodeEngine(arena, n_utt, True, 256, 64, pair_mode=1)
        try:
            eng._create_ctx()
            assert eng.lib.ssrhip_lm_set_pair4_pk(eng._ctx, 1) < 0 and want in eng.lib.ssrhip_last_error()
        finally:
            eng.close()
    eng = DecodeEngine(arena16, 2, True, 256, 64, pair_mode=1)                            # pair_mode 1: accepted, and the engine does not pair
    try:
        eng._create_ctx()
        assert eng.lib.ssrhip_lm_set_pair4_pk(eng._ctx, 1) == 0
        assert eng.lib.ssrhip_lm_pairing(eng._ctx, why, 256) == 0 and b"pair_mode 1" in why.value
        assert eng.lib.ssrhip_lm_pair4_pk_launches(eng._ctx) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
@pytest.mark.parametrize("stream", STREAMS)
def test_inference_batch_of_two_under_the_switch_equals_the_run_without(tiny2048, monkeypatch, stream):
    args, sd = tiny2048
    _clear_switches(monkeypatch)
    gc.collect()
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    m.set_weight_dtype(FMT[stream])
    g = torch.Generator().manual_seed(31)
    utts = []
    for Lt, T in ((10, 18), (13, 25)):
        utts.append(dict(x=torch.randint(0, args.text_vocab_size, (1, Lt), generator=g), y=torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True, seed=9, group=2)
    eng_of = lambda: next(iter(m._engines.values()))
    singles = lambda e: getattr(e, stream + "_launches_per_step")
    try:
        r_off = m.inference_batch(utts, **kw)
        e_off = eng_of()
        assert e_off.B == 4 and e_off.pair4_pk is False and e_off.pairing is False and e_off.pair4_pk_launches_per_step == 0
        assert getattr(e_off, "stream_" + stream) is True and singles(e_off) == 4 * LAYERS + 2                    # the parent's launches
        monkeypatch.setenv("SSRHIP_GEMV_PAIR4_PK", "1")
        r_on = m.inference_batch(utts, **kw)                     # the switch is part of the engine key: a new engine is built
        e_on = eng_of()
        assert e_on is not e_off and len(m._engines) == 1
        assert e_on.B == 4 and e_on.pair4_pk is True and e_on.pairing is True, e_on.pairing_why
        assert e_on.pair4_pk_launches_per_step == 2 * LAYERS and singles(e_on) == 2
        assert len(r_on) == len(r_off) == 2
        for got, ref in zip(r_on, r_off):
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2]
    finally:
        for e in m._engines.values():
            e.close()
