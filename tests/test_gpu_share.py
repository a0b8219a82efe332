"""GPU: prompt sharing among the samples of one utterance (DESIGN.md Part I.15).

Rows with the same text and prompt audio have the same prompt K / V, so their table rows may name the same physical pages, and
`ssrhip_attn_rows_group` reads such a page once for a whole chunk of rows. Sharing moves a row to another workgroup and never reorders
its arithmetic: every launch-level comparison is `torch.equal` against `ssrhip_attn_rows` on the same aliased table (whole poisoned
output buffers, pads included), and the sharing engine is held bit for bit to the unshared engine wherever that one takes the fused walk
(16 heads, >= 12 rows), and to the plain oracle within the 2e-4 of tests/test_gpu_lm.py where it takes the split kernels (d128, 6 rows)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_kv16 as HK
import helpers_share as HS
from helpers_w16 import L  # noqa: F401  (module-scoped fixture)
from helpers_w16 import PAD, POISON, _utterance, from_panels
from oracle import lm as O
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

PAGE = _lib.PAGE
ALL_MEMBERS = (2, 4, 8)                                    # the chunk sizes the kernel is built for (SSRHIP_ATTN_GROUP_MEMBERS)


# ------------------------------------------------------------------------------------------ launch level
def _rows(group, n, n_shared, own, last):
    """n rows of group `group` (None: unshared): n_shared common pages, then own[i % len] pages of their own, the last of them filled up to
    key last[i % len] (1 = the page's first key only, PAGE = up to its last)"""
    return [dict(group=group, n_shared=n_shared, own=own[i % len(own)], last=last[i % len(last)]) for i in range(n)]


def _interleave(*lists):
    out = []
    for i in range(max(len(x) for x in lists)):
        out += [x[i] for x in lists if i < len(x)]
    return out


CASE_NAMES = ["chunk1_ns0", "chunk2_ns1", "chunk2_ns2", "chunkM_ns1", "chunkM_ns2", "chunkM_ns3", "chunkM1_ns1", "chunkM1_ns3", "two_groups",
              "cond_uncond", "no_own_page", "short_member", "pages63", "pages64", "pages65", "r32", "r32_two16", "identity6", "identity16",
              "identity32"]


@functools.lru_cache(maxsize=None)
def _cases(MEMBERS):
    """the rows of every case for a kernel built for chunks of MEMBERS rows"""
    return {
        # chunks of 1, 2, MEMBERS rows, and MEMBERS + 1 rows that split into two chunks; n_shared 0..3; own pages 1..3 (odd and even totals)
        "chunk1_ns0": _rows(None, 5, 0, [1, 2, 3], [1, PAGE, 77]),
        "chunk2_ns1": _rows("a", 2, 1, [1, 2], [1, PAGE]) + _rows(None, 3, 0, [1], [5]),
        "chunk2_ns2": _rows("a", 2, 2, [2, 1], [PAGE, 1]) + _rows(None, 3, 0, [2], [128]),
        "chunkM_ns1": _rows("a", MEMBERS, 1, [1, 2, 3], [1, 64, PAGE, 127]),
        "chunkM_ns2": _rows("a", MEMBERS, 2, [1, 3, 2], [PAGE, 2, 1]),
        "chunkM_ns3": _rows("a", MEMBERS, 3, [2, 1, 3], [33, PAGE, 1]),
        "chunkM1_ns1": _rows("a", MEMBERS + 1, 1, [1, 2], [1, PAGE, 90]),
        "chunkM1_ns3": _rows("a", MEMBERS + 1, 3, [3, 1, 2], [PAGE, 1]),
        # two groups and unshared rows in one launch, members interleaved (conditional rows are rows 0, 2, 4, ...)
        "two_groups": _interleave(_rows("a", 5, 2, [1, 2], [1, 100]), _rows("b", 4, 1, [3, 1], [PAGE, 7]), _rows(None, 4, 0, [1, 2, 3], [64])),
        "cond_uncond": _interleave(_rows("a", 6, 2, [1], [17, 18, 19]), _rows(None, 6, 0, [3], [17, 18, 19])),
        # members of different lengths: a member without a page of its own (its length ends with the shared pages), and one whose length ends
        # INSIDE the pages the head calls shared (the kernel clamps to the whole pages every member has; the table still aliases)
        "no_own_page": _rows("a", 3, 2, [0, 1, 2], [PAGE, 1, 5]),
        "short_member": _rows("a", 2, 2, [1], [9]) + [dict(group="a", n_shared=2, own=0, last=72, cut=1)] + _rows(None, 2, 0, [1], [3]),
        # the page-id registers: 63, 64 and 65 pages in total (a register holds 64 ids)
        "pages63": _rows("a", 3, 61, [2], [1, PAGE, 50]) + _rows(None, 2, 0, [63], [9]),
        "pages64": _rows("a", 3, 62, [2], [1, PAGE, 50]) + _rows(None, 2, 0, [64], [9]),
        "pages65": _rows("a", 3, 63, [2], [1, PAGE, 50]) + _rows("b", 2, 1, [64], [PAGE, 1]) + _rows(None, 1, 0, [65], [9]),
        # R = 32, row-major and tiled; identity arrays (no sharing) at 6, 16 and 32 rows
        "r32": _interleave(_rows("a", 16, 2, [1, 2], [1, PAGE, 31]), _rows(None, 16, 0, [3, 4], [1, PAGE, 31])),
        "r32_two16": _interleave(_rows("a", 16, 3, [1], [40, 41]), _rows("b", 16, 1, [3], [PAGE, 1])),
        "identity6": _rows(None, 6, 0, [1, 2, 3, 4], [1, PAGE, 60]),
        "identity16": _rows(None, 16, 0, [1, 2, 3, 4], [1, PAGE, 60]),
        "identity32": _rows(None, 32, 0, [1, 2, 3, 4], [1, PAGE, 60]),
    }


@functools.lru_cache(maxsize=None)
def _case(name, hd, MEMBERS):
    """The operands of one case, built once and never modified: a shuffled page table in which the rows of a group name the same physical
    pages in their first n_shared entries, the chunk arrays, a pool that is POISON wherever no row may look, and q"""
    spec = _cases(MEMBERS)[name]
    R, Hh = len(spec), (1 if name.startswith("pages") else 2)
    g = torch.Generator().manual_seed(len(name) * 131 + hd + R)
    lens, n_entries = [], []
    for s in spec:
        if s.get("cut"):                                                     # ends inside shared page `cut` (0-based)
            n_entries.append(s["n_shared"])
            lens.append(s["cut"] * PAGE + s["last"])
        else:
            n_entries.append(s["n_shared"] + s["own"])
            lens.append((s["n_shared"] + s["own"] - 1) * PAGE + s["last"] if s["own"] else s["n_shared"] * PAGE)
    max_pages = max(n_entries) + 1
    groups = {}
    for r, s in enumerate(spec):
        if s["group"] is not None:
            groups.setdefault(s["group"], []).append(r)
    n_pages = sum(s["own"] for s in spec) + sum(spec[rows[0]]["n_shared"] for rows in groups.values())
    free = torch.randperm(n_pages, generator=g).tolist()
    table = torch.full((R, max_pages), n_pages, dtype=torch.int32)           # entries past a row's pages: the spare page
    for rows in groups.values():
        for i in range(spec[rows[0]]["n_shared"]):
            table[rows, i] = free.pop()
    for r, s in enumerate(spec):
        for i in range(s["own"]):
            table[r, s["n_shared"] + i] = free.pop()
    assert not free
    chunk_head, n_shared = list(range(R)), [0] * R
    for rows in groups.values():
        for c0 in range(0, len(rows), MEMBERS):
            chunk = rows[c0:c0 + MEMBERS]
            for r in chunk:
                chunk_head[r] = chunk[0]
            n_shared[chunk[0]] = spec[chunk[0]]["n_shared"]
    vals = torch.randn(n_pages + 1, 1, 2, Hh, PAGE, hd, generator=g)
    seen = torch.zeros(n_pages + 1, PAGE, dtype=torch.bool)                   # positions some row attends to
    for r in range(R):
        for p in range((lens[r] + PAGE - 1) // PAGE):
            seen[int(table[r, p]), :min(PAGE, lens[r] - p * PAGE)] = True
    pool = torch.where(seen[:, None, None, None, :, None], vals, torch.tensor(POISON))
    q = torch.randn(R, Hh * hd, generator=g)
    dev = lambda t: t.cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    return dict(R=R, Hh=Hh, max_pages=max_pages, lens=lens, table=table, pool=pool, q=q, chunk_head=chunk_head, n_shared=n_shared,
                d_pool=dev(pool), d_table=dev(table), d_q=dev(q), d_len=i32(lens), d_head=i32(chunk_head), d_ns=i32(n_shared))


def _attn_args(c, hd, out_tiled):
    a = _lib.AttnArgs()
    a.q, a.q_stride = c["d_q"].data_ptr(), 0
    a.kv = _lib.KV(c["d_pool"].data_ptr(), c["d_table"].data_ptr(), c["max_pages"], 1, c["Hh"], hd)
    a.layer, a.row_seq, a.row_len = 0, 0, c["d_len"].data_ptr()
    a.R, a.max_splits, a.scale, a.out_tiled = c["R"], c["max_pages"], 1.0 / math.sqrt(hd), out_tiled
    return a


def _both(L, c, hd, out_tiled):
    """(grouped launch, ungrouped launch) on the same table: the whole poisoned output buffers. The caller has set the chunk size the
    case was cut for (SSRHIP_ATTN_GROUP_MEMBERS is read at every launch)."""
    D = c["Hh"] * hd
    n_out = (16 * ((c["R"] + 15) // 16) if out_tiled else c["R"]) * D
    got, want = torch.full((n_out + PAD,), POISON, device="cuda"), torch.full((n_out + PAD,), POISON, device="cuda")
    a = _attn_args(c, hd, out_tiled)
    _lib.check(L.ssrhip_attn_rows_group(C.byref(a), c["d_head"].data_ptr(), c["d_ns"].data_ptr(), got.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_rows_group")
    _lib.check(L.ssrhip_attn_rows(C.byref(a), want.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_rows")
    torch.cuda.synchronize()
    return got, want, n_out


def _untile(buf, R, D):
    return from_panels(buf[:32 * D], R, D) if R > 16 else buf[:16 * D].view(D // 4, 16, 4)[:, :R].permute(1, 0, 2).reshape(R, D)


@pytest.mark.parametrize("members", ALL_MEMBERS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("name", sorted(CASE_NAMES))
def test_group_launch_equals_attn_rows_on_the_same_aliased_table(L, monkeypatch, name, hd, members):
    c = _case(name, hd, members)
    assert max(c["chunk_head"].count(h) for h in set(c["chunk_head"])) <= members
    monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", str(members))
    assert L.ssrhip_attn_group_members() == members
    for out_tiled in ((0, 1) if c["R"] <= 32 else (0,)):
        got, want, n_out = _both(L, c, hd, out_tiled)
        assert torch.equal(got, want), (out_tiled, float((got - want).abs().max()))   # every row bit for bit, untouched entries and the pad too
        assert torch.equal(got[n_out:], torch.full((PAD,), POISON, device="cuda"))
        D = c["Hh"] * hd
        rows = _untile(got, c["R"], D) if out_tiled else got[:n_out].view(c["R"], D)
        assert torch.isfinite(rows).all() and float(rows.abs().max()) < 100.0  # no poisoned K / V entry was folded in


@pytest.mark.parametrize("MEMBERS", ALL_MEMBERS)
def test_cases_cover_what_they_claim(MEMBERS):
    """(no launch) the case table against the list it was written from"""
    CASES = _cases(MEMBERS)
    assert sorted(CASES) == sorted(CASE_NAMES)
    _case = lambda name, hd: globals()["_case"](name, hd, MEMBERS)
    sizes = set()
    for name in CASES:
        c = _case(name, 64)
        sizes |= {c["chunk_head"].count(h) for h in set(c["chunk_head"])}
    assert {1, 2, MEMBERS} <= sizes
    c = _case("chunkM1_ns1", 64)
    assert sorted(c["chunk_head"].count(h) for h in set(c["chunk_head"])) == [1, MEMBERS]      # MEMBERS + 1 rows: two chunks
    assert {max(_case(n, 64)["n_shared"]) for n in CASES} >= {0, 1, 2, 3}
    assert {(ln + PAGE - 1) // PAGE for n in ("pages63", "pages64", "pages65") for ln in _case(n, 64)["lens"]} >= {63, 64, 65}
    assert {ln % PAGE for n in CASES for ln in _case(n, 64)["lens"]} >= {0, 1}
    heads = _case("two_groups", 64)["chunk_head"]
    groups = [s["group"] for s in CASES["two_groups"]]                         # two groups (each cut into chunks of <= MEMBERS rows) and unshared rows
    assert {g for g in groups if g is not None} == {"a", "b"} and None in groups
    assert all(len({groups[r] for r in range(len(heads)) if heads[r] == h}) == 1 for h in set(heads))     # no chunk mixes groups
    assert len({h for h in heads if heads.count(h) > 1}) >= 2 and any(groups[r] != groups[r + 1] for r in range(len(groups) - 1))
    assert _case("r32", 64)["R"] == 32 and {_case(f"identity{r}", 64)["R"] for r in (6, 16, 32)} == {6, 16, 32}


@pytest.mark.parametrize("members", ALL_MEMBERS)
@pytest.mark.parametrize("hd", [64, 128])
def test_group_launch_against_an_fp64_softmax(L, monkeypatch, hd, members):
    """one case held to a reference of its own: the bound tests/test_gpu_kernels.py holds ssrhip_attn_rows to"""
    c = _case("two_groups", hd, members)
    monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", str(members))
    got, _, n_out = _both(L, c, hd, 0)
    D = c["Hh"] * hd
    ref = torch.zeros(c["R"], D, dtype=torch.float64)
    pool, table = c["pool"].double(), c["table"]
    for r, ln in enumerate(c["lens"]):
        for h in range(c["Hh"]):
            k = torch.cat([pool[int(table[r, p]), 0, 0, h] for p in range((ln + PAGE - 1) // PAGE)])[:ln]
            v = torch.cat([pool[int(table[r, p]), 0, 1, h] for p in range((ln + PAGE - 1) // PAGE)])[:ln]
            w = torch.softmax(k @ c["q"][r, h * hd:(h + 1) * hd].double() / math.sqrt(hd), 0)
            ref[r, h * hd:(h + 1) * hd] = w @ v
    torch.testing.assert_close(got[:n_out].view(c["R"], D).cpu().double(), ref, rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _arena(cfg):
    args, sd = HK.model_cpu(cfg)
    return args, LMWeightsArena(args, {k: v.cuda() for k, v in sd.items()}, torch.device("cuda"))


def _engine(arena, n_utt, share, **kw):
    return DecodeEngine(arena, n_utt, True, 512, 64, debug_logits=True, share_prompt=share, **kw)


def _steps(eng, inputs, use_graph):
    """24 single steps from a fresh start: (prefilled rows, free pages after the start, logits [STEPS][n_utt][K][card], tokens, device
    allocations during the steps)"""
    prefilled = eng.start(*inputs, noise=None)
    torch.cuda.synchronize()
    free0 = eng.pages.n_free
    allocs0 = torch.cuda.memory_stats()["num_device_alloc"]
    logits = []
    for _ in range(HK.STEPS):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        logits.append(eng.dbg_logits.cpu().clone())
    return prefilled, free0, torch.stack(logits), eng.generated[:, :HK.STEPS].cpu().clone(), torch.cuda.memory_stats()["num_device_alloc"] - allocs0


def _check_bookkeeping(eng, args, n, N, own_uncond, prefilled, free0, plain_free0):
    groups = 1 if own_uncond else 2                                           # the conditional rows; the unconditional ones when they are equal
    assert prefilled == ((N + 1) * n if own_uncond else 2 * n), (prefilled, n)
    assert free0 - plain_free0 == groups * (N - 1) * (n // PAGE)              # every follower holds the leader's whole prompt pages
    assert eng.group_launches_per_step == args.num_decoder_layers            # every attention launch was the grouped walk
    assert all(k == n for k in eng._kv0)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("N,n,own_uncond,members", [(8, 128, True, None), (8, 129, True, None), (8, 255, True, None), (8, 256, True, None),
                                                    (8, 257, True, None), (8, 257, False, None), (16, 129, True, None), (16, 257, True, None),
                                                    (16, 256, False, None), (16, 257, True, 4), (16, 257, False, 8), (16, 129, True, 8),
                                                    (8, 256, False, 2)])
def test_sharing_engine_equals_the_unshared_engine_bit_for_bit(monkeypatch, N, n, own_uncond, members, use_graph):
    """d1024: 16 heads and >= 12 rows, so the unshared engine takes the fused walk too — N samples of one utterance whose prompt is n
    positions long (n % 128 in {0, 1, 127}; 1 and 2 shared pages). members: the chunk size in force when the engine is CREATED (None: the
    default); the knob then changes to another value before the first step, and the engine's launches keep the size its chunks were cut
    for (ssrhip_lm_set_group_members)."""
    args, arena = _arena("d1024")
    if members is not None:
        monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", str(members))
    MEMBERS = _lib.lib().ssrhip_attn_group_members()
    assert members in (None, MEMBERS)
    Lt, T = HS.utterance_of_len(args, 3, n)
    inputs = HS.sample_inputs(args, 3, N, Lt, T, own_uncond)
    out = {}
    for share in (False, True):
        if members is not None:
            monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", str(members))
        eng = _engine(arena, N, share)
        if members is not None:                                               # from here on the knob says something else
            monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", "2" if members != 2 else "8")
        try:
            assert eng.share_prompt is share and eng.group_members == (MEMBERS if share else 1)
            out[share] = _steps(eng, inputs, use_graph)
            if share:
                assert eng.lib.ssrhip_lm_group_members(eng._ctx) == MEMBERS
            if share:
                _check_bookkeeping(eng, args, n, N, own_uncond, out[True][0], out[True][1], out[False][1])
                if n // PAGE:
                    assert sorted(len(c) for c in eng._chunks) == sorted([min(MEMBERS, N - i) for i in range(0, N, MEMBERS)] * (1 if own_uncond else 2))
            else:
                assert out[False][0] == 2 * N * n and eng.group_launches_per_step == 0
        finally:
            eng.close()
    (_, _, lg0, tok0, _), (_, _, lg1, tok1, allocs) = out[False], out[True]
    assert torch.isfinite(lg1[torch.isfinite(lg0)]).all() and allocs == 0, allocs
    for s in range(HK.STEPS):
        assert torch.equal(lg1[s], lg0[s]), (s, float((lg1[s] - lg0[s]).nan_to_num(0, 0, 0).abs().max()))
    assert torch.equal(tok1, tok0)
    for u in range(1, N):                                                     # greedy samples of one utterance: all the same tokens
        assert own_uncond or torch.equal(tok1[u], tok1[0])


def _oracle(args, sd, seed, Lt, T):
    x, y, unc, mi = _utterance(args, seed, Lt, T)
    trace = {}
    O.inference(O.reference_params(sd), args, x, y, mi, uncond_x=unc, max_steps=HK.STEPS, trace=trace, **HK.KW)
    return torch.stack(trace["edited_logits"]).numpy(), torch.stack(trace["samples"]).numpy()


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("n", [None, 257], ids=["short", "n257"])
def test_sharing_engine_at_six_rows_matches_the_plain_oracle(monkeypatch, n, use_graph):
    """d128 at 6 rows x 2 heads: the unshared step takes the split kernels there, the sharing step the grouped walk (the rule the bf16
    cache uses). 3 samples with equal unconditional rows: each is the utterance the oracle decodes alone. `short`: the utterance of
    tests/helpers_kv16.py (a prompt inside one page: one prefill, no shared page, the tail copied); n257: two shared pages and a tail."""
    cfg, seed, N = "d128", 2, 3
    args, arena = _arena(cfg)
    if n is None:
        Lt, T = 10, 18
        ref_lg, ref_tok = HK.oracle_trace(monkeypatch, cfg, seed, False)
        n = HS.prompt_len(args, seed, Lt, T)
    else:
        Lt, T = HS.utterance_of_len(args, seed, n)
        ref_lg, ref_tok = _oracle(args, HK.model_cpu(cfg)[1], seed, Lt, T)
    inputs = HS.sample_inputs(args, seed, N, Lt, T, own_uncond=False)
    eng = _engine(arena, N, True)
    try:
        plain_free0 = eng.pages.n_pages - 2 * N * (n // PAGE + 1)
        prefilled, free0, lg, tok, allocs = _steps(eng, inputs, use_graph)
        _check_bookkeeping(eng, args, n, N, False, prefilled, free0, plain_free0)
        assert allocs == 0, allocs
    finally:
        eng.close()
    steps = ref_lg.shape[0]
    assert steps >= 8
    finite = np.isfinite(ref_lg)
    worst = 0.0
    for u in range(N):
        assert np.array_equal(tok[u, :steps].numpy(), ref_tok), (u, tok[u], ref_tok)
        got = lg[:steps, u].numpy()
        assert np.array_equal(np.isfinite(got), finite)
        worst = max(worst, float(np.abs(np.where(finite, got - ref_lg, 0.0)).max()))
    print(f"d128 6 rows n={n} {'graph' if use_graph else 'eager'}: max |logit - plain oracle| over {steps} steps = {worst:.2e}")
    assert worst <= HK.LOGIT_ATOL, worst


def test_setter_refusals_on_real_engines():
    args, arena = _arena("d128")
    with pytest.raises(ValueError, match="5..32 rows"):
        DecodeEngine(arena, 2, True, 512, 64, share_prompt=True)
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(arena, 3, True, 512, 64, share_prompt=True, kv_dtype="bf16")
    with pytest.raises(ValueError, match="256 pages"):
        DecodeEngine(arena, 3, True, 257 * PAGE, 64, share_prompt=True)
    fake = (0x5000, 0x6000)                                                   # refused before anything reads them
    small = DecodeEngine(arena, 2, True, 512, 64)
    kv16 = DecodeEngine(arena, 3, True, 512, 64, kv_dtype="bf16")
    eng = _engine(arena, 3, True)
    try:
        for e in (small, kv16, eng):
            e.start(*HS.sample_inputs(args, 2, e.n_utt), noise=None)           # creates the context; nothing is captured yet
        assert small.lib.ssrhip_lm_set_prompt_groups(small._ctx, *fake) < 0 and b"5..32 rows" in small.lib.ssrhip_last_error()
        assert kv16.lib.ssrhip_lm_set_prompt_groups(kv16._ctx, *fake) < 0 and b"bf16 KV cache" in kv16.lib.ssrhip_last_error()
        assert eng.lib.ssrhip_lm_set_prompt_groups(eng._ctx, fake[0], None) < 0 and b"come together" in eng.lib.ssrhip_last_error()
        assert eng.lib.ssrhip_lm_set_kv16(eng._ctx, 1) < 0 and b"shares prompts" in eng.lib.ssrhip_last_error()
        eng.decode(1, use_graph=True)
        torch.cuda.synchronize()
        assert eng.lib.ssrhip_lm_set_prompt_groups(eng._ctx, None, None) < 0 and b"already captured" in eng.lib.ssrhip_last_error()
        assert eng.lib.ssrhip_lm_set_group_members(eng._ctx, 4) < 0 and b"already captured" in eng.lib.ssrhip_last_error()
        assert eng.lib.ssrhip_lm_group_members(eng._ctx) == eng.group_members
        assert eng.group_launches_per_step == args.num_decoder_layers and small.group_launches_per_step == 0
    finally:
        for e in (small, kv16, eng):
            e.close()


def _jobs(args, N, n, caps):
    Lt, T = HS.utterance_of_len(args, 5, n)
    rows, cols, knobs = HS.sample_inputs(args, 5, N, Lt, T, own_uncond=True)
    return [dict(text_rows=rows[2 * i:2 * i + 2], audio_cols=cols[i], knobs=knobs[i], gen=None, cap=caps[i]) for i in range(N)]


@pytest.mark.parametrize("first_out", [0, 3], ids=["leader", "middle"])
def test_run_queue_releases_a_member_first(first_out):
    """8 samples through 8 slots; one job's cap ends it at the first poll — the chunk's leader (row 0), or a member in the middle — while
    the others go on for two more chunks: the survivors decode what they decode unshared, the released slot's pages that others hold stay,
    and at the end every page is back in the pool"""
    args, arena = _arena("d1024")
    N, n = 8, 257
    caps = [48] * N
    caps[first_out] = 16
    jobs = _jobs(args, N, n, caps)
    res = {}
    for share in (False, True):
        eng = _engine(arena, N, share)
        try:
            res[share] = eng.run_queue(jobs, chunk=16, use_graph=True, sampling=False)
            assert eng.n_admitted == N and eng.n_refills == 0
            assert eng.pages.n_free == eng.pages.n_pages, (eng.pages.n_free, eng.pages.n_pages)
            assert not eng._chunks and eng._chunk_host[0].tolist() == list(range(eng.B)) and not eng._chunk_host[1].any()
            if share:
                assert eng.prefilled_rows == (N + 1) * n and eng.group_launches_per_step == args.num_decoder_layers
        finally:
            eng.close()
    for j in range(N):
        (st0, gen0), (st1, gen1) = res[False][j], res[True][j]
        assert np.array_equal(np.asarray(gen0), np.asarray(gen1)), j
        assert (st0.n_steps, st0.done) == (st1.n_steps, st1.done), j
    assert len(np.asarray(res[True][first_out][1])) <= 16 < max(len(np.asarray(res[True][j][1])) for j in range(N))   # it left first, others went on


def test_release_keeps_the_groups_pages_until_the_last_holder(monkeypatch):
    """host bookkeeping on a live engine (chunks of 4, read when the engine is created; no step is launched): the leader leaves first,
    then a middle member, then everybody"""
    monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", "4")
    args, arena = _arena("d1024")
    N, n = 4, 257
    Lt, T = HS.utterance_of_len(args, 5, n)
    eng = _engine(arena, N, True)
    try:
        eng.start(*HS.sample_inputs(args, 5, N, Lt, T, own_uncond=True), noise=None)
        shared = eng._row_pages[0][:2]
        assert all(eng.pages.holders(p) == N for p in shared) and eng._chunks == [[0, 2, 4, 6]]
        assert eng._chunk_host[0].tolist() == [0, 1, 0, 3, 0, 5, 0, 7] and eng._chunk_host[1].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
        free = eng.pages.n_free
        eng.release_utterance(0)                                              # the leader: its own pages go, the shared ones stay
        assert all(eng.pages.holders(p) == N - 1 for p in shared) and eng.pages.n_free == free + 1 + 3
        assert eng._chunk_host[0].tolist() == [0, 1, 2, 3, 2, 5, 2, 7] and eng._chunk_host[1].tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
        assert torch.equal(eng.chunk_dev.cpu(), torch.from_numpy(eng._chunk_host))
        eng.release_utterance(2)
        assert eng._chunk_host[0].tolist() == [0, 1, 2, 3, 4, 5, 2, 7] and eng._chunk_host[1].tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
        eng.release_utterance(1)
        assert not eng._chunks and eng._chunk_host[0].tolist() == list(range(8)) and not eng._chunk_host[1].any()
        assert all(eng.pages.holders(p) == 1 for p in shared)
        eng.release_utterance(3)
        assert eng.pages.n_free == eng.pages.n_pages
    finally:
        eng.close()


def test_inference_batch_with_sampling():
    """the public switch: 8 sampled samples of one utterance (16 rows at d1024), same results with and without sharing; <= 4 rows run
    unshared without error"""
    args, sd = HK.model_cpu("d1024")
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda:0").eval()
    Lt, T = HS.utterance_of_len(args, 6, 257)
    x, y, _, mi = _utterance(args, 6, Lt, T)
    one = dict(x=x, y=y, mask_interval=mi)
    kw = dict(top_k=20, top_p=0.9, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True, seed=21)
    plain = m.inference_batch([one] * 8, **kw)
    e0 = next(iter(m._engines.values()))
    assert e0.share_prompt is False and e0.group_launches_per_step == 0
    shared = m.inference_batch([one] * 8, share_prompt=True, **kw)
    e1 = next(iter(m._engines.values()))
    assert e1 is not e0 and e1.share_prompt is True and e1.B == 16                 # part of the engine key
    assert e1.group_launches_per_step == args.num_decoder_layers and e1.prefilled_rows == 9 * 257
    assert e1.pages.n_free == e1.pages.n_pages
    for i in range(8):
        assert torch.equal(plain[i][0], shared[i][0]) and torch.equal(plain[i][1], shared[i][1]) and plain[i][2] == shared[i][2] and plain[i][3] == shared[i][3], i
    assert any(not torch.equal(shared[0][0], shared[i][0]) for i in range(1, 8))   # sampled: the samples differ
    two = m.inference_batch([one] * 2, share_prompt=True, **kw)                    # 4 rows: unshared, no error
    e2 = next(iter(m._engines.values()))
    assert e2.B == 4 and e2.share_prompt is False
    assert torch.equal(two[0][0], plain[0][0]) and torch.equal(two[1][0], plain[1][0])
