"""GPU: nothing a decode step did not write reaches its results (DESIGN.md Part I.27, "the first decode of an engine").

Consumers: every merge of the split-KV partials — the row-per-wave prologue, the segment prologue (fp32, bf16 and e4m3 streams), the
2- and 4-row pair launches over all three weight formats and the stand-alone merge kernel — with the pages beyond each row's length
filled with every value of helpers_poison.DEAD_FILLS in turn: the whole output buffer keeps its BITS, and the form's own fp64 or
bit-identity check holds under the fills. Live page counts run over 1..max_splits for every form.

Producers: the five attention entries over a paged pool whose dead positions (at and beyond a row's length in its last page, the
pages beyond it, the other layer) differ between two launches — a second random draw, and +-3.0e38 — while the live ones are the
same: the live outputs keep their bits. No fp64 reference here, the tests beside the kernels carry those."""
import ctypes as C
import gc
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as hc
import helpers_kv16 as HK
import helpers_poison as HP
import helpers_w16 as H16
import helpers_w8 as H8
from helpers_w16 import L  # noqa: F401
from ssr_speech_amd import _lib

pytestmark = pytest.mark.gpu

PAGE = _lib.PAGE
PAD, POISON = 64, -777.25
FILLS = HP.DEAD_FILLS
TOL_KERNELS = 3e-5                                                 # rtol = atol of the merge launches in tests/test_gpu_kernels.py


def _rows_that_differ(got, ref, B, N):
    """rows b of the [B, N] block behind the front pad whose bits differ, and whether the pads do"""
    g, r = HP.bits(got), HP.bits(ref)
    body = (g[PAD:PAD + B * N] != r[PAD:PAD + B * N]).view(B, N).any(dim=1)
    pads = bool((g[:PAD] != r[:PAD]).any()) or bool((g[PAD + B * N:] != r[PAD + B * N:]).any())
    return [b for b in range(B) if bool(body[b])], pads


def _gemv_merge(lib, B, N, K, H, hd, MS, lens, part_o, part_ml, dW, dbias, y0):
    """one PRO_ATTN_COMBINE + EPI_RESIDUAL launch of ssrhip_gemv; returns the WHOLE buffer (pad | y [B, N] | pad) on the CPU"""
    buf = torch.cat([torch.full((PAD,), POISON), y0.reshape(-1), torch.full((PAD,), POISON)]).cuda()
    d_po, d_ml, dlen = part_o.cuda(), part_ml.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    a = _lib.GemvArgs()
    a.W, a.bias, a.y, a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = dW.data_ptr(), dbias.data_ptr(), buf.data_ptr() + 4 * PAD, B, N, K, 1, K, N
    a.pro, a.act, a.epi = _lib.PRO_ATTN_COMBINE, 0, _lib.EPI_RESIDUAL
    a.part_o, a.part_ml, a.max_splits, a.row_len = d_po.data_ptr(), d_ml.data_ptr(), MS, dlen.data_ptr()
    a.kv = _lib.KV(0, 0, MS, 1, H, hd)
    _lib.check(lib.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return buf.cpu()


def _gemv_merge_under_every_fill(lib, form, B, K, H, MS):
    """ssrhip_gemv's merge prologue, N = 48, head_dim 128: for every list of helpers_poison.rotations and every fill one launch. The NaN
    launch is held to fp64 within helpers_conditioning.tol(FLOOR_GEMV, the fp32 reference's own error), every other launch to the NaN
    launch's bits, whole buffer. Every miss is collected as (lengths, fill, [(row, live pages)], what) before anything is asserted."""
    N, hd = 48, 128
    g = torch.Generator().manual_seed(B * 10 + MS + K)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    y0 = torch.randn(B, N, generator=g)
    dW, dbias = W.cuda(), bias.cuda()
    lin = lambda xin, dt: y0.to(dt) + F.linear(xin, W.to(dt), bias.to(dt))
    bad, seen = [], set()
    for lens in HP.rotations(B, MS):
        seen |= {HP.n_pages(v) for v in lens}
        live_o = torch.randn(B, H, MS, hd, generator=g)
        live_ml = torch.stack([torch.randn(B, H, MS, generator=g) * 2, torch.rand(B, H, MS, generator=g) + 0.5], dim=-1).contiguous()
        want = lin(hc.merge_ref(live_o, live_ml, lens), torch.float64)
        err_ref = hc.max_err(lin(hc.merge_ref(live_o, live_ml, lens, dtype=torch.float32), torch.float32), want)
        ref = None
        for dead in FILLS:
            part_o, part_ml = HP.fill_dead(live_o.clone(), live_ml.clone(), lens, dead)
            got = _gemv_merge(lib, B, N, K, H, hd, MS, lens, part_o, part_ml, dW, dbias, y0)
            if ref is None:
                ref = got
                assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + B * N:] == POISON).all())
                err_k = hc.max_err(got[PAD:PAD + B * N].view(B, N), want)
                print(f"{form} lens={lens}: max |kernel - fp64| = {err_k:.3e}, fp32 reference {err_ref:.3e}")
                if not err_k <= hc.tol(hc.FLOOR_GEMV, err_ref):
                    bad.append((lens, "nan", err_k, err_ref, "fp64 bound"))
                continue
            rows, pads = _rows_that_differ(got, ref, B, N)
            if rows or pads:
                finite = bool(torch.isfinite(got[PAD:PAD + B * N]).all())
                bad.append((lens, HP.fill_name(dead), [(b, HP.n_pages(lens[b])) for b in rows], "pads differ" if pads else "",
                            "last-bit mismatch" if finite else "NaN output"))
    assert seen == set(range(1, MS + 1)), seen                        # every live page count 1..MS was some row's
    for miss in bad:
        print("MISS", form, f"B={B} MS={MS}", miss)
    assert not bad, (form, B, MS, bad)


# ------------------------------------------------------------------------------------------ ssrhip_gemv's two merge prologues
@pytest.mark.parametrize("MS", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_row_per_wave_merge_ignores_its_dead_pages(L, B, MS):
    """K = 512 (4 heads of 128): not a segment shape, `combine_issue` / `combine_finish` of csrc/gemv.hip merge. Even and odd max_splits,
    and more pages than the 8 (<= 2 rows) / 2 (4 rows) it prefetches."""
    _gemv_merge_under_every_fill(L, "merge_rowwave", B, 512, 4, MS)


@pytest.mark.parametrize("two", [None, "1"])
@pytest.mark.parametrize("MS", [1, 7, 8])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_segment_merge_ignores_its_dead_pages(L, monkeypatch, B, MS, two):
    """K = 2048 (16 heads of 128): `gemv_seg_kernel`'s merge, one and two workgroups per CU (SSRHIP_GEMV_SEG_COMBINE_2, read per call)."""
    if two is None:
        monkeypatch.delenv("SSRHIP_GEMV_SEG_COMBINE_2", raising=False)
    else:
        monkeypatch.setenv("SSRHIP_GEMV_SEG_COMBINE_2", two)
    _gemv_merge_under_every_fill(L, f"merge_seg/two={two}", B, 2048, 16, MS)


# ------------------------------------------------------------------------------------------ the bf16 / e4m3 segment merges
W16 = H16.Stream("w16", "w16.", None, [130, 7, 383, 256], 3, hold_fp32=False)      # the <= 4-row bf16 stream of tests/test_gpu_w16.py


def _stream_lens(B, MS):
    return [[300, 129, 384, 1][:B]] + HP.rotations(B, MS)             # the helper's own list, then every live page count


@pytest.mark.parametrize("B", [1, 2, 4])
def test_bf16_segment_merge_ignores_its_dead_pages(L, B):
    """helpers_w16.check_launch on its merge shape (N = 2048, K = 2048, 3 pages): under every fill the packed launch equals the fp32
    launch, both pass the helper's fp64 check (TOL = 3e-5), and the buffers of all fills are the same bits."""
    for lens in _stream_lens(B, W16.max_pages):
        outs = {dead: H16.check_launch(L, W16, B, 1, 2048, 2048, _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL, lens=lens, dead=dead)
                for dead in FILLS}
        HP.same_bits(outs, ("w16 merge", B, lens))


@pytest.mark.parametrize("B", [1, 2, 4])
def test_e4m3_segment_merge_ignores_its_dead_pages(L, B):
    """helpers_w8.check_launch, the same way."""
    for lens in _stream_lens(B, 3):
        outs = {dead: H8.check_launch(L, B, 1, 2048, 2048, _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL, lens=lens, dead=dead)
                for dead in FILLS}
        HP.same_bits(outs, ("w8 merge", B, lens))


# ------------------------------------------------------------------------------------------ the pair launches' merge halves
@pytest.fixture(scope="module")
def needs_256_cus():
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip("the pair launches need 256 CUs")
    gc.collect()                                                 # engines of earlier test modules give their slot back when they are collected


@pytest.fixture(scope="module")
def pair_mats(needs_256_cus):
    """The matrices of the neighbours' merge chains, built once for this module and never modified."""
    import test_gpu_kernels as TK
    import test_gpu_pair4 as T4
    import test_gpu_w16_pair as T16
    import test_gpu_w8_pair as T8
    return dict(fp32=TK._gemv_pair_merge_mats(8), w16=T16.weights.__wrapped__(), w8=T8.weights.__wrapped__(), pair4=T4.weights.__wrapped__())


def _pair_lens(B, MS):
    """lists of B lengths that give every live page count 1..MS to some row (B = 2: four lists, B = 4: two)"""
    return HP.rotations(B, MS)


def _as_tuple(res):
    """{form: (x, y)} -> one flat tuple of whole buffers in a fixed order"""
    return tuple(t for form in sorted(res) for t in res[form])


@pytest.mark.parametrize("MS", [8, 7])
@pytest.mark.parametrize("fmt", ["fp32", "w16", "w8"])
def test_two_row_pair_merges_ignore_their_dead_pages(L, pair_mats, monkeypatch, fmt, MS):
    """`gemv_pair_merge_kernel` over fp32 weights (the merge half of test_gpu_kernels._gemv_pair_chains: pair == two launches) and over
    the bf16 / e4m3 streams (_merge_three_ways: pair == two packed launches == the fp32 pair): the helpers' own bit-identity checks
    hold under every fill, and residual stream and consumer output (pads included) of every form are the same bits under all fills."""
    import test_gpu_kernels as TK
    import test_gpu_w16_pair as T16
    import test_gpu_w8_pair as T8
    ws = torch.zeros(TK._lib_pair_ws_bytes() // 4, dtype=torch.int32, device="cuda")
    for lens in _pair_lens(2, MS):
        outs = {}
        for dead in FILLS:
            if fmt == "fp32":
                res = TK._gemv_pair_merge_chains(L, ws, MS, lens, dead=dead, mats=pair_mats["fp32"])
            else:
                mod = T16 if fmt == "w16" else T8
                res = mod._merge_three_ways(L, pair_mats[fmt], monkeypatch, MS, lens, None, dead=dead)
            outs[dead] = _as_tuple(res)
        HP.same_bits(outs, ("pair merge", fmt, MS, lens))


@pytest.mark.parametrize("MS", [8, 7])
@pytest.mark.parametrize("fmt", ["fp32", "w16", "w8", "w8s"])
def test_four_row_pair_merges_ignore_their_dead_pages(L, pair_mats, monkeypatch, fmt, MS):
    """`gemv_pair4.hip` (_merge_both_forms) and `gemv_pair4_pk.hip` over bf16 codes, e4m3 codes and e4m3 codes with row-dependent scales
    (_merge_three_ways, both weight keys of the e4m3 stream), the same way."""
    import test_gpu_pair4 as T4
    import test_gpu_pair4_pk as TPK
    for lens in _pair_lens(4, MS):
        outs = {}
        for dead in FILLS:
            if fmt == "fp32":
                res = T4._merge_both_forms(L, pair_mats["pair4"], MS, lens, dead=dead)
            else:
                res = TPK._merge_three_ways(L, "w16" if fmt == "w16" else "w8", monkeypatch, MS, lens, None, wkey=fmt, dead=dead)
            outs[dead] = _as_tuple(res)
        HP.same_bits(outs, ("pair4 merge", fmt, MS, lens))


# ------------------------------------------------------------------------------------------ the stand-alone merge
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_combine_ignores_its_dead_pages(L, hd, tiled):
    """`attn_combine_kernel`, R = 4, H = 3 (a partly dead last wave), 8 pages; row-major and tiled output. The NaN launch within
    helpers_conditioning.tol(FLOOR_ATTN, the fp32 reference's own error) of fp64, every other fill the same bits, pads included."""
    R, H, MS = 4, 3, 8
    D = H * hd
    g = torch.Generator().manual_seed(hd + tiled)
    dummy = torch.zeros(64, device="cuda")
    n_out = (16 if tiled else R) * D
    seen = set()
    for lens in HP.rotations(R, MS):
        seen |= {HP.n_pages(v) for v in lens}
        live_o = torch.randn(R, H, MS, hd, generator=g)
        live_ml = torch.stack([torch.randn(R, H, MS, generator=g) * 2, torch.rand(R, H, MS, generator=g) + 0.5], dim=-1).contiguous()
        want = hc.merge_ref(live_o, live_ml, lens)
        err_ref = hc.max_err(hc.merge_ref(live_o, live_ml, lens, dtype=torch.float32), want)
        dlen = torch.tensor(lens, dtype=torch.int32).cuda()
        outs = {}
        for dead in FILLS:
            part_o, part_ml = HP.fill_dead(live_o.clone(), live_ml.clone(), lens, dead)
            d_po, d_ml = part_o.cuda(), part_ml.cuda()
            buf = torch.full((PAD + n_out + PAD,), POISON, device="cuda")
            a = _lib.AttnArgs()
            a.q, a.q_stride = dummy.data_ptr(), 0
            a.kv = _lib.KV(dummy.data_ptr(), dummy.data_ptr(), MS, 1, H, hd)
            a.layer, a.row_seq, a.row_len, a.R, a.max_splits = 0, 0, dlen.data_ptr(), R, MS
            a.scale, a.part_o, a.part_ml, a.out_tiled = 1.0 / math.sqrt(hd), d_po.data_ptr(), d_ml.data_ptr(), tiled
            _lib.check(L.ssrhip_attn_combine(C.byref(a), buf.data_ptr() + 4 * PAD, _lib.stream_ptr()))
            torch.cuda.synchronize()
            outs[dead] = buf.cpu()
        got = outs[FILLS[0]]
        assert bool((got[:PAD] == POISON).all()) and bool((got[PAD + n_out:] == POISON).all())
        body = got[PAD:PAD + n_out]
        y = H16.from_tiled(body, R, D) if tiled else body.view(R, D)
        err_k = hc.max_err(y, want)
        print(f"attn_combine hd={hd} tiled={tiled} lens={lens}: max |kernel - fp64| = {err_k:.3e}, fp32 reference {err_ref:.3e}")
        assert err_k <= hc.tol(hc.FLOOR_ATTN, err_ref), (lens, err_k, err_ref)
        HP.same_bits(outs, ("attn_combine", hd, tiled, lens))
    assert seen == set(range(1, MS + 1)), seen


# ------------------------------------------------------------------------------------------ the producers' dead keys
KV_H, KV_LAYERS, KV_LAYER, KV_PAGES = 2, 2, 1, 3
KV_LENS = [1, 127, 128, 129, 3 * PAGE]


def _pools(R, hd, lens, seed):
    """(table [R, 3], the three pools [R * 3, 2, 2, H, PAGE, hd]): the same values at every live position (layer KV_LAYER, positions
    below a row's length), at the dead ones a second random draw / +3.0e38 and -3.0e38 in a random pattern / the first draw itself."""
    g = torch.Generator().manual_seed(seed)
    n_pg = R * KV_PAGES
    shape = (n_pg, KV_LAYERS, 2, KV_H, PAGE, hd)
    base = torch.randn(shape, generator=g)
    table = torch.randperm(n_pg, generator=g).to(torch.int32).view(R, KV_PAGES)
    live = torch.zeros(shape, dtype=torch.bool)
    for r, length in enumerate(lens):
        for p in range(HP.n_pages(length)):
            live[table[r, p], KV_LAYER, :, :, :min(PAGE, length - p * PAGE)] = True
    other = torch.randn(shape, generator=g)
    huge = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(3.0e38), torch.tensor(-3.0e38))
    assert 0 < int(live.sum()) < live.numel()
    return table, [torch.where(live, base, dead).contiguous() for dead in (other, huge)]


def _attn_args(d_pool, d_table, d_q, d_len, R, hd):
    a = _lib.AttnArgs()
    a.q, a.q_stride = d_q.data_ptr(), 0
    a.kv = _lib.KV(d_pool.data_ptr(), d_table.data_ptr(), KV_PAGES, KV_LAYERS, KV_H, hd)
    a.layer, a.row_seq, a.row_len, a.R, a.max_splits = KV_LAYER, 0, d_len.data_ptr(), R, KV_PAGES
    a.scale = 1.0 / math.sqrt(hd)
    return a


def _live_partials(part_o, part_ml, lens, hd):
    """the pages below ceil(len / PAGE) of every (row, head), as one flat tensor each"""
    R = len(lens)
    po, pml = part_o.cpu().view(R, KV_H, KV_PAGES, hd), part_ml.cpu().view(R, KV_H, KV_PAGES, 2)
    return (torch.cat([po[r, :, :HP.n_pages(v)].reshape(-1) for r, v in enumerate(lens)]),
            torch.cat([pml[r, :, :HP.n_pages(v)].reshape(-1) for r, v in enumerate(lens)]))


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_attn_decode_ignores_dead_keys(L, R, hd, kv16):
    """`ssrhip_attn_decode` / `ssrhip_attn_decode_kv16` (the row's last position in the landing cache, whose other positions are dead
    too): five launches per fill, the lengths rotated so that every row count meets every length."""
    for rot in range(len(KV_LENS)):
        lens = [KV_LENS[(rot + r) % len(KV_LENS)] for r in range(R)]
        table, pools = _pools(R, hd, lens, 100 * R + hd + rot)
        g = torch.Generator().manual_seed(rot)
        q = torch.randn(R, KV_H * hd, generator=g)
        d_table, d_q, d_len = table.cuda(), q.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
        outs = {}
        for name, pool in zip(("randn", "3.0e38"), pools):
            part_o = torch.full((R * KV_H * KV_PAGES * hd,), POISON, device="cuda")
            part_ml = torch.full((R * KV_H * KV_PAGES * 2,), POISON, device="cuda")
            if kv16:
                land = torch.randn(R, 1, 2, KV_H, PAGE, hd, generator=g) * (1.0 if name == "randn" else 1.0e30)
                pool16 = HK.bf16_bits(pool)
                for r, length in enumerate(lens):
                    page, j = int(table[r, (length - 1) // PAGE]), (length - 1) % PAGE
                    land[r, 0, :, :, KV_LAYER] = pools[0][page, KV_LAYER, :, :, j]       # the fp32 entry the QKV launch left
                    pool16[page, KV_LAYER, :, :, j] = HK.bf16_bits(pool[page, KV_LAYER, :, :, j]) if name == "randn" else 0x7F00
                d_pool, d_land = pool16.cuda(), land.cuda()
            else:
                d_pool = pool.cuda()
            a = _attn_args(d_pool, d_table, d_q, d_len, R, hd)
            a.part_o, a.part_ml = part_o.data_ptr(), part_ml.data_ptr()
            if kv16:
                _lib.check(L.ssrhip_attn_decode_kv16(C.byref(a), d_land.data_ptr(), _lib.stream_ptr()), "ssrhip_attn_decode_kv16")
            else:
                _lib.check(L.ssrhip_attn_decode(C.byref(a), _lib.stream_ptr()), "ssrhip_attn_decode")
            torch.cuda.synchronize()
            outs[name] = _live_partials(part_o, part_ml, lens, hd)
            assert bool(torch.isfinite(outs[name][0]).all()) and not bool((outs[name][1] == POISON).any()), (name, lens)
        HP.same_bits(outs, ("attn_decode", "kv16" if kv16 else "fp32", R, hd, lens))


@pytest.mark.parametrize("kv16", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("R", [5, 16, 17, 32])
def test_attn_rows_ignores_dead_keys(L, R, hd, kv16):
    """`ssrhip_attn_rows` / `ssrhip_attn_rows_kv16` at the row counts of the one- and two-panel steps; whole output buffer, pads included."""
    lens = [KV_LENS[r % len(KV_LENS)] for r in range(R)]
    table, pools = _pools(R, hd, lens, 7 * R + hd)
    q = torch.randn(R, KV_H * hd, generator=torch.Generator().manual_seed(R))
    d_table, d_q, d_len = table.cuda(), q.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    n_out = R * KV_H * hd
    outs = {}
    for name, pool in zip(("randn", "3.0e38"), pools):
        d_pool = (HK.bf16_bits(pool) if kv16 else pool).cuda()
        out = torch.full((PAD + n_out + PAD,), POISON, device="cuda")
        a = _attn_args(d_pool, d_table, d_q, d_len, R, hd)
        entry = L.ssrhip_attn_rows_kv16 if kv16 else L.ssrhip_attn_rows
        _lib.check(entry(C.byref(a), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs[name] = out.cpu()
        assert bool(torch.isfinite(outs[name]).all()) and not bool((outs[name][PAD:PAD + n_out] == POISON).any()), name
    HP.same_bits(outs, ("attn_rows", "kv16" if kv16 else "fp32", R, hd))


@pytest.mark.parametrize("hd", [64, 128])
def test_attn_prefill_ignores_dead_keys(L, hd):
    """`ssrhip_attn_prefill`: five prompts of 1, 127, 128, 129 and 384 positions, causal; whole output buffer, pads included."""
    lens = KV_LENS
    R, n = len(lens), sum(lens)
    table, pools = _pools(R, hd, lens, 900 + hd)
    q = torch.randn(n, KV_H * hd, generator=torch.Generator().manual_seed(hd))
    starts = torch.tensor([sum(lens[:i]) for i in range(R + 1)], dtype=torch.int32).cuda()
    d_table, d_q = table.cuda(), q.cuda()
    n_out = n * KV_H * hd
    outs = {}
    for name, pool in zip(("randn", "3.0e38"), pools):
        d_pool = pool.cuda()
        out = torch.full((PAD + n_out + PAD,), POISON, device="cuda")
        a = _attn_args(d_pool, d_table, d_q, starts, R, hd)
        a.row_len, a.R = 0, n
        _lib.check(L.ssrhip_attn_prefill(C.byref(a), starts.data_ptr(), R, max(lens), out.data_ptr() + 4 * PAD, _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs[name] = out.cpu()
        assert bool(torch.isfinite(outs[name]).all()) and not bool((outs[name][PAD:PAD + n_out] == POISON).any()), name
    HP.same_bits(outs, ("attn_prefill", hd))
