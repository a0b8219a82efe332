"""CPU: the host side of the e4m3 weight stream of the 5..16-row decode step (DESIGN.md Part I.22) — the packed layout against its index
formula (include/ssrhip.h SSRHIP_WT8_INDEX) element by element, a lane-level model of the addresses both kernel forms of
csrc/gemv_mfma_w8.hip compute against what the fp32 kernels read from the streaming order (SSRHIP_WTILED_INDEX), the switch
(`resolve_wt8_stream`) with its exact messages and its precedence over `stream_wt16`, what the arena builds, and the answers
`ssrhip_gemv_wt8` gives before any launch."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from helpers_w16 import fake_gemv_args
from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import (LMWeightsArena, e4m3_master, from_wt8_order, quantize_e4m3, resolve_wt8_stream, to_wt8_order,
                                   wt8_streamable)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wt8_index(n, k, K):
    """SSRHIP_WT8_INDEX as the header documents it in words: n = 8u + c, k = 128o + 16j + 4ks + e, h = j % 2, g = j / 2"""
    u, c = n // 8, n % 8
    o, j, ks, e = k // 128, (k % 128) // 16, (k % 16) // 4, k % 4
    h, g = j % 2, j // 2
    return ((u * (K // 128) + o) * 2 + h) * 512 + (ks * 8 + c) * 16 + g * 4 + e


def wtiled_index(n, k, K):
    """SSRHIP_WTILED_INDEX (the fp32 streaming order), in floats"""
    return ((n // 8) * (K // 16) + k // 16) * 128 + (((k % 16) // 4) * 8 + n % 8) * 4 + k % 4


def _header_macro(name):
    """the macro's own text from include/ssrhip.h, as a Python expression (C's integer `/` on non-negative operands is `//`)"""
    src = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    m = re.search(r"#define " + name + r"\(n, k, K\) (?:\\\n\s*)?(.*)\n", src)
    assert m, name + " not found in include/ssrhip.h"
    return m.group(1).replace("(size_t)", "").replace("/", "//")


@pytest.mark.parametrize("N,K", [(24, 256), (52, 128), (8, 1920)])
def test_to_wt8_order_is_the_documented_index_element_by_element(N, K):
    g = torch.Generator().manual_seed(N + K)
    codes = torch.randint(1, 0x7f, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)       # nonzero: a padded slot cannot pass for a code
    packed = to_wt8_order(codes)
    U = (N + 7) // 8
    assert packed.dtype == torch.uint8 and packed.shape == (U * 8, K)
    flat = packed.reshape(-1).tolist()
    want = codes.tolist()
    hits = [0] * (U * 8 * K)
    macro = compile(_header_macro("SSRHIP_WT8_INDEX"), "SSRHIP_WT8_INDEX", "eval")
    for n in range(U * 8):
        for k in range(K):
            i = wt8_index(n, k, K)
            assert i == eval(macro, {}, dict(n=n, k=k, K=K)), (n, k)           # the macro says the same
            hits[i] += 1
            assert flat[i] == (want[n][k] if n < N else 0), (n, k)             # the padded rows are code 0
    assert all(h == 1 for h in hits)                                           # a bijection onto the padded buffer
    assert torch.equal(from_wt8_order(packed, N), codes)
    # a group dimension is carried along
    assert torch.equal(to_wt8_order(torch.stack([codes, codes.flip(0)]))[1], to_wt8_order(codes.flip(0)))
    assert torch.equal(from_wt8_order(to_wt8_order(torch.stack([codes, codes.flip(0)])), N)[1], codes.flip(0))


def test_wt8_streamable():
    assert all(wt8_streamable(K) for K in (128, 1024, 1920, 2048, 2176, 4096, 8192))
    assert not any(wt8_streamable(K) for K in (0, 16, 64, 192, 1040, 1088, 2112))


# ------------------------------------------------------------------------------------------ lane-level addressing model
# The device code's own arithmetic (csrc/gemv_mfma_w8.hip wt8_row / wt8_ptr / wt8_off and the loops' `m`, `g`), transcribed: for a lane, a
# tile and a k-step of its wave slice it gives the BYTE address of each of the four codes the lane feeds the MFMA; the inverse of
# SSRHIP_WT8_INDEX turns that into (row, k). The fp32 kernels' arithmetic (csrc/gemv_mfma_tile.h tile_wptr, csrc/gemv_mfma.hip's loads)
# gives the FLOAT address in the streaming-order copy; the inverse of SSRHIP_WTILED_INDEX turns that into (row, k). They must agree.
def _inverse(index, NP, K):
    inv = {}
    for n in range(NP):
        for k in range(K):
            inv[index(n, k, K)] = (n, k)
    assert len(inv) == NP * K
    return inv


def _wt8_row(row_lo, nun, tile, c):
    rows = 16 if 2 * tile + 1 < nun else 8
    return row_lo + tile * 16 + (c & (rows - 1))


def _wt8_ptr(row_lo, nun, tile, c, ks, K):
    rr = _wt8_row(row_lo, nun, tile, c)
    return (rr >> 3) * 8 * K + (ks * 8 + (rr & 7)) * 16


def _wt8_off(obase, m, lasto):
    return (min(obase + (m >> 1), lasto) * 2 + (m & 1)) * 512


def _tile_wptr(row_lo, nun, tile, c, ks, K):
    rows = 16 if 2 * tile + 1 < nun else 8
    rr = row_lo + tile * 16 + (c & (rows - 1))
    return (rr >> 3) * 8 * K + (ks * 8 + (rr & 7)) * 4


def _model(N, K, nun_list, spw, pair):
    """mismatches over every lane, tile, wave slice, load and dword; (checked codes, clamped k-steps seen)"""
    NP = (N + 7) // 8 * 8
    inv8, inv32 = _inverse(wt8_index, NP, K), _inverse(wtiled_index, NP, K)
    steps, lasto = K // 16, K // 128 - 1
    last = steps - 1
    nw = (steps + spw - 1) // spw
    bad = checked = clamped = 0
    row_lo = 0
    for nun in nun_list:                                                       # the units of consecutive workgroups
        ntile = (nun + 1) // 2
        for wave, lane in itertools.product(range(nw), range(64)):
            c, ks = lane & 15, lane >> 4
            tbase = wave * spw
            obase = tbase >> 3
            for tile in range(ntile):
                if pair:
                    wp = _wt8_ptr(row_lo, nun, 0, c, ks, K) + (c >> 3) * 512
                    fp = _tile_wptr(row_lo, nun, 0, c, ks, K) + (c >> 3) * 128
                else:
                    wp, fp = _wt8_ptr(row_lo, nun, tile, c, ks, K), _tile_wptr(row_lo, nun, tile, c, ks, K)
                for t in range(0, spw, 2 if pair else 1):
                    if pair:                                                   # pair i = t / 2: load i / 4 (one octet), dword i % 4
                        i = t // 2
                        addr = wp + min(obase + (i >> 2), lasto) * 1024 + (i & 3) * 4
                        faddr = fp + min(tbase + t, last - 1) * 128
                        kstep = tbase + t + (c >> 3)                           # lanes c >= 8: the other k-step of the pair
                    else:                                                      # load m = 2 (t / 8) + t % 2, dword g = (t / 2) % 4
                        m, g = 2 * (t >> 3) + (t & 1), (t >> 1) & 3
                        addr = wp + _wt8_off(obase, m, lasto) + g * 4
                        faddr = fp + min(tbase + t, last) * 128
                        kstep = tbase + t
                    for e in range(4):
                        n8, k8 = inv8[addr + e]                                # in bounds, or this raises
                        if tbase + t > last:                                   # past the end of K: x is zeroed; the clamped octet is the row's last
                            clamped += 1
                            bad += not (k8 // 128 == lasto and n8 == _wt8_row(row_lo, nun, 0 if pair else tile, c))
                            continue
                        n32, k32 = inv32[faddr + e]
                        checked += 1
                        bad += (n8, k8) != (n32, k32) or k8 != 16 * kstep + 4 * ks + e
        row_lo += nun * 8
    return bad, checked, clamped


@pytest.mark.parametrize("N,K,nun_list,spw,pair,want_clamped", [
    (40, 256, [3, 2], 16, False, False),       # x in registers: 16-row tile + 8-row duplicate tile, then one full tile
    (40, 1920, [3, 2], 16, False, True),       # 120 k-steps: the last wave's slice holds one octet, its second is clamped
    (24, 4096, [3], 32, False, False),         # SPWX = 32
    (24, 2176, [1, 2], 32, False, True),       # the streaming form's slices (spw = 32): 136 k-steps, wave 4 holds one octet, waves 5.. none
    (16, 256, [1, 1], 16, True, False),        # pair form, x in registers
    (16, 1920, [1, 1], 16, True, True),
    (16, 2176, [1, 1], 32, True, True),        # pair form, streaming slices
])
def test_lane_addressing_of_both_forms_meets_the_fp32_streaming_order(N, K, nun_list, spw, pair, want_clamped):
    if spw == 32 and K == 2176:                # gemv_rows_plan's streaming split: 8 waves of ((steps + 7) / 8 rounded up to 16) k-steps
        assert ((K // 16 + 7) // 8 + 15) // 16 * 16 == 32
    bad, checked, clamped = _model(N, K, nun_list, spw, pair)
    print(f"N={N} K={K} units={nun_list} spw={spw} pair={pair}: {checked} codes checked, {clamped} clamped, {bad} mismatches")
    assert checked > 0 and bad == 0
    assert (clamped > 0) is want_clamped


# ------------------------------------------------------------------------------------------ the switch
def test_resolve_wt8_stream_every_case_and_message():
    assert E.WT8_DEFAULT == "0"
    for rows, dtype, req, sw in itertools.product((1, 2, 4, 5, 16, 17, 32), E.WEIGHT_DTYPES, (None, True, False), (None, "0", "1")):
        env = {} if sw is None else {"SSRHIP_GEMVM_W8": sw}
        case = (rows, dtype, req, sw)
        if req is None:
            assert resolve_wt8_stream(rows, dtype, None, env) is (dtype == "e4m3" and 5 <= rows <= 16 and sw == "1"), case
        elif req is False:
            assert resolve_wt8_stream(rows, dtype, False, env) is False, case
        elif rows <= 4:
            with pytest.raises(ValueError) as err:
                resolve_wt8_stream(rows, dtype, True, env)
            assert str(err.value) == f"stream_wt8 is the e4m3 weight stream of the 5..16-row step; an engine of {rows} rows takes stream_w8", case
        elif rows > 16:
            with pytest.raises(ValueError) as err:
                resolve_wt8_stream(rows, dtype, True, env)
            assert str(err.value) == f"stream_wt8: the e4m3 weight stream of the matrix-core step exists for 5..16 rows only (this engine has {rows} rows)", case
        elif dtype != "e4m3":
            with pytest.raises(ValueError) as err:
                resolve_wt8_stream(rows, dtype, True, env)
            assert str(err.value) == "stream_wt8 needs an arena built with weight_dtype='e4m3'", case
        else:
            assert resolve_wt8_stream(rows, dtype, True, env) is True, case
    # only the first character of the switch counts, and no other variable is read
    assert resolve_wt8_stream(8, "e4m3", None, {"SSRHIP_GEMVM_W8": "01"}) is False
    assert resolve_wt8_stream(8, "e4m3", None, {"SSRHIP_GEMVM_W8": "yes"}) is True
    assert resolve_wt8_stream(8, "e4m3", None, {"SSRHIP_GEMVM_W16": "1", "SSRHIP_GEMV_W8": "1"}) is False


@pytest.fixture(scope="module")
def arenas():
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=1, vocab=64)
    sd = W.lm_state_dict(args, seed=3)
    mk = lambda dt: LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype=dt)
    return mk("e4m3"), mk("bf16"), mk("fp32")


class _Stop(Exception):
    pass


def _resolved(monkeypatch, arena, n_utt, use_cfg, env, **kw):
    """(stream_wt8, stream_wt16, stream_wt32) as DecodeEngine.__init__ resolves them; the constructor is stopped before it builds anything"""
    seen = {}

    def stop(self, *a, **k):
        raise _Stop

    monkeypatch.setattr(LMWeightsArena, "ensure_positions", stop)
    for name in ("SSRHIP_GEMVM_W8", "SSRHIP_GEMVM_W16"):
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    eng = E.DecodeEngine.__new__(E.DecodeEngine)
    eng._ctx = None
    try:
        E.DecodeEngine.__init__(eng, arena, n_utt, use_cfg, 256, 64, **kw)
    except _Stop:
        seen = (eng.stream_wt8, eng.stream_wt16, eng.stream_wt32)
    return seen


def test_stream_wt8_takes_precedence_over_an_unasked_stream_wt16(monkeypatch, arenas):
    a8, a16, a32 = arenas
    both = {"SSRHIP_GEMVM_W8": "1", "SSRHIP_GEMVM_W16": "1"}
    assert _resolved(monkeypatch, a8, 8, True, {}) == (False, False, False)                       # nothing set: nothing changes
    assert _resolved(monkeypatch, a8, 8, True, {"SSRHIP_GEMVM_W16": "1"}) == (False, True, False)  # as before this stream existed
    assert _resolved(monkeypatch, a8, 8, True, both) == (True, False, False)                      # the 1-byte stream takes the step
    assert _resolved(monkeypatch, a8, 8, True, {"SSRHIP_GEMVM_W16": "1"}, stream_wt8=True) == (True, False, False)
    assert _resolved(monkeypatch, a8, 8, True, both, stream_wt8=False) == (False, True, False)
    assert _resolved(monkeypatch, a8, 5, False, both, stream_wt16=False) == (True, False, False)
    assert _resolved(monkeypatch, a8, 16, True, both) == (False, False, True)                     # 32 rows: out of scope, stream_wt32 as before
    assert _resolved(monkeypatch, a8, 2, True, both) == (False, False, False)                     # 4 rows
    assert _resolved(monkeypatch, a16, 8, True, both) == (False, True, False)                     # a bf16 arena has no codes
    assert _resolved(monkeypatch, a32, 8, True, both) == (False, False, False)
    with pytest.raises(ValueError, match="an engine takes one"):
        _resolved(monkeypatch, a8, 8, True, {}, stream_wt8=True, stream_wt16=True)
    with pytest.raises(ValueError, match="takes stream_w8"):
        _resolved(monkeypatch, a8, 2, True, {}, stream_wt8=True)
    with pytest.raises(ValueError, match="5..16 rows only"):
        _resolved(monkeypatch, a8, 17, False, {}, stream_wt8=True)
    with pytest.raises(ValueError, match="weight_dtype='e4m3'"):
        _resolved(monkeypatch, a16, 8, True, {}, stream_wt8=True)


# ------------------------------------------------------------------------------------------ the arena
def test_e4m3_arena_builds_the_wt8_copies_once_and_they_round_trip(arenas):
    a8, a16, a32 = arenas
    for other in (a16, a32):
        with pytest.raises(ValueError, match="e4m3"):
            other.ensure_wt8_copies()
    n32, gen0 = a8.nbytes_per_step(), a8.generation
    assert not hasattr(a8, "head1_wt8")
    assert a8.ensure_wt8_copies() is True and a8.ensure_wt8_copies() is False and a8.generation == gen0 + 1
    lay = a8.layers[0]
    saved = 0
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        Wm, sc, P = lay[name + "_w"], lay[name + "_w8s"], lay[name + "_wt8"]
        assert P.dtype == torch.uint8 and P.shape == ((Wm.shape[0] + 7) // 8 * 8, Wm.shape[1]), name
        assert torch.equal(e4m3_master(from_wt8_order(P, Wm.shape[0]), sc), Wm), name                # codes * scale is the master
        saved += 3 * Wm.numel() - 4 * sc.numel()
    assert torch.equal(e4m3_master(from_wt8_order(a8.head1_wt8, a8.head1_w.shape[0]), a8.head1_w8s), a8.head1_w)
    saved += 3 * a8.head1_w.numel() - 4 * a8.head1_w8s.numel()
    assert a8.head2_w.shape[-1] == 32 and a8.head2_wt8 is None                 # K = 32 is no whole octet: streams its fp32 copy
    assert a8.nbytes_per_step() == n32 - saved                                # 1 byte per weight + a scale per row; the count skips the new keys
    w = a8.wt8_struct()
    assert w.head1_w8 == a8.head1_wt8.data_ptr() and w.head1_s == a8.head1_w8s.data_ptr() and not w.head2_w8 and not w.head2_s
    assert w.ffn2_w8[0] == lay["ffn2_wt8"].data_ptr() and w.ffn2_s[0] == lay["ffn2_w8s"].data_ptr()


def test_quantized_rows_survive_the_round_trip_with_distinct_scales():
    raw = torch.randn(52, 256, generator=torch.Generator().manual_seed(4)) * torch.ldexp(torch.ones(52), (5 * torch.arange(52)) % 13 - 9).unsqueeze(1)
    codes, scale = quantize_e4m3(raw)
    assert len(set(scale.tolist())) >= 8
    assert torch.equal(e4m3_master(from_wt8_order(to_wt8_order(codes), 52), scale), e4m3_master(codes, scale))


# ------------------------------------------------------------------------------------------ the C side, before any launch
def test_gemv_wt8_refusals_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_gemv_wt8(None, 0x4000, 0x5000, None) < 0 and b"ssrhip_gemv_wt8: null argument" in L.ssrhip_last_error()
    a = fake_gemv_args(8)
    assert L.ssrhip_gemv_wt8(C.byref(a), None, 0x5000, None) < 0 and b"ssrhip_gemv_wt8: null argument" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_wt8(C.byref(a), 0x4000, None, None) < 0 and b"ssrhip_gemv_wt8: null argument" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_wt8_applicable(None) == 0
    for kw in (dict(B=4), dict(B=17), dict(w_tiled=0), dict(K=1088), dict(K=1040)):
        a = fake_gemv_args(**{"B": 8, **kw})
        assert L.ssrhip_gemv_wt8(C.byref(a), 0x4000, 0x5000, None) == 1, kw   # does not qualify, nothing launched
        assert L.ssrhip_gemv_wt8_applicable(C.byref(a)) == 0, kw
    a = fake_gemv_args(8, K=8192, pro=_lib.PRO_LAYERNORM)                      # what ssrhip_gemv refuses at these rows is refused here too
    assert L.ssrhip_gemv_wt8(C.byref(a), 0x4000, 0x5000, None) < 0 and b"LayerNorm" in L.ssrhip_last_error()
    assert L.ssrhip_lm_wt8_launches(None) == 0
    assert L.ssrhip_lm_set_wt8(None, None) < 0 and b"ssrhip_lm_set_wt8" in L.ssrhip_last_error()
    assert L.ssrhip_version() == 107                                           # additions only; the record is ssrhip_lm_w8


def test_the_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("ssrhip_gemv_wt8", "ssrhip_gemv_wt8_applicable", "ssrhip_lm_set_wt8", "ssrhip_lm_wt8_launches"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in bound, name
    assert "SSRHIP_GEMVM_W8" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
