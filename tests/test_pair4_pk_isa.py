"""CPU (hipcc cross-compiles gfx950 without a GPU): the pair kernels of the 4-row decode step over the packed weight streams
(csrc/gemv_pair4_pk.hip; DESIGN.md Part I.26), read off the ISA:

  * the expected instantiations exist and nothing else: per stream (w16 = packed bf16, w8 = e4m3 codes) pair4_<s>_kernel<4 | 6 | 8> and
    pair4_<s>_merge_kernel<8, EARLY = 2 | 0>, and no name collides with the substrings the older ISA tests find their kernels by;
  * no kernel has scratch, none uses AGPRs, and every one fits a 12-wave workgroup: 3 waves per SIMD = 512 / 3 rounded down to the
    allocation granule of 8 = at most 168 VGPRs;
  * static LDS between 32 KB (x' of four rows is in there) and 48 KB (the merge form adds at most 16 KB of merge weights at launch);
  * the weights arrive only as 16-byte non-temporal loads — bf16: two per (row, 1024-element) unit, 16 + 2 * NUWB in the FFN2 form (8 units
    of A, NUWB of B), 4 + 16 in the merge form (2 units of A, 8 of B); e4m3: one per unit, 8 + NUWB and 2 + 8 — no 1- or 2-byte loads, no MFMA;
  * e4m3 codes are widened in registers by v_cvt_pk_f32_fp8;
  * both roles keep every barrier: 5 per arm in the FFN2 form, 7 in the merge form, as in every other pair kernel;
  * the hand-off is one 8-byte agent-scope store per published value."""
import os
import re

import pytest

import helpers_isa as HI

needs_hipcc = pytest.mark.skipif(not os.path.exists(HI.HIPCC), reason="hipcc not installed")
MAX_VGPRS = 168
STREAMS = ("w16", "w8")
PER_UNIT = {"w16": 2, "w8": 1}            # 16-byte loads per (row, 1024-element) unit and lane
OLDER = ("gemv_pair", "gemv_seg", "w16_seg", "w8_seg", "w16_pair_kernel", "w8_pair_kernel", "pair4_kernelI", "pair4_merge_kernelI")


def _ints(sym):
    return [int(x) for x in re.findall(r"Li(\d+)E", sym)]


def _stream(sym):
    found = [s for s in STREAMS if re.search(rf"\d+pair4_{s}_(merge_)?kernelI", sym)]
    assert len(found) == 1, sym
    return found[0]


@pytest.fixture(scope="module")
def unit():
    asm = HI.compile_unit("gemv_pair4_pk")
    return asm, HI.kernel_meta(asm)


@needs_hipcc
def test_pair4_pk_kernels_are_all_there(unit):
    _, meta = unit
    n = 0
    for s in STREAMS:
        ffn2 = sorted(k for k in meta if re.search(rf"\d+pair4_{s}_kernelI", k))
        merge = sorted(k for k in meta if re.search(rf"\d+pair4_{s}_merge_kernelI", k))
        assert sorted(_ints(k) for k in ffn2) == [[4], [6], [8]], (s, ffn2)
        assert sorted(_ints(k) for k in merge) == [[8, 0], [8, 2]], (s, merge)           # <NUWB, EARLY>: both early forms ship for both streams
        n += len(ffn2) + len(merge)
    assert n == len(meta), sorted(meta)
    for sym in meta:
        for piece in OLDER:                                                            # the older ISA tests find their kernels by these
            assert piece not in sym, (sym, piece)


@needs_hipcc
def test_pair4_pk_kernels_fit_three_waves_per_simd_without_scratch(unit):
    asm, meta = unit
    for sym, (vgpr, scratch, lds) in sorted(meta.items()):
        print(f"{sym}: VGPRs {vgpr}, static LDS {lds}, scratch {scratch}")
        assert scratch == 0, (sym, scratch)
        assert vgpr <= MAX_VGPRS, (sym, vgpr)
        assert 32 * 1024 <= lds <= 48 * 1024, (sym, lds)
    assert set(re.findall(r"\.agpr_count:\s+(\d+)", asm)) == {"0"}


@needs_hipcc
def test_pair4_pk_weight_loads_barriers_and_publish(unit):
    asm, meta = unit
    for sym in meta:
        body = HI.body(asm, sym)
        s, merge, nuwb = _stream(sym), "_merge_kernel" in sym, _ints(sym)[0]
        nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))
        assert len(re.findall(r"global_load_\w+ [^\n]* nt\b", body)) == nt, sym                  # nothing narrower is non-temporal
        assert nt == PER_UNIT[s] * (2 + 8 if merge else 8 + nuwb), (sym, nt)
        assert not re.search(r"global_load_(u|s)?(short|byte)", body), sym                       # no 1- or 2-byte fetches of weights
        assert "v_mfma" not in body, sym
        assert ("v_cvt_pk_f32_fp8" in body) == (s == "w8"), sym                                  # the codes are widened in registers, exactly
        assert len(re.findall(r"^\s+s_barrier", body, re.M)) == (14 if merge else 10), sym       # every barrier in both arms of the role branch
        assert len(re.findall(r"global_store_dwordx2 [^\n]* sc1", body)) == 1, sym               # value and tag travel in one agent-scope store
