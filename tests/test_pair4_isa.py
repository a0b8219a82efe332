"""CPU (hipcc cross-compiles gfx950 without a GPU): the pair kernels of the 4-row decode step (csrc/gemv_pair4.hip; DESIGN.md Part I.24),
read off the ISA:

  * the expected instantiations exist and nothing else: pair4_kernel<4 | 6 | 8>, pair4_merge_kernel<8>;
  * no kernel has scratch, none uses AGPRs, and every one fits a 12-wave workgroup: 3 waves per SIMD = 512 / 3 rounded down to the
    allocation granule of 8 = at most 168 VGPRs;
  * LDS: x' of four rows (32 KB) + the parked partial sums, under the 64 KB a workgroup gets without asking (the merge form adds at most
    16 KB of merge weights at launch);
  * the weights arrive only as 16-byte non-temporal loads, four per (row, 1024-float) unit: 32 + 4 * NUWB in the FFN2 form (8 units of A,
    NUWB of B), 8 + 32 in the merge form (2 units of A, 8 of B);
  * both roles keep every barrier: 5 per arm in the FFN2 form, 7 in the merge form, as in the 2-row kernels;
  * the hand-off is one 8-byte agent-scope store per published value."""
import os
import re

import pytest

import helpers_isa as HI

needs_hipcc = pytest.mark.skipif(not os.path.exists(HI.HIPCC), reason="hipcc not installed")
MAX_VGPRS = 168


def _ints(sym):
    return [int(x) for x in re.findall(r"Li(\d+)E", sym)]


@pytest.fixture(scope="module")
def unit():
    asm = HI.compile_unit("gemv_pair4")
    return asm, HI.kernel_meta(asm)


@needs_hipcc
def test_pair4_kernels_are_all_there(unit):
    _, meta = unit
    ffn2 = sorted(s for s in meta if re.search(r"\d+pair4_kernelI", s))
    merge = sorted(s for s in meta if re.search(r"\d+pair4_merge_kernelI", s))
    assert len(ffn2) + len(merge) == len(meta), sorted(meta)
    assert sorted(_ints(s) for s in ffn2) == [[4], [6], [8]]
    assert sorted(_ints(s) for s in merge) == [[8]]
    for sym in meta:
        assert "gemv_pair" not in sym and "gemv_seg" not in sym, sym        # tests/test_isa_guards.py finds the 2-row fp32 kernels by these


@needs_hipcc
def test_pair4_kernels_fit_three_waves_per_simd_without_scratch(unit):
    asm, meta = unit
    for sym, (vgpr, scratch, lds) in meta.items():
        print(f"{sym}: VGPRs {vgpr}, static LDS {lds}, scratch {scratch}")
        assert scratch == 0, (sym, scratch)
        assert vgpr <= MAX_VGPRS, (sym, vgpr)
        assert 4 * 2048 * 4 <= lds <= 64 * 1024 - 16 * 1024, (sym, lds)     # x' of four rows is in there; room for the merge weights
        body = HI.body(asm, sym)
        assert "scratch_" not in body and "v_accvgpr" not in body, sym


@needs_hipcc
def test_pair4_weight_loads_barriers_and_publish(unit):
    asm, meta = unit
    for sym in meta:
        body = HI.body(asm, sym)
        merge = "pair4_merge_kernel" in sym
        nuwb = _ints(sym)[0]
        nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))
        assert len(re.findall(r"global_load_\w+ [^\n]* nt\b", body)) == nt, sym                  # nothing narrower is non-temporal
        assert nt == (8 + 32 if merge else 32 + 4 * nuwb), (sym, nt)
        assert "v_mfma" not in body, sym
        assert len(re.findall(r"^\s+s_barrier", body, re.M)) == (14 if merge else 10), sym       # every barrier in both arms of the role branch
        assert len(re.findall(r"global_store_dwordx2 [^\n]* sc1", body)) == 1, sym               # value and tag travel in one agent-scope store
