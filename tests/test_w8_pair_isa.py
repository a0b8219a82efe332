"""CPU (hipcc cross-compiles gfx950 without a GPU): the pair kernels over packed e4m3 codes (csrc/gemv_pair_w8.hip), read off the ISA
beside their fp32 counterparts of csrc/gemv.hip compiled with the same flags:

  * exactly the five instantiations the launcher uses;
  * no kernel spills or uses AGPRs, and none takes more VGPRs or more static LDS than the fp32 kernel it mirrors (the ring holds a quarter
    of the bytes; the scales held across the A phase fit beside it);
  * the weights arrive only as 16-byte non-temporal loads (`global_load_dwordx4 ... nt`), exactly ONE per (row, 1024-element) unit:
    8 + NUWB in the FFN2 form (8 units of A, NUWB of B), 2 + 8 in the merge form (2 units of A, 8 of B) — a quarter of the fp32 kernel's;
  * widened by v_cvt_pk_f32_fp8 into fp32 FMAs: no MFMA and no v_dot2;
  * both roles keep every barrier: 5 per arm in the FFN2 form, 7 in the merge form, as in the fp32 kernels.
"""
import re

import pytest

from test_w16_pair_isa import _compile, _ints, needs_hipcc


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_w8_pair")
    return _compile("gemv_pair_w8", d), _compile("gemv", d)


def _counterpart(sym, fp32):
    """the fp32 kernel of the same template arguments: w8_pair_kernel<N> -> gemv_pair_kernel<N>, w8_pair_merge_kernel<..> -> gemv_pair_merge_kernel<..>"""
    base = "gemv_pair_merge_kernel" if "w8_pair_merge_kernel" in sym else "gemv_pair_kernel"
    hits = [s for s in fp32 if re.search(r"\d+" + base + "I", s) and _ints(s) == _ints(sym)]
    assert len(hits) == 1, (sym, hits)
    return fp32[hits[0]]


@needs_hipcc
def test_w8_pair_kernels_are_all_there(units):
    w8, _ = units
    ffn2 = sorted(s for s in w8 if re.search(r"\d+w8_pair_kernelI", s))
    merge = sorted(s for s in w8 if re.search(r"\d+w8_pair_merge_kernelI", s))
    assert len(ffn2) + len(merge) == len(w8), sorted(w8)
    assert sorted(_ints(s) for s in ffn2) == [[4], [6], [8]]
    assert sorted(_ints(s) for s in merge) == [[8, 0, 3], [8, 2, 3]]         # <NUWB, EARLY, PF>: the shipped form posts 3 units behind (1b)
    for sym in w8:
        assert "gemv_pair" not in sym and "gemv_seg" not in sym, sym        # tests/test_isa_guards.py finds the fp32 kernels by these


@needs_hipcc
def test_w8_pair_kernels_take_no_more_than_their_fp32_counterparts(units):
    w8, fp32 = units
    for sym, k in w8.items():
        ref = _counterpart(sym, fp32)
        print(f"{sym}: VGPRs {k['vgpr']} (fp32 {ref['vgpr']}), static LDS {k['lds']} (fp32 {ref['lds']}), scratch {k['scratch']}")
        assert k["scratch"] == 0, (sym, k["scratch"])
        assert k["agpr"] == 0, (sym, k["agpr"])
        assert k["vgpr"] <= ref["vgpr"], (sym, k["vgpr"], ref["vgpr"])
        assert k["lds"] <= ref["lds"], (sym, k["lds"], ref["lds"])


@needs_hipcc
def test_w8_pair_weights_arrive_as_one_16_byte_non_temporal_load_per_unit(units):
    w8, fp32 = units
    for sym, k in w8.items():
        body = k["body"]
        nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))
        assert len(re.findall(r"global_load_\w+ [^\n]* nt\b", body)) == nt, sym                # nothing narrower is non-temporal
        assert not re.search(r"global_load_(u|s)?(short|byte)", body), sym                       # no 1- or 2-byte fetches of weights
        assert "v_cvt_pk_f32_fp8" in body, sym                                                   # the codes are widened in registers, exactly
        assert "v_dot2" not in body and "v_mfma" not in body, sym                                # fp32 FMAs on widened weights; x is never rounded
        merge = "w8_pair_merge_kernel" in sym
        nuwb = _ints(sym)[0]
        assert nt == (2 + 8 if merge else 8 + nuwb), (sym, nt)
        # a quarter of the loads of the fp32 kernel, which reads four 16-byte pieces per unit
        assert 4 * nt == len(re.findall(r"global_load_dwordx4 [^\n]* nt", _counterpart(sym, fp32)["body"])), sym
        # every barrier in both arms of the role branch
        assert len(re.findall(r"^\s+s_barrier", body, re.M)) == (14 if merge else 10), sym
