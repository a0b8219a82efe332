"""CPU (hipcc cross-compiles gfx950 without a GPU): the pair kernels over packed bf16 weights (csrc/gemv_pair_w16.hip), read off the ISA
beside their fp32 counterparts of csrc/gemv.hip compiled with the same flags:

  * no kernel spills, and none takes more VGPRs or more static LDS than the fp32 kernel it mirrors (the ring holds half the bytes);
  * the weights arrive only as 16-byte non-temporal loads (`global_load_dwordx4 ... nt`), exactly two per (row, 1024-element) unit:
    16 + 2 * NUWB in the FFN2 form (8 units of A, NUWB of B), 4 + 16 in the merge form (2 units of A, 8 of B);
  * fp32 FMAs on widened weights: no bf16 MFMA (no MFMA at all) and no v_dot2;
  * both roles keep every barrier: 5 per arm in the FFN2 form, 7 in the merge form, as in the fp32 kernels.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _compile(unit, out_dir):
    """symbol -> dict(vgpr, scratch, lds, body)"""
    out = out_dir / (unit + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, unit + ".hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    asm = open(out).read()
    found = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):     # one metadata entry per kernel
        meta = m.group(0)
        sym = re.search(r"\.name:\s+(\S+)", meta).group(1)
        num = lambda key: int(re.search(key + r":\s+(\d+)", meta).group(1))
        start = asm.index("\n" + sym + ":")
        found[sym] = dict(vgpr=num(r"\.vgpr_count"), agpr=num(r"\.agpr_count"), scratch=num(r"\.private_segment_fixed_size"),
                          lds=num(r"\.group_segment_fixed_size"), body=asm[start:asm.index(".Lfunc_end", start)])
    return found


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_w16_pair")
    return _compile("gemv_pair_w16", d), _compile("gemv", d)


def _ints(sym):
    return [int(x) for x in re.findall(r"Li(\d+)E", sym)]


def _counterpart(sym, fp32):
    """the fp32 kernel of the same template arguments: w16_pair_kernel<N> -> gemv_pair_kernel<N>, w16_pair_merge_kernel<..> -> gemv_pair_merge_kernel<..>"""
    base = "gemv_pair_merge_kernel" if "w16_pair_merge_kernel" in sym else "gemv_pair_kernel"
    hits = [s for s in fp32 if re.search(r"\d+" + base + "I", s) and _ints(s) == _ints(sym)]
    assert len(hits) == 1, (sym, hits)
    return fp32[hits[0]]


@needs_hipcc
def test_w16_pair_kernels_are_all_there(units):
    w16, _ = units
    ffn2 = sorted(s for s in w16 if re.search(r"\d+w16_pair_kernelI", s))
    merge = sorted(s for s in w16 if re.search(r"\d+w16_pair_merge_kernelI", s))
    assert len(ffn2) + len(merge) == len(w16), sorted(w16)
    assert sorted(_ints(s) for s in ffn2) == [[4], [6], [8]]
    assert sorted(_ints(s) for s in merge) == [[8, 0, 3], [8, 2, 3]]        # <NUWB, EARLY, PF>: the shipped form posts 3 units behind (1b)
    for sym in w16:
        assert "gemv_pair" not in sym and "gemv_seg" not in sym, sym        # tests/test_isa_guards.py finds the fp32 kernels by these


@needs_hipcc
def test_w16_pair_kernels_take_no_more_than_their_fp32_counterparts(units):
    w16, fp32 = units
    for sym, k in w16.items():
        ref = _counterpart(sym, fp32)
        print(f"{sym}: VGPRs {k['vgpr']} (fp32 {ref['vgpr']}), static LDS {k['lds']} (fp32 {ref['lds']}), scratch {k['scratch']}")
        assert k["scratch"] == 0, (sym, k["scratch"])
        assert k["agpr"] == 0, (sym, k["agpr"])
        assert k["vgpr"] <= ref["vgpr"], (sym, k["vgpr"], ref["vgpr"])
        assert k["lds"] <= ref["lds"], (sym, k["lds"], ref["lds"])


@needs_hipcc
def test_w16_pair_weights_arrive_as_two_16_byte_non_temporal_loads_per_unit(units):
    w16, fp32 = units
    for sym, k in w16.items():
        body = k["body"]
        nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))
        assert len(re.findall(r"global_load_\w+ [^\n]* nt\b", body)) == nt, sym                # nothing narrower is non-temporal
        assert not re.search(r"global_load_(u|s)?(short|byte)", body), sym                       # no 2-byte fetches of weights
        assert "v_dot2" not in body and "v_mfma" not in body, sym                                # fp32 FMAs on widened weights; x is never rounded
        merge = "w16_pair_merge_kernel" in sym
        nuwb = _ints(sym)[0]
        assert nt == (4 + 16 if merge else 16 + 2 * nuwb), (sym, nt)
        # half the loads of the fp32 kernel, which reads four 16-byte pieces per unit
        assert 2 * nt == len(re.findall(r"global_load_dwordx4 [^\n]* nt", _counterpart(sym, fp32)["body"])), sym
        # every barrier in both arms of the role branch
        assert len(re.findall(r"^\s+s_barrier", body, re.M)) == (14 if merge else 10), sym
