"""CPU (hipcc cross-compiles gfx950 without a GPU): the e4m3-weight-stream kernels of csrc/gemv_w8.hip, read off the ISA.

  * the kernels are all there under their own names, and no symbol carries a substring by which the older ISA tests find the fp32 / bf16
    kernels;
  * no kernel spills (private_segment_fixed_size == 0) and each stays within the registers its `__launch_bounds__` promise: 128 VGPRs for
    the generic form at two 512-thread workgroups per CU, 256 for the merge prologue and for the straight-line form;
  * the weights arrive as 16-byte non-temporal loads (`global_load_dwordx4 ... nt`), one per (row, 1024-element) unit — the straight-line
    form issues exactly NUW of them — and nothing is fetched in 1- or 2-byte pieces;
  * the codes are widened by `v_cvt_pk_f32_fp8` (two per instruction: 8 per unit), and there is no `v_dot2` (x is never rounded).
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

OLDER = ("gemv_kernel", "gemv_seg", "gemv_pair", "gemv_rows", "attn_decode_kernel", "w16_seg", "wt16_", "wt32_")
RING = 4                      # csrc/gemv_w8.hip W8_RING: units in flight per wave of the generic form


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """symbol -> (vgpr_count, private_segment_fixed_size, body)"""
    out = tmp_path_factory.mktemp("isa_w8") / "gemv_w8.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, "gemv_w8.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = open(out).read()
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S):
        v = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", asm[m.start() - 400:m.end()])
        assert v and p, m.group(1)
        sym = m.group(1)
        start = asm.index("\n" + sym + ":")
        found[sym] = (int(v.group(1)), int(p.group(1)), asm[start:asm.index("s_endpgm", start)])
    return found


def _template_ints(sym):
    return [int(x) for x in re.findall(r"Li(\d+)E", sym)]


@needs_hipcc
def test_w8_kernels_are_all_there_under_their_own_names(kernels):
    seg = sorted(s for s in kernels if "w8_seg_kernel" in s)
    segu = sorted(s for s in kernels if "w8_segu_kernel" in s)
    assert len(seg) + len(segu) == len(kernels), sorted(kernels)
    assert sorted(_template_ints(s) for s in seg) == sorted([b, pro] for b in (1, 2, 4) for pro in (0, 1, 2))
    # B in {1, 2, 4}, PRO in {NONE, LAYERNORM}, NUW in {4, 6, 8}, DEPTH = 2, 4 or NUW (every unit at entry)
    assert sorted(_template_ints(s) for s in segu) == sorted([b, pro, nuw, d] for b in (1, 2, 4) for pro in (0, 1) for nuw in (4, 6, 8) for d in {nuw, 4, 2})
    for sym in kernels:
        for old in OLDER:
            assert old not in sym, (sym, old)


@needs_hipcc
def test_w8_kernels_fit_their_launch_bounds_without_scratch(kernels):
    for sym, (vgpr, scratch, _) in kernels.items():
        assert scratch == 0, (sym, scratch)
        if "w8_seg_kernel" in sym:
            limit = 256 if _template_ints(sym)[1] == 2 else 128   # the merge prologue runs at one 512-thread workgroup per CU, the others at two
        else:
            limit = 256                                           # __launch_bounds__(512, 2): one workgroup of 8 waves per CU
        assert vgpr <= limit, (sym, vgpr, limit)


@needs_hipcc
def test_w8_weights_arrive_as_16_byte_non_temporal_loads_and_are_widened_in_hardware(kernels):
    for sym, (_, _, body) in kernels.items():
        nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))
        cvt = len(re.findall(r"v_cvt_pk_f32_fp8", body))
        assert not re.search(r"global_load_(u|s)?(short|byte)", body), sym        # no 1- or 2-byte fetches of weights
        assert not re.search(r"global_load_dword(x2|x3)? [^\n]* nt", body), sym   # and no narrower non-temporal ones
        assert "v_dot2" not in body, sym                                          # fp32 FMAs on widened weights, x is never rounded
        assert not re.search(r"v_cvt_(pk_)?f32_bf8|v_cvt_f32_fp8", body), sym     # e4m3, two codes per instruction
        if "w8_segu_kernel" in sym:
            nuw = _template_ints(sym)[2]
            assert nt == nuw, (sym, nt)               # straight-line: every unit's one piece exactly once
        else:
            assert nt == 3 * RING - 1, (sym, nt)      # RING units at entry, the refill loop (RING), the tail's refills (RING - 1)
        assert cvt == 8 * nt, (sym, cvt, nt)          # every place a unit is used widens its 16 codes, and nothing else is widened
