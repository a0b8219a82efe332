"""CPU (hipcc cross-compiles gfx950 without a GPU): the bf16-stream kernels of csrc/gemv_mfma32_w16.hip (17..32 rows), read off the ISA.

  * every kernel fits one 8-wave workgroup per CU (<= 256 VGPRs) without scratch, and its name collides with none of the substrings by
    which the other ISA tests find the older kernels;
  * its weight loads are non-temporal 16-byte loads (`global_load_dwordx4 ... nt`), and a load carries two k-steps for both panels: against
    the matching fp32 kernel of csrc/gemv_mfma32.hip the same number of `v_mfma_f32_16x16x4_f32` on half as many weight loads (16:1 plain,
    32:1 in the k-step-pair form).
Register counts and load-to-MFMA ratios only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# bf16-stream kernel -> the fp32 kernel ssrhip_gemv_mfma32_launch picks for the same launch shape (template arguments as they are mangled)
PAIRS = {
    "wt32_xreg_kernelILi1ELb0E": "gemv_rows32_xregILi1ELb0E",      # LayerNorm + QKV / FFN1 / head MLP 1
    "wt32_xreg_kernelILi0ELb0E": "gemv_rows32_xregILi0ELb0E",      # K <= 2048, no prologue
    "wt32_xreg_kernelILi0ELb1E": "gemv_rows32_xregILi0ELb1E",      # out-projection (k-step pairs)
    "wt32_stream_kernelILb0E": "gemv_rows32_streamILb0E",          # K > 2048
    "wt32_stream_kernelILb1E": "gemv_rows32_streamILb1E",          # FFN2 (k-step pairs)
}
# tests/test_wt16_isa.py's OLD_NAMES, and the 5..16-row stream's own prefix
OLD_NAMES = ("gemv_kernel", "gemv_seg", "gemv_rows_xreg_kernel", "gemv_rows_stream_kernel", "gemv_rows32_", "gemv_pair", "w16_seg",
             "attn_decode_kernel", "wt16_")


def _asm(tmp_path_factory, name):
    out = tmp_path_factory.mktemp("isa_wt32") / (name + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, name + ".hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


def _meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size)"""
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S):
        v = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", asm[m.start() - 400:m.end()])
        if v and p:
            meta[m.group(1)] = (int(v.group(1)), int(p.group(1)))
    return meta


def _counts(asm, key):
    """(MFMAs, non-temporal 16-byte loads, text) of the whole function of the one kernel whose symbol contains `key`"""
    syms = [s for s in re.findall(r"\n(_Z\S+):", asm) if key in s]
    assert len(syms) == 1, (key, syms)
    start = asm.index("\n" + syms[0] + ":")
    body = asm[start:asm.index(".Lfunc_end", start)]
    nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))               # only the weights are loaded non-temporally
    return body.count("v_mfma_f32_16x16x4"), nt, body


@pytest.fixture(scope="module")
def asm_wt32(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma32_w16")


@pytest.fixture(scope="module")
def asm_fp32(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma32")


@needs_hipcc
def test_wt32_kernels_fit_256_vgprs_without_scratch(asm_wt32):
    meta = _meta(asm_wt32)
    assert len(meta) == len(PAIRS), sorted(meta)
    for sym, (vgpr, scratch) in meta.items():
        assert "wt32_" in sym, sym
        assert sum(key in sym for key in PAIRS) == 1, sym
        for old in OLD_NAMES:
            assert old not in sym, (sym, old)
        assert vgpr <= 256, (sym, vgpr)
        assert scratch == 0, (sym, scratch)


@needs_hipcc
@pytest.mark.parametrize("new,old", sorted(PAIRS.items()))
def test_a_weight_load_carries_two_k_steps_for_both_panels(asm_wt32, asm_fp32, new, old):
    mfma, nt, body = _counts(asm_wt32, new)
    mfma32, nt32, _ = _counts(asm_fp32, old)
    assert nt > 0 and nt32 > 0
    assert mfma == mfma32, (new, mfma, old, mfma32)                            # the same matrix-core work ...
    assert 2 * nt == nt32, (new, nt, old, nt32)                                # ... on half as many weight loads
    assert mfma / nt == (32 if "Lb1E" in new else 16), (new, mfma, nt)
    # every other 16-byte global load of the kernel is x (plain, cached); the weights have no load of another width
    assert not re.search(r"global_load_dword(x2|x3)? [^\n]* nt", body), new
