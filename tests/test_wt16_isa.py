"""CPU (hipcc cross-compiles gfx950 without a GPU): the bf16-stream kernels of csrc/gemv_mfma_w16.hip (5..16 rows), read off the ISA.

  * every kernel fits one 8-wave workgroup per CU (<= 256 VGPRs) without scratch, and its name collides with none of the substrings by
    which the other ISA tests find the older kernels;
  * its weight loads are non-temporal 16-byte loads (`global_load_dwordx4 ... nt`), and a load carries two k-steps: per weight load the
    kernel issues twice as many `v_mfma_f32_16x16x4_f32` as the matching fp32 kernel of csrc/gemv_mfma.hip (8:1 plain, 16:1 in the
    k-step-pair form).
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

# bf16-stream kernel -> the fp32 kernel the dispatcher picks for the same launch shape (template arguments as they are mangled)
PAIRS = {
    "wt16_xreg_kernelILi1ELi16ELi8ELb0ELi0E": "gemv_rows_xreg_kernelILi1ELi16ELi16ELb0ELb0E",    # LayerNorm + QKV / FFN1 / head MLP 1
    "wt16_xreg_kernelILi1ELi16ELi8ELb0ELi2E": "gemv_rows_xreg_kernelILi1ELi16ELi16ELb0ELb0E",    # ... its all-at-entry form (opt-in)
    "wt16_xreg_kernelILi1ELi32ELi8ELb0ELi0E": "gemv_rows_xreg_kernelILi1ELi32ELi16ELb0ELb0E",    # LayerNorm, 2048 < K <= 4096
    "wt16_xreg_kernelILi0ELi16ELi8ELb0ELi0E": "gemv_rows_xreg_kernelILi0ELi16ELi16ELb0ELb0E",    # K <= 2048, no prologue
    "wt16_xreg_kernelILi0ELi32ELi8ELb0ELi0E": "gemv_rows_xreg_kernelILi0ELi32ELi16ELb0ELb0E",
    "wt16_xreg_kernelILi0ELi16ELi8ELb1ELi0E": "gemv_rows_xreg_kernelILi0ELi16ELi16ELb1ELb0E",    # out-projection (k-step pairs)
    "wt16_stream_kernelILb0E": "gemv_rows_stream_kernelILb0E",                                   # K > 2048
    "wt16_stream_kernelILb1E": "gemv_rows_stream_kernelILb1E",                                   # FFN2 (k-step pairs)
}
OLD_NAMES = ("gemv_kernel", "gemv_seg", "gemv_rows_xreg_kernel", "gemv_rows_stream_kernel", "gemv_rows32_", "gemv_pair", "w16_seg",
             "attn_decode_kernel")


def _asm(tmp_path_factory, name):
    out = tmp_path_factory.mktemp("isa_wt16") / (name + ".s")
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


def _body(asm, key):
    """the whole function of the one kernel whose symbol contains `key` (the code behind an early s_endpgm included)"""
    syms = [s for s in re.findall(r"\n(_Z\S+):", asm) if key in s]
    assert len(syms) == 1, (key, syms)
    start = asm.index("\n" + syms[0] + ":")
    return asm[start:asm.index(".Lfunc_end", start)]


def _counts(asm, key):
    body = _body(asm, key)
    nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))               # only the weights are loaded non-temporally
    return body.count("v_mfma_f32_16x16x4"), nt, body


@pytest.fixture(scope="module")
def asm_wt16(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma_w16")


@pytest.fixture(scope="module")
def asm_fp32(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma")


@needs_hipcc
def test_wt16_kernels_fit_256_vgprs_without_scratch(asm_wt16):
    meta = _meta(asm_wt16)
    assert len(meta) == len(PAIRS), sorted(meta)
    for sym, (vgpr, scratch) in meta.items():
        assert "wt16_" in sym, sym
        assert sum(key in sym for key in PAIRS) == 1, sym
        for old in OLD_NAMES:
            assert old not in sym, (sym, old)
        assert vgpr <= 256, (sym, vgpr)
        assert scratch == 0, (sym, scratch)


@needs_hipcc
@pytest.mark.parametrize("new,old", sorted(PAIRS.items()))
def test_a_weight_load_carries_two_k_steps(asm_wt16, asm_fp32, new, old):
    mfma, nt, body = _counts(asm_wt16, new)
    mfma32, nt32, _ = _counts(asm_fp32, old)
    assert nt > 0 and nt32 > 0
    assert mfma == mfma32, (new, mfma, old, mfma32)                            # the same matrix-core work ...
    assert 2 * nt == nt32, (new, nt, old, nt32)                                # ... on half as many weight loads
    assert mfma / nt == (16 if "Lb1E" in new else 8), (new, mfma, nt)
    # every other 16-byte global load of the kernel is x (plain, cached); the weights have no load of another width
    assert not re.search(r"global_load_dword(x2|x3)? [^\n]* nt", body), new
