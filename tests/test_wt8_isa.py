"""CPU (hipcc cross-compiles gfx950 without a GPU): the e4m3-stream kernels of csrc/gemv_mfma_w8.hip (5..16 rows), read off the ISA.

  * every kernel fits one 8-wave workgroup per CU (<= 256 VGPRs) without scratch, and its name collides with none of the substrings by
    which the other ISA tests find the older kernels;
  * its weights are loaded only by non-temporal 16-byte loads (`global_load_dwordx4 ... nt`), no narrower non-temporal load;
  * it widens with `v_cvt_pk_f32_fp8` and multiplies on `v_mfma_f32_16x16x4_f32`, no other MFMA flavour (an fp8 / bf16 MFMA would round x).
Nothing beyond that; the per-kernel table (registers, loads, conversions, MFMAs, the waits in the loops) is profiles/wt8_isa.md."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# the kernels of the unit (template arguments as they are mangled) and the launch each serves
KERNELS = {
    "wt8_xreg_kernelILi1ELi16ELb0E": "LayerNorm + QKV / FFN1 / head MLP 1",
    "wt8_xreg_kernelILi1ELi32ELb0E": "LayerNorm, 2048 < K <= 4096",
    "wt8_xreg_kernelILi0ELi16ELb0E": "K <= 2048, no prologue",
    "wt8_xreg_kernelILi0ELi32ELb0E": "the dispatcher's last arm",
    "wt8_xreg_kernelILi0ELi16ELb1E": "out-projection (k-step pairs)",
    "wt8_stream_kernelILb0E": "K > 2048",
    "wt8_stream_kernelILb1E": "FFN2 (k-step pairs)",
}
OLD_NAMES = ("gemv_kernel", "gemv_seg", "gemv_rows_xreg_kernel", "gemv_rows_stream_kernel", "gemv_rows32_", "gemv_pair", "w16_seg", "wt16_",
             "wt32_", "w8_seg", "w8_kernel", "w8_pair", "attn_decode_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_wt8") / "gemv_mfma_w8.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, "gemv_mfma_w8.hip"), "-o", str(out)]
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


@needs_hipcc
def test_wt8_kernels_fit_256_vgprs_without_scratch_under_names_of_their_own(asm):
    meta = _meta(asm)
    assert len(meta) == len(KERNELS), sorted(meta)
    for sym, (vgpr, scratch) in meta.items():
        assert "wt8_" in sym, sym
        assert sum(key in sym for key in KERNELS) == 1, sym
        for old in OLD_NAMES:
            assert old not in sym, (sym, old)
        assert vgpr <= 256, (sym, vgpr)
        assert scratch == 0, (sym, scratch)


@needs_hipcc
@pytest.mark.parametrize("key", sorted(KERNELS))
def test_wt8_weight_loads_conversions_and_mfma_flavour(asm, key):
    body = _body(asm, key)
    assert len(re.findall(r"global_load_dwordx4 [^\n]* nt", body)) > 0, key   # the codes: 16-byte non-temporal loads ...
    assert not re.search(r"global_load_(dword(x2|x3)?|[us]byte\w*|[us]short\w*) [^\n]* nt", body), key   # ... and nothing narrower
    assert "v_cvt_pk_f32_fp8" in body, key
    flavours = set(re.findall(r"\b(v_mfma_\w+)", body))
    assert flavours == {"v_mfma_f32_16x16x4_f32"}, (key, flavours)
