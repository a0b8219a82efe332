"""CPU (hipcc cross-compiles gfx950 without a GPU): the 17..32-row GEMV kernels of csrc/gemv_mfma32.hip, read off the ISA.

  * every kernel fits one 8-wave workgroup per CU (<= 256 VGPRs) without scratch;
  * one weight fetch feeds two column tiles: per non-temporal weight load (`global_load_dwordx4 ... nt`) the kernel issues twice as many
    `v_mfma_f32_16x16x4_f32` as the matching 16-row kernel of csrc/gemv_mfma.hip (8:1 plain, 16:1 in the k-step-pair form);
  * `ssrhip_gemv` refuses 33 rows with an error that names them (no GPU needed: the check runs before any launch).
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# 32-row kernel -> the 16-row kernel the dispatcher picks for the same launch shape
PAIRS = {
    "gemv_rows32_xregILi1ELb0E": "gemv_rows_xreg_kernelILi1ELi16ELi16ELb0ELb0E",    # LayerNorm + QKV / FFN1 / head MLP 1
    "gemv_rows32_xregILi0ELb0E": "gemv_rows_xreg_kernelILi0ELi16ELi16ELb0ELb0E",    # K <= 2048, no prologue
    "gemv_rows32_xregILi0ELb1E": "gemv_rows_xreg_kernelILi0ELi16ELi16ELb1ELb0E",    # out-projection (k-step pairs)
    "gemv_rows32_streamILb0E": "gemv_rows_stream_kernelILb0E",                       # K > 2048
    "gemv_rows32_streamILb1E": "gemv_rows_stream_kernelILb1E",                       # FFN2 (k-step pairs)
}


def _asm(tmp_path_factory, name):
    out = tmp_path_factory.mktemp("isa32") / (name + ".s")
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


def _symbol(asm, key):
    syms = [s for s in re.findall(r"\n(_Z\S+):", asm) if key in s]
    assert len(syms) == 1, (key, syms)
    return syms[0]


def _mfma_per_weight_load(asm, key):
    sym = _symbol(asm, key)
    start = asm.index("\n" + sym + ":")
    body = asm[start:asm.index("s_endpgm", start)]
    mfma = body.count("v_mfma_f32_16x16x4")
    loads = len(re.findall(r"global_load_dwordx4 [^\n]* nt", body))     # only the weights are loaded non-temporally
    assert loads > 0, sym
    return mfma / loads


@pytest.fixture(scope="module")
def asm32(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma32")


@pytest.fixture(scope="module")
def asm16(tmp_path_factory):
    return _asm(tmp_path_factory, "gemv_mfma")


@needs_hipcc
def test_rows32_kernels_fit_256_vgprs_without_scratch(asm32):
    meta = _meta(asm32)
    assert len(meta) == len(PAIRS), sorted(meta)
    for sym, (vgpr, scratch) in meta.items():
        assert "gemv_rows32_" in sym, sym
        for old in ("gemv_kernel", "gemv_seg", "gemv_rows_xreg_kernel", "gemv_rows_stream_kernel", "gemv_pair", "attn_decode_kernel"):
            assert old not in sym, (sym, old)          # test_isa_guards.py finds the older kernels by these substrings
        assert vgpr <= 256, (sym, vgpr)
        assert scratch == 0, (sym, scratch)


@needs_hipcc
@pytest.mark.parametrize("new,old", sorted(PAIRS.items()))
def test_one_weight_fetch_feeds_two_column_tiles(asm32, asm16, new, old):
    r32, r16 = _mfma_per_weight_load(asm32, new), _mfma_per_weight_load(asm16, old)
    assert r32 == 2 * r16, (new, r32, old, r16)
    assert r32 == (16 if "Lb1E" in new else 8), (new, r32)


def test_gemv_refuses_33_rows():
    from ssr_speech_amd import _lib
    try:
        L = _lib.lib()
    except _lib.SsrHipUnavailable as e:
        pytest.skip(str(e))
    a = _lib.GemvArgs()
    a.W, a.y, a.x = 0x1000, 0x2000, 0x3000                 # never dereferenced: the row count is refused before any launch
    a.B, a.N, a.K, a.groups = 33, 512, 2048, 1
    a.x_tiled, a.y_tiled = 1, 1
    assert L.ssrhip_gemv(C.byref(a), None) != 0
    assert b"B=33" in L.ssrhip_last_error()
