"""CPU (hipcc cross-compiles gfx950 without a GPU): what the bf16-activation codec kernels (DESIGN I.32) are for, read off the ISA as
tests/test_codec_w1_isa.py does for the one-plane kernels — matrix instructions, LDS-DMA loads, VGPRs and scratch bytes, nothing else.

  * every new GEMM kernel (csrc/gemm_split.hip `codec_a1_dma_kernel<BM, ELU, TMF>`, `codec_a1_kernel<BM, ELU>`) has a third of the matrix
    instructions of its one-plane twin (`codec_w1_*`, or `gemm_w1_*` for the forms without ELU on load and time mask), the same number
    of LDS-DMA loads, no more VGPRs, no scratch;
  * the residual-block kernels (csrc/resblock_split.hip `resblock_a1_dma_kernel<C, RING>`) have a third of the matrix instructions of
    `resblock_w1_dma_kernel<C, RING>`, the same DMA loads, no scratch;
  * no new kernel's name contains an existing kernel's name: the `in` searches of the older ISA tests keep finding what they found.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MFMA = "v_mfma_f32_32x32x16_bf16"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# new GEMM kernel -> its one-plane twin of the same <BM, ELU, TMF>, as substrings of the mangled names
GEMM_TWINS = {"codec_a1_dma_kernelILi128ELb1ELb0E": "codec_w1_dma_kernelILi128ELb1ELb0E",
              "codec_a1_dma_kernelILi64ELb1ELb0E": "codec_w1_dma_kernelILi64ELb1ELb0E",
              "codec_a1_dma_kernelILi128ELb0ELb1E": "codec_w1_dma_kernelILi128ELb0ELb1E",
              "codec_a1_dma_kernelILi128ELb1ELb1E": "codec_w1_dma_kernelILi128ELb1ELb1E",
              "codec_a1_dma_kernelILi128ELb0ELb0E": "gemm_w1_dma_kernelILi128E",
              "codec_a1_dma_kernelILi64ELb0ELb0E": "gemm_w1_dma_kernelILi64E",
              "codec_a1_kernelILi128ELb1E": "codec_w1_kernelILi128ELb1E",
              "codec_a1_kernelILi64ELb1E": "codec_w1_kernelILi64ELb1E",
              "codec_a1_kernelILi128ELb0E": "gemm_w1_kernelILi128E",
              "codec_a1_kernelILi64ELb0E": "gemm_w1_kernelILi64E"}
RESBLOCK_FORMS = [(128, 2), (128, 4), (64, 2), (64, 4)]
# the kernel families of the two files before the bf16-activation kernels (every older ISA test finds its kernels by one of these)
OLD_FAMILIES = ("gemm_split_dma_kernel", "gemm_split_kernel", "gemm_w1_dma_kernel", "gemm_w1_kernel", "codec_w1_dma_kernel", "codec_w1_kernel",
                "codec_w1_", "gemm_w1_", "split_weights_kernel", "resblock_split_dma_kernel", "resblock_w1_dma_kernel")


def _asm(tmp_path_factory, name):
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, name + ".hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


@pytest.fixture(scope="module")
def gemm_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "gemm_split")


@pytest.fixture(scope="module")
def res_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "resblock_split")


def _kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size) from the .amdhsa metadata"""
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):
        t = m.group(0)
        g = lambda key: int(re.search(key + r":\s+(\d+)", t).group(1))                 # noqa: E731
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = (g(r"\.vgpr_count"), g(r"\.private_segment_fixed_size"))
    return meta


def _whole_body(asm, symbol):
    start = asm.index("\n" + symbol + ":")
    return asm[start:asm.index(".Lfunc_end", start)]


def _dma_loads(text):
    return len([ln for ln in text.splitlines() if "buffer_load_dwordx4" in ln and ln.rstrip().endswith("lds")])


def _sym(meta, piece):
    found = [k for k in meta if piece in k]
    assert len(found) == 1, (piece, found)
    return found[0]


def test_the_new_gemm_kernels_are_these_ten(gemm_asm):
    """Every form ssrhip_codec_gemm_w1 dispatches has a bf16-activation kernel of its own, the no-ELU forms included."""
    new = sorted(k for k in _kernel_meta(gemm_asm) if "codec_a1_" in k)
    assert len(new) == len(GEMM_TWINS) == 10 and all(any(p in k for k in new) for p in GEMM_TWINS), new


def test_no_new_kernel_name_contains_an_old_one(gemm_asm, res_asm):
    new = [k for k in list(_kernel_meta(gemm_asm)) + list(_kernel_meta(res_asm)) if "_a1_" in k]
    assert len(new) == 14, sorted(new)
    for k in new:
        assert not [f for f in OLD_FAMILIES if f in k], k


def test_new_gemm_kernels_a_third_of_the_matrix_instructions_the_same_dma(gemm_asm):
    meta = _kernel_meta(gemm_asm)
    for piece, twin in GEMM_TWINS.items():
        ba, b1 = _whole_body(gemm_asm, _sym(meta, piece)), _whole_body(gemm_asm, _sym(meta, twin))
        na, n1 = ba.count(MFMA), b1.count(MFMA)
        assert n1 % 3 == 0 and na > 0 and 3 * na == n1, (piece, na, n1)
        da, d1 = _dma_loads(ba), _dma_loads(b1)
        assert da == d1 and (da > 0) == ("dma" in piece), (piece, da, d1)


def test_new_gemm_kernels_use_no_more_vgprs_than_the_twin_and_no_scratch(gemm_asm):
    meta = _kernel_meta(gemm_asm)
    for piece, twin in GEMM_TWINS.items():
        vgpr, scratch = meta[_sym(meta, piece)]
        assert scratch == 0 and vgpr <= meta[_sym(meta, twin)][0], (piece, vgpr, scratch, meta[_sym(meta, twin)])


def test_new_gemm_kernels_convert_once_per_float4(gemm_asm):
    """One `v_cvt_pk_bf16_f32` per pair of activations where the twin issues three (the conversion `split4` starts with, nothing behind it)."""
    meta = _kernel_meta(gemm_asm)
    for piece, twin in GEMM_TWINS.items():
        ca, c1 = (_whole_body(gemm_asm, _sym(meta, p)).count("v_cvt_pk_bf16_f32") for p in (piece, twin))
        assert ca > 0 and 3 * ca == c1, (piece, ca, c1)


def test_resblock_kernels_a_third_of_the_matrix_instructions_the_same_dma_no_scratch(res_asm):
    meta = _kernel_meta(res_asm)
    new = [k for k in meta if "resblock_a1_dma_kernel" in k]
    assert len(new) == len(RESBLOCK_FORMS), sorted(new)
    for Cc, ring in RESBLOCK_FORMS:
        sa, s1 = (_sym(meta, f"{fam}ILi{Cc}ELi{ring}E") for fam in ("resblock_a1_dma_kernel", "resblock_w1_dma_kernel"))
        ba, b1 = _whole_body(res_asm, sa), _whole_body(res_asm, s1)
        na, n1 = ba.count(MFMA), b1.count(MFMA)
        assert n1 % 3 == 0 and na > 0 and 3 * na == n1, (Cc, ring, na, n1)
        assert _dma_loads(ba) == _dma_loads(b1) > 0, (Cc, ring, _dma_loads(ba), _dma_loads(b1))
        assert meta[sa][1] == 0, (Cc, ring, meta[sa])                                   # no scratch
        assert meta[sa][0] <= 170, (Cc, ring, meta[sa])                                 # three waves per SIMD, as the twin (146-152 VGPRs)
