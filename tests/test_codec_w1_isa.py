"""CPU (hipcc cross-compiles gfx950 without a GPU): what the one-plane codec kernels (DESIGN I.30) are for, read off the ISA as
tests/test_w1_isa.py does for the LM's — matrix instructions, LDS-DMA loads, VGPRs and scratch bytes, nothing else.

  * every new GEMM kernel (csrc/gemm_split.hip `codec_w1_dma_kernel<BM, ELU, TMF>`, `codec_w1_kernel<BM, ELU>`) has half the matrix
    instructions and a third of the LDS-DMA loads of its three-plane twin with the same <BM, ELU, TMF>, no more VGPRs, no scratch;
  * the one-plane residual-block kernels (csrc/resblock_split.hip `resblock_w1_dma_kernel<C, RING>`) have half the matrix instructions
    of their three-plane twins, the weight DMA loads of a tile of a third of the bytes, and no scratch;
  * the three-plane residual-block kernels issue what the parent commit's build issues.
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

# new GEMM kernel -> its three-plane twin with the same <BM, ELU, TMF>, as substrings of the mangled names
GEMM_TWINS = {"codec_w1_dma_kernelILi128ELb1ELb0E": "gemm_split_dma_kernelILi128ELb1ELi0ELb0E",
              "codec_w1_dma_kernelILi64ELb1ELb0E": "gemm_split_dma_kernelILi64ELb1ELi0ELb0E",
              "codec_w1_dma_kernelILi128ELb0ELb1E": "gemm_split_dma_kernelILi128ELb0ELi0ELb1E",
              "codec_w1_dma_kernelILi128ELb1ELb1E": "gemm_split_dma_kernelILi128ELb1ELi0ELb1E",
              "codec_w1_kernelILi128ELb1E": "gemm_split_kernelILi128ELb1E",
              "codec_w1_kernelILi64ELb1E": "gemm_split_kernelILi64ELb1E"}
# (C, ring) -> (matrix instructions, LDS-DMA loads) of resblock_split_dma_kernel<C, ring, 0> in a build of the parent commit (hipcc of
# ROCm 7.2, the flags of `_asm` below). C = 128: the first channel tile peeled + one tile in the loop (2 x 3 taps x 24) + stage 2 (96)
RESBLOCK_PARENT = {(128, 2): (240, 33), (128, 4): (240, 39), (64, 2): (60, 12), (64, 4): (60, 16)}


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


def test_the_new_gemm_kernels_are_these_six(gemm_asm):
    new = sorted(k for k in _kernel_meta(gemm_asm) if "codec_w1_" in k)
    assert len(new) == len(GEMM_TWINS) and all(any(p in k for k in new) for p in GEMM_TWINS), new
    # the forms without ELU on load and time mask are ssrhip_gemm_w1's kernels: not compiled a second time
    assert not [k for k in new if "ELb0ELb0E" in k or "codec_w1_kernelILi128ELb0E" in k or "codec_w1_kernelILi64ELb0E" in k], new


def test_new_gemm_kernels_half_the_matrix_instructions_a_third_of_the_dma(gemm_asm):
    meta = _kernel_meta(gemm_asm)
    for piece, twin in GEMM_TWINS.items():
        b1, b3 = _whole_body(gemm_asm, _sym(meta, piece)), _whole_body(gemm_asm, _sym(meta, twin))
        n1, n3 = b1.count(MFMA), b3.count(MFMA)
        assert n3 % 6 == 0 and n1 > 0 and 2 * n1 == n3, (piece, n1, n3)
        d1, d3 = _dma_loads(b1), _dma_loads(b3)
        if "dma" in piece:
            assert d3 % 3 == 0 and d1 > 0 and 3 * d1 == d3, (piece, d1, d3)
        else:
            assert d1 == d3 == 0, (piece, d1, d3)


def test_new_gemm_kernels_use_no_more_vgprs_than_the_twin_and_no_scratch(gemm_asm):
    meta = _kernel_meta(gemm_asm)
    for piece, twin in GEMM_TWINS.items():
        vgpr, scratch = meta[_sym(meta, piece)]
        assert scratch == 0 and vgpr <= meta[_sym(meta, twin)][0], (piece, vgpr, scratch, meta[_sym(meta, twin)])


def _res_sym(meta, family, Cc, ring):
    return _sym(meta, f"{family}ILi{Cc}ELi{ring}E")


def test_three_plane_resblock_kernels_issue_what_the_parent_issued(res_asm):
    meta = _kernel_meta(res_asm)
    assert len([k for k in meta if "resblock_split_dma_kernel" in k]) == len(RESBLOCK_PARENT)
    for (Cc, ring), want in RESBLOCK_PARENT.items():
        body = _whole_body(res_asm, _res_sym(meta, "resblock_split_dma_kernel", Cc, ring))
        assert (body.count(MFMA), _dma_loads(body)) == want, (Cc, ring, body.count(MFMA), _dma_loads(body))


def test_one_plane_resblock_kernels_half_the_matrix_instructions_and_the_dma_of_a_third_of_the_tile(res_asm):
    """A weight tile is C/32 KiB-DMAs instead of 3 C/32, dealt over the four waves: every wave issues ceil(C/128) instead of ceil(3 C/128)
    per tile. C = 128: 1 instead of 3 — a third of the DMA instructions. C = 64: the three-plane tile's 6 KiB take 2 instructions per
    wave (the surplus repeats the last KiB), the one-plane tile's 2 KiB take 1: half the INSTRUCTIONS for a third of the bytes — a wave
    cannot issue less than one, and no load runs under a run-time predicate."""
    meta = _kernel_meta(res_asm)
    one = [k for k in meta if "resblock_w1_dma_kernel" in k]
    assert len(one) == 4, sorted(one)
    for (Cc, ring) in RESBLOCK_PARENT:
        s1, s3 = _res_sym(meta, "resblock_w1_dma_kernel", Cc, ring), _res_sym(meta, "resblock_split_dma_kernel", Cc, ring)
        b1, b3 = _whole_body(res_asm, s1), _whole_body(res_asm, s3)
        n1, n3 = b1.count(MFMA), b3.count(MFMA)
        assert n3 % 6 == 0 and n1 > 0 and 2 * n1 == n3, (Cc, ring, n1, n3)
        per_wave1, per_wave3 = -(-(Cc // 32) // 4), -(-(3 * Cc // 32) // 4)
        assert (per_wave1, per_wave3) == ((1, 3) if Cc == 128 else (1, 2))
        d1, d3 = _dma_loads(b1), _dma_loads(b3)
        assert d1 > 0 and d1 * per_wave3 == d3 * per_wave1, (Cc, ring, d1, d3)
        assert meta[s1][1] == 0 and meta[s3][1] == 0, (Cc, ring, meta[s1], meta[s3])     # no scratch
        assert meta[s1][0] <= meta[s3][0], (Cc, ring, meta[s1], meta[s3])                # ... and no more registers than the twin
