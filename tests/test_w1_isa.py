"""CPU (hipcc cross-compiles gfx950 without a GPU): what the one-plane split GEMM (csrc/gemm_split.hip, DESIGN I.13) is for, read off the
ISA — half the matrix instructions and a third of the LDS-DMA loads of its three-plane twin, in the same registers and behind the same
drain — and that the three-plane kernels issue what they issued before the plane count became a template parameter."""
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

# one-plane kernel -> its three-plane counterpart (no ELU on load, no time-mask epilogue), as substrings of the mangled names
TWINS = {"gemm_w1_dma_kernelILi128E": "gemm_split_dma_kernelILi128ELb0ELi0ELb0E", "gemm_w1_dma_kernelILi64E": "gemm_split_dma_kernelILi64ELb0ELi0ELb0E",
         "gemm_w1_kernelILi128E": "gemm_split_kernelILi128ELb0E", "gemm_w1_kernelILi64E": "gemm_split_kernelILi64ELb0E"}
# (matrix instructions, LDS-DMA loads) of every three-plane kernel as the commit before the plane count compiled them: 2 k blocks x 6
# products x accumulators per wave; three planes in the prologue and three in the loop
PARENT_COUNTS = {"gemm_split_dma_kernelILi128ELb0ELi0ELb0E": (24, 6), "gemm_split_dma_kernelILi128ELb1ELi0ELb0E": (24, 6),
                 "gemm_split_dma_kernelILi128ELb0ELi0ELb1E": (24, 6), "gemm_split_dma_kernelILi128ELb1ELi0ELb1E": (24, 6),
                 "gemm_split_dma_kernelILi64ELb0ELi0ELb0E": (12, 6), "gemm_split_dma_kernelILi64ELb1ELi0ELb0E": (12, 6),
                 "gemm_split_kernelILi128ELb0E": (48, 0), "gemm_split_kernelILi128ELb1E": (48, 0),
                 "gemm_split_kernelILi64ELb0E": (24, 0), "gemm_split_kernelILi64ELb1E": (24, 0)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "gemm_split.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, "gemm_split.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


def _kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size, dynamic-or-static LDS bytes) from the .amdhsa metadata"""
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):
        t = m.group(0)
        g = lambda key: int(re.search(key + r":\s+(\d+)", t).group(1))
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = (g(r"\.vgpr_count"), g(r"\.private_segment_fixed_size"), g(r"\.group_segment_fixed_size"))
    return meta


def _whole_body(asm, symbol):
    start = asm.index("\n" + symbol + ":")
    return asm[start:asm.index(".Lfunc_end", start)]


def _k_loop(body):
    """the k loop's text: from its header to the first branch behind its last matrix instruction (the back edge)"""
    lo = body.index("=>This Inner Loop Header")
    last = body.rindex(MFMA)
    return body[lo:body.index("s_cbranch", last)]


def _dma_loads(text):
    return len([ln for ln in text.splitlines() if "buffer_load_dwordx4" in ln and ln.rstrip().endswith("lds")])


def _sym(meta, piece):
    found = [k for k in meta if piece in k]
    assert len(found) == 1, (piece, found)
    return found[0]


def test_one_plane_kernels_fit_128_vgprs_without_scratch(asm):
    meta = _kernel_meta(asm)
    w1 = {k: v for k, v in meta.items() if "gemm_w1_" in k}
    assert len(w1) == 4, sorted(w1)                                       # DMA 128 / 64, 4-wave 128 / 64: what the LM uses, nothing else
    for sym, (vgpr, scratch, lds) in w1.items():
        assert vgpr <= 128 and scratch == 0, (sym, vgpr, scratch)
    for piece, twin in TWINS.items():                                      # no more registers than the three-plane twin
        assert meta[_sym(meta, piece)][0] <= meta[_sym(meta, twin)][0], piece


def test_one_plane_kernels_issue_half_the_matrix_instructions_and_a_third_of_the_dma(asm):
    meta = _kernel_meta(asm)
    for piece, twin in TWINS.items():
        b1, b3 = _whole_body(asm, _sym(meta, piece)), _whole_body(asm, _sym(meta, twin))
        n1, n3 = b1.count(MFMA), b3.count(MFMA)                            # the source has them in the k loop only
        assert n3 % 6 == 0 and 2 * n1 == n3, (piece, n1, n3)
        if "dma" in piece:
            l1, l3 = _k_loop(b1), _k_loop(b3)
            assert (l1.count(MFMA), l3.count(MFMA)) == (n1, n3), piece      # ... and so has the ISA
            assert _dma_loads(l3) == 3 and _dma_loads(l1) == 1, (piece, _dma_loads(l1), _dma_loads(l3))          # per stage: three planes, one plane
            assert _dma_loads(b3) == 6 and _dma_loads(b1) == 2, (piece, _dma_loads(b1), _dma_loads(b3))          # ... and the prologue's stage
        else:
            assert _dma_loads(b1) == _dma_loads(b3) == 0, piece
            assert meta[_sym(meta, twin)][2] - meta[_sym(meta, piece)][2] == 2 * 128 * 80, piece  # static LDS: two W planes of 128 rows x 80 B less


def test_one_plane_dma_kernels_drain_their_dma_before_the_tile_barrier(asm):
    """As test_isa_guards.py test_split_gemm_drains_its_dma_before_the_tile_barrier: the W tile arrives by OTHER waves' DMA; every wave waits
    for its own (vmcnt(0)) between the loop's two barriers, in front of the first matrix instruction."""
    meta = _kernel_meta(asm)
    syms = [k for k in meta if "gemm_w1_dma_kernel" in k]
    assert len(syms) == 2, syms
    for sym in syms:
        body = _whole_body(asm, sym)
        loop = body[body.index("=>This Inner Loop Header"):]
        head = loop[:loop.index(MFMA)]
        bars = [m.start() for m in re.finditer(r"s_barrier", head)]
        assert len(bars) >= 2, sym
        assert "s_waitcnt vmcnt(0)" in head[bars[0]:bars[1]], sym


def test_three_plane_kernels_issue_what_the_parent_issued(asm):
    meta = _kernel_meta(asm)
    three = [k for k in meta if "gemm_split_dma_kernel" in k or "gemm_split_kernel" in k]
    assert len(three) == len(PARENT_COUNTS), sorted(three)
    for piece, (n_mfma, n_dma) in PARENT_COUNTS.items():
        body = _whole_body(asm, _sym(meta, piece))
        assert (body.count(MFMA), _dma_loads(body)) == (n_mfma, n_dma), (piece, body.count(MFMA), _dma_loads(body))
