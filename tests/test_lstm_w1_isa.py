"""CPU (hipcc cross-compiles gfx950 without a GPU): what the one-plane LSTM step (DESIGN I.31, csrc/lstm_w1.hip) compiles to, read off the
ISA in the manner of tests/test_codec_w1_isa.py — and that the three-plane step beside it (csrc/lstm_split.hip), which now shares its
text outside the k-loop with the new kernel through csrc/lstm_split_step.h, still compiles to what the parent commit's build has.

  * every `lstm_step_w1_kernel<DEPTH>` (DEPTH 2, 4, 8): no scratch, at least 12 DEPTH matrix instructions and 8 DEPTH 16-byte loads in
    the k-loop (12 + 8 per k-step where the three-plane step has 24 + 12), and no `vmcnt(0)` in the k-loop — one wave per SIMD has nobody
    to hide an L2 round trip behind, so the refills must stay DEPTH - 1 MFMA blocks ahead;
  * `lstm_step_split_kernel<2>` / `<4>`: the VGPRs, matrix instructions and loads of the parent commit.
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
LOAD = "global_load_dwordx4"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# DEPTH -> (VGPRs, matrix instructions, 16-byte loads in the k-loop) of lstm_step_split_kernel<DEPTH> in a build of the parent commit
# (hipcc of ROCm 7.2, the flags of `_asm` below)
SPLIT_PARENT = {2: (208, 48, 24), 4: (304, 96, 48)}
W1_DEPTHS = (2, 4, 8)


def _asm(tmp_path_factory, name):
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, name + ".hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


@pytest.fixture(scope="module")
def w1_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "lstm_w1")


@pytest.fixture(scope="module")
def split_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "lstm_split")


def _kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size) from the .amdhsa metadata"""
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):
        t = m.group(0)
        g = lambda key: int(re.search(key + r":\s+(\d+)", t).group(1))                 # noqa: E731
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = (g(r"\.vgpr_count"), g(r"\.private_segment_fixed_size"))
    return meta


def _k_loop(asm, symbol):
    """the k-loop of a step kernel: from the inner loop's header to its back edge (the loop ends in front of the LDS meeting's barrier)"""
    start = asm.index("\n" + symbol + ":")
    body = asm[start:asm.index(".Lfunc_end", start)]
    lo = body.index("=>This Inner Loop Header")
    loop = body[lo:body.index("s_barrier", lo)]
    return loop[:loop.rindex("s_cbranch")]


def _by_depth(meta, family):
    found = {int(re.search(family + r"ILi(\d+)E", k).group(1)): k for k in meta if family in k}
    return found


def test_the_one_plane_step_has_these_three_depths_and_another_name(w1_asm, split_asm):
    assert sorted(_by_depth(_kernel_meta(w1_asm), "lstm_step_w1_kernel")) == list(W1_DEPTHS)
    assert not [k for k in _kernel_meta(w1_asm) if "lstm_step_split_kernel" in k]
    assert not [k for k in _kernel_meta(split_asm) if "lstm_step_w1_kernel" in k]


def test_one_plane_step_no_scratch_half_the_products_two_thirds_of_the_loads_and_its_prefetch_distance(w1_asm):
    meta = _kernel_meta(w1_asm)
    for depth, sym in _by_depth(meta, "lstm_step_w1_kernel").items():
        vgpr, scratch = meta[sym]
        assert scratch == 0 and vgpr <= 512, (depth, vgpr, scratch)
        loop = _k_loop(w1_asm, sym)
        assert loop.count(MFMA) >= 12 * depth, (depth, loop.count(MFMA))
        assert loop.count(LOAD) >= 8 * depth, (depth, loop.count(LOAD))
        assert "vmcnt(0)" not in loop, depth


def test_one_plane_step_needs_fewer_registers_than_its_three_plane_twin(w1_asm, split_asm):
    m1, m3 = _kernel_meta(w1_asm), _kernel_meta(split_asm)
    w1, s3 = _by_depth(m1, "lstm_step_w1_kernel"), _by_depth(m3, "lstm_step_split_kernel")
    for depth in SPLIT_PARENT:
        assert m1[w1[depth]][0] < m3[s3[depth]][0], (depth, m1[w1[depth]], m3[s3[depth]])       # 8 operand blocks per slot instead of 12


def test_three_plane_step_compiles_to_what_the_parent_compiled(split_asm):
    meta = _kernel_meta(split_asm)
    syms = _by_depth(meta, "lstm_step_split_kernel")
    assert sorted(syms) == sorted(SPLIT_PARENT)
    for depth, (vgpr, mfma, loads) in SPLIT_PARENT.items():
        loop = _k_loop(split_asm, syms[depth])
        assert (meta[syms[depth]], loop.count(MFMA), loop.count(LOAD)) == ((vgpr, 0), mfma, loads), (depth, meta[syms[depth]])
        assert "vmcnt(0)" not in loop, depth
