"""CPU (hipcc cross-compiles gfx950 without a GPU): code-generation properties of the scoring kernel (csrc/score.hip), read off the ISA:
`xent_rank_kernel` does not spill, streams the logits with 16-byte loads, and reduces across the wave without LDS (DPP / permlane)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def score_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "score.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, "score.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


def _symbol(asm):
    syms = re.findall(r"^(\S*xent_rank_kernel\S*):", asm, re.M)
    assert len(syms) == 1, syms
    return syms[0]


def test_xent_rank_kernel_does_not_spill(score_asm):
    sym = _symbol(score_asm)
    m = re.search(r"\.name:\s+" + re.escape(sym) + r"\n(.*?)\.wavefront_size", score_asm, re.S)
    assert m, sym
    body = m.group(1)
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)) <= 64          # 8 waves per SIMD


def test_xent_rank_kernel_streams_dwordx4_and_reduces_without_lds(score_asm):
    sym = _symbol(score_asm)
    start = score_asm.index("\n" + sym + ":")
    code = score_asm[start:score_asm.index("s_endpgm", start)]
    assert "global_load_dwordx4" in code
    assert "v_permlane32_swap" in code and "row_ror" in code
    assert not re.search(r"\bds_(read|write|bpermute|swizzle)", code)
