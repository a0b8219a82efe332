"""CPU (hipcc cross-compiles gfx950 without a GPU): the grouped attention walk of prompt sharing (DESIGN.md Part I.15) read off the ISA —
no instantiation uses scratch, each stays within the 256 VGPRs a 512-thread workgroup allows, and K / V arrive in 16-byte vector loads,
as many per issue site as in the ungrouped kernel. The counts are printed; profiles/share_isa.md holds them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

HDS, MEMBERS = (64, 128), (2, 4, 8)
GROUP = {(hd, m): f"attn_rows_group_kernelILi{hd}ELi{m}E" for hd in HDS for m in MEMBERS}
ROWS32 = {hd: f"attn_rows_kernelILi{hd}ELb0ELi2E" for hd in HDS}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "attn.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
           os.path.join(CSRC, "attn.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


def _kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size, group_segment_fixed_size) from the .amdhsa metadata"""
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):
        t = m.group(0)
        g = lambda key: int(re.search(key + r":\s+(\d+)", t).group(1))
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = (g(r"\.vgpr_count"), g(r"\.private_segment_fixed_size"), g(r"\.group_segment_fixed_size"))
    return meta


def _sym(meta, piece):
    found = [k for k in meta if piece in k]
    assert len(found) == 1, (piece, found)
    return found[0]


def _body(asm, symbol):
    start = asm.index("\n" + symbol + ":")
    return asm[start:asm.index(".Lfunc_end", start)]


def _loads(body, width):
    return len(re.findall(rf"^\s+global_load_dword{width}\b", body, re.M))


def test_every_instantiation_exists_without_scratch_within_256_vgprs(asm):
    meta = _kernel_meta(asm)
    for (hd, m), piece in GROUP.items():
        vgpr, scratch, lds = meta[_sym(meta, piece)]
        print(f"attn_rows_group head_dim {hd} members {m}: {vgpr} VGPRs, {lds} B LDS (ungrouped kernel: {meta[_sym(meta, ROWS32[hd])][0]} VGPRs)")
        assert scratch == 0, (piece, scratch)
        assert vgpr <= 256, (piece, vgpr)                                    # 512-thread workgroups: 2 waves per SIMD, 256 registers each
        assert lds == m * 8 * (hd + 4) * 4, (piece, lds)                      # one slab of the 8 waves' states per member
        assert lds <= 64 * 1024


@pytest.mark.parametrize("hd", HDS)
def test_k_and_v_arrive_in_16_byte_vector_loads(asm, hd):
    meta = _kernel_meta(asm)
    ni = 128 // 8 // (64 // (hd // 4))                                        # K (or V) loads per wave and page
    for m in MEMBERS:
        body = _body(asm, _sym(meta, GROUP[(hd, m)]))
        x4 = _loads(body, "x4")
        # the shared walk has 3 issue sites of K + V, every member's own walk 3 more; and one q per member
        assert x4 == (3 + 3 * m) * 2 * ni + m, (hd, m, x4)
        assert _loads(body, "x2") == 0 and _loads(body, "x3") == 0, (hd, m)
