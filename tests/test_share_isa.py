"""CPU (hipcc cross-compiles gfx950 without a GPU): the grouped attention walk of prompt sharing (DESIGN.md Part I.15) read off the ISA —
no instantiation uses scratch, each stays within the 256 VGPRs a 512-thread workgroup allows, and K / V arrive in 16-byte vector loads,
as many per issue site as in the ungrouped kernel. The counts are printed; profiles/share_isa.md holds them."""
import os

import pytest

from helpers_isa import HIPCC, compile_unit, kernel_meta as _kernel_meta, sym as _sym, body as _body, loads as _loads

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

HDS, MEMBERS = (64, 128), (2, 4, 8)
GROUP = {(hd, m): f"attn_rows_group_kernelILi{hd}ELi{m}E" for hd in HDS for m in MEMBERS}
ROWS32 = {hd: f"attn_rows_kernelILi{hd}ELb0ELi2E" for hd in HDS}


@pytest.fixture(scope="module")
def asm():
    return compile_unit("attn")


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
