"""CPU (hipcc cross-compiles gfx950 without a GPU): the kernels of the bf16 KV cache (DESIGN I.14) read off the ISA — none of them uses
scratch, the K / V loads of the two attention kernels are 8-byte vector loads (half the bytes of the fp32 kernels' 16-byte loads, the same
number of them), and their VGPR counts are printed and held below what their workgroup sizes allow."""
import os

import pytest

from helpers_isa import HIPCC, compile_unit, kernel_meta, sym as _sym, body as _body, loads as _loads

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# pieces of the mangled names: the fused walk <head_dim, 2-byte entries, pages in flight>, the prefill kernel <head_dim>, the scatter <2-byte>
ROWS16 = {(hd, depth): f"attn_rows_kernelILi{hd}ELb1ELi{depth}E" for hd in (64, 128) for depth in (2, 4)}
ROWS32 = {hd: f"attn_rows_kernelILi{hd}ELb0ELi2E" for hd in (64, 128)}
PREFILL16 = {hd: f"attn_prefill_kv16_kernelILi{hd}E" for hd in (64, 128)}
PREFILL32 = {hd: f"attn_prefill_kernelILi{hd}E" for hd in (64, 128)}
SCATTER16 = "kv_scatter_kernelILb1E"


@pytest.fixture(scope="module")
def asm():
    return {name: compile_unit(name) for name in ("attn", "gemm")}


def _kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size)"""
    return {name: counts[:2] for name, counts in kernel_meta(asm).items()}


def test_new_kernels_use_no_scratch_and_their_vgprs_fit(asm):
    attn, gemm = _kernel_meta(asm["attn"]), _kernel_meta(asm["gemm"])
    for (hd, depth), piece in ROWS16.items():
        vgpr, scratch = attn[_sym(attn, piece)]
        print(f"attn_rows kv16 head_dim {hd} depth {depth}: {vgpr} VGPRs (fp32 kernel: {attn[_sym(attn, ROWS32[hd])][0]})")
        assert scratch == 0 and vgpr <= 256, (piece, vgpr, scratch)         # 512-thread workgroups: 2 waves per SIMD, 256 registers each
        if depth == 2:                                                      # the fp32 kernel's structure on half the K / V registers
            assert vgpr <= attn[_sym(attn, ROWS32[hd])][0], (piece, vgpr)
    for hd, piece in PREFILL16.items():
        vgpr, scratch = attn[_sym(attn, piece + "E")]
        print(f"attn_prefill kv16 head_dim {hd}: {vgpr} VGPRs (fp32 kernel: {attn[_sym(attn, PREFILL32[hd] + 'E')][0]})")
        assert scratch == 0 and vgpr <= 512, (piece, vgpr, scratch)         # 256-thread workgroups: one wave per SIMD
    vgpr, scratch = gemm[_sym(gemm, SCATTER16)]
    print(f"kv_scatter kv16: {vgpr} VGPRs")
    assert scratch == 0 and vgpr <= 128, (vgpr, scratch)


@pytest.mark.parametrize("hd", [64, 128])
def test_kv16_attention_loads_k_and_v_with_8_byte_vector_loads(asm, hd):
    attn = _kernel_meta(asm["attn"])
    ni = 128 // 8 // (64 // (hd // 4))                                      # K (or V) loads per wave and page: 16 keys, 64 / (hd / 4) per instruction
    fp32 = _body(asm["attn"], _sym(attn, ROWS32[hd]))
    assert (_loads(fp32, "x4"), _loads(fp32, "x2")) == (3 * 2 * ni + 1, 0)  # three issue sites of K + V, and q
    for depth in (2, 4):
        body = _body(asm["attn"], _sym(attn, ROWS16[(hd, depth)]))
        assert _loads(body, "x2") == (2 * depth - 1) * 2 * ni, (hd, depth, _loads(body, "x2"))   # depth - 1 pages ahead, depth issue sites in the loop
        assert _loads(body, "x4") == 1, (hd, depth)                         # q alone is a 16-byte load
    nld = 32 * (hd // 4) // 256                                             # tile loads per thread (K, and as many for V), at two call sites
    p32, p16 = _body(asm["attn"], _sym(attn, PREFILL32[hd] + "E")), _body(asm["attn"], _sym(attn, PREFILL16[hd] + "E"))
    assert _loads(p32, "x2") == 0 and _loads(p16, "x2") == 4 * nld
    assert _loads(p16, "x4") == _loads(p32, "x4") - 4 * nld                 # what is left are the q loads
