"""CPU (hipcc cross-compiles gfx950 without a GPU): the split-KV attention kernel of the bf16 cache of the 1/2/4-row step (DESIGN.md Part
I.23), `attn_decode_kernel<head_dim, false, VAT, true>`, read off the ISA — no scratch, its K / V loads from the pool are 8-byte vector
loads (as many as the fp32 kernel has 16-byte ones), it needs no more VGPRs than the fp32 kernel of the same build at each head_dim
and VAT (the figures are printed), and the register its `prefetch` touch lands in stays untouched while the touch can be in flight."""
import os
import re

import pytest

from helpers_isa import HIPCC, compile_unit, kernel_meta, sym as _sym, body as _body, loads as _loads

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# (head_dim, VAT) of the instantiations the launcher can reach; VAT is spelled n1 for -1 in a mangled name
CASES = [(64, -1), (128, -1), (128, 4), (128, 8), (128, 12)]


def _piece(hd, vat, kv16):
    return f"attn_decode_kernelILi{hd}ELb0ELi{'n1' if vat < 0 else vat}ELb{int(kv16)}E"


@pytest.fixture(scope="module")
def asm():
    return compile_unit("attn")


@pytest.mark.parametrize("hd,vat", CASES)
def test_no_scratch(asm, hd, vat):
    meta = kernel_meta(asm)
    vgpr, scratch, lds = meta[_sym(meta, _piece(hd, vat, True))]
    assert scratch == 0, (hd, vat, scratch)
    assert lds == meta[_sym(meta, _piece(hd, vat, False))][2]                # the 4-wave merge buffer and nothing else


@pytest.mark.parametrize("hd,vat", CASES)
def test_pool_loads_are_8_byte_vector_loads(asm, hd, vat):
    meta = kernel_meta(asm)
    ni = 32 // (64 // (hd // 4))                                            # K (or V) loads per wave: 32 keys, 64 / (hd / 4) per instruction
    fp32, kv16 = _body(asm, _sym(meta, _piece(hd, vat, False))), _body(asm, _sym(meta, _piece(hd, vat, True)))
    assert (_loads(fp32, "x4"), _loads(fp32, "x2")) == (2 * ni + 2, 0)      # K + V, q, and the prefetch experiment's touch
    assert _loads(kv16, "x2") == 2 * ni, (hd, vat, _loads(kv16, "x2"))      # K + V of the pool: half the bytes, the same count
    assert _loads(kv16, "x4") == 3, (hd, vat, _loads(kv16, "x4"))           # q and the landing K and V (fp32)
    assert kv16.count("global_store_dwordx2") == 2 + fp32.count("global_store_dwordx2")   # the promoted K and V, 8 bytes per lane


@pytest.mark.parametrize("hd,vat", CASES)
def test_vgprs_are_not_above_the_fp32_kernels(asm, hd, vat):
    meta = kernel_meta(asm)
    v16, v32 = meta[_sym(meta, _piece(hd, vat, True))][0], meta[_sym(meta, _piece(hd, vat, False))][0]
    print(f"attn_decode kv16 head_dim {hd} VAT {vat}: {v16} VGPRs (fp32 kernel: {v32})")
    assert v16 <= v32, (hd, vat, v16, v32)


def _named(line):
    """the VGPR numbers an instruction names, singly or inside a range"""
    code = line.split(";")[0]
    out = {int(x) for x in re.findall(r"\bv(\d+)\b", code)}
    for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", code):
        out |= set(range(int(lo), int(hi) + 1))
    return out


@pytest.mark.parametrize("hd,vat", CASES)
def test_the_prefetch_touch_keeps_its_register_until_a_k_row_has_arrived(asm, hd, vat):
    """The touch of `a->prefetch` is a load the compiler does not count, so nothing may write its destination while it can be in flight:
    from the touch to the statement that consumes the landing entry — which waits for the first K row, a younger request — no instruction
    names the register, except its zero-initialisation in the block that bypasses the touch loop (behind a label: not reachable from it)."""
    meta = kernel_meta(asm)
    lines = _body(asm, _sym(meta, _piece(hd, vat, True))).split("\n")
    touch = [i for i, l in enumerate(lines) if re.match(r"\s+global_load_dword v\d+, v\[\d+:\d+\], off\s*$", l)]
    tie = [i for i, l in enumerate(lines) if "the landing entry is consumed behind the first K row" in l]
    assert len(touch) == 1 and len(tie) == 1 and touch[0] < tie[0], (touch, tie)
    reg = int(re.match(r"\s+global_load_dword v(\d+)", lines[touch[0]]).group(1))
    assert any("s_waitcnt vmcnt" in l for l in lines[touch[0]:tie[0]])           # the wait for the K row stands in front of the statement
    for i in range(touch[0] + 1, tie[0]):
        if reg in _named(lines[i]):
            assert re.match(rf"\s+v_mov_b32_e32 v{reg}, 0\s*$", lines[i]) and re.match(r"\.LBB\w+:", lines[i - 1]), (hd, vat, i, lines[i])
