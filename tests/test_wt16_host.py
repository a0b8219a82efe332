"""CPU: the host side of the bf16 weight stream of the 5..16-row decode step (DESIGN.md Part I.11) — the packed layout against its index
formula (include/ssrhip.h SSRHIP_WT16_INDEX) element by element, the exact unpack, which inner dimensions get a packed copy, what the arena
builds, and the answers `ssrhip_gemv_wt16` gives before any launch."""
import ctypes as C
import os
import re

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from helpers_w16 import fake_gemv_args
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import LMWeightsArena, from_wt16_order, to_streaming_order, to_wt16_order, wt16_streamable


def wt16_index(n, k, K):
    """SSRHIP_WT16_INDEX as the header documents it in words: n = 8u + c, k = 64q + 16j + 4ks + e, h = j % 2, g = j / 2"""
    u, c = n // 8, n % 8
    q, j, ks, e = k // 64, (k % 64) // 16, (k % 16) // 4, k % 4
    h, g = j % 2, j // 2
    return ((u * (K // 64) + q) * 2 + h) * 256 + (ks * 8 + c) * 8 + g * 4 + e


def _header_macro():
    """the macro's own text from include/ssrhip.h, as a Python expression (C's integer `/` on non-negative operands is `//`)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssrhip.h")).read()
    m = re.search(r"#define SSRHIP_WT16_INDEX\(n, k, K\) \\\n\s*(.*)\n", src)
    assert m, "SSRHIP_WT16_INDEX not found in include/ssrhip.h"
    return m.group(1).replace("(size_t)", "").replace("/", "//")


def test_to_wt16_order_is_the_documented_index_element_by_element():
    G, N, K = 2, 20, 192                                                       # ragged: 3 units, the last with 4 real rows; 3 quads
    g = torch.Generator().manual_seed(7)
    master = torch.randn(G, N, K, generator=g).to(torch.bfloat16).float()      # a rounded master
    packed = to_wt16_order(master)
    U = (N + 7) // 8
    assert packed.dtype == torch.int16 and packed.shape == (G, U * 8, K)
    want_bits = master.to(torch.bfloat16).view(torch.int16)
    flat = packed.reshape(G, -1)
    hits = torch.zeros(U * 8 * K, dtype=torch.int32)
    macro = _header_macro()
    for n in range(U * 8):
        for k in range(K):
            i = wt16_index(n, k, K)
            assert i == eval(macro, {}, dict(n=n, k=k, K=K)), (n, k)           # the macro says the same
            hits[i] += 1
            for grp in range(G):
                assert int(flat[grp, i]) == (int(want_bits[grp, n, k]) if n < N else 0), (grp, n, k)   # the padded rows are zero
    assert bool((hits == 1).all())                                             # every slot is written exactly once
    # the unpack helper (inverse permute plus << 16) returns the rounded master exactly
    assert torch.equal(from_wt16_order(packed, N), master)
    # unrounded input is rounded to nearest even on the way; a group dimension is carried along
    raw = torch.randn(N, K, generator=g)
    assert torch.equal(from_wt16_order(to_wt16_order(raw), N), raw.to(torch.bfloat16).float())
    assert torch.equal(to_wt16_order(torch.stack([raw, -raw]))[1], to_wt16_order(-raw))


def test_wt16_blocks_are_what_the_two_kernel_forms_load():
    """Block (u, q, h), piece ks*8 + c = the four weights of k-step 4q + h, then the four of k-step 4q + h + 2 — the same 16-float k-steps
    the fp32 streaming order (SSRHIP_WTILED_INDEX) keeps in its 512-byte blocks."""
    N, K = 16, 128
    master = torch.randn(N, K, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).float()
    p16 = from_bits(to_wt16_order(master)).view(N // 8, K // 64, 2, 32, 2, 4)          # [u][q][h][piece][g][e]
    p32 = to_streaming_order(master).view(N // 8, K // 16, 32, 4)                      # [u][k-step][piece][e]
    for q in range(K // 64):
        for h in range(2):
            for g in range(2):
                assert torch.equal(p16[:, q, h, :, g], p32[:, 4 * q + h + 2 * g])


def from_bits(packed_i16):
    return ((packed_i16.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)


def test_wt16_streamable():
    assert all(wt16_streamable(K) for K in (64, 128, 1024, 2048, 2112, 4096, 8192))
    assert not any(wt16_streamable(K) for K in (0, 16, 32, 48, 1040, 2064))


def test_bf16_arena_builds_the_wt16_copies_once():
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=1, vocab=64)
    sd = W.lm_state_dict(args, seed=3)
    a32 = LMWeightsArena(args, sd, torch.device("cpu"))
    a16 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    with pytest.raises(ValueError):
        a32.ensure_wt16_copies()
    n32, gen0 = a16.nbytes_per_step(), a16.generation
    assert a16.ensure_wt16_copies() is True and a16.ensure_wt16_copies() is False and a16.generation == gen0 + 1
    lay = a16.layers[0]
    packed = 0
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        assert torch.equal(lay[name + "_wt16"], to_wt16_order(lay[name + "_w"])), name
        assert torch.equal(from_wt16_order(lay[name + "_wt16"], lay[name + "_w"].shape[0]), lay[name + "_w"]), name
        packed += lay[name + "_w"].numel()
    assert torch.equal(a16.head1_wt16, to_wt16_order(a16.head1_w))
    packed += a16.head1_w.numel()
    assert a16.head2_w.shape[-1] == 32 and a16.head2_wt16 is None              # K = 32 is no whole quad: streams its fp32 copy
    assert a16.nbytes_per_step() == n32 - 2 * packed                          # the 2-byte copies, the fp32 count skips them
    w = a16.wt16_struct()
    assert w.head1_w16 == a16.head1_wt16.data_ptr() and not w.head2_w16 and w.ffn2_w16[0] == lay["ffn2_wt16"].data_ptr()


def _fake_args(B=8, **kw):
    return fake_gemv_args(B, **kw)


def test_gemv_wt16_refusals_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_gemv_wt16(None, 0x4000, None) < 0 and b"ssrhip_gemv_wt16: null argument" in L.ssrhip_last_error()
    a = _fake_args()
    assert L.ssrhip_gemv_wt16(C.byref(a), None, None) < 0 and b"ssrhip_gemv_wt16: null argument" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_wt16_applicable(None) == 0
    for kw in (dict(B=4), dict(B=17), dict(w_tiled=0), dict(K=1040)):
        a = _fake_args(**kw)
        assert L.ssrhip_gemv_wt16(C.byref(a), 0x4000, None) == 1, kw          # does not qualify, nothing launched
        assert L.ssrhip_gemv_wt16_applicable(C.byref(a)) == 0, kw
    assert L.ssrhip_lm_wt16_launches(None) == 0
    assert L.ssrhip_lm_set_wt16(None, None) < 0 and b"ssrhip_lm_set_wt16" in L.ssrhip_last_error()
    assert L.ssrhip_version() == 107 and L.ssrhip_sizeof(16) == -1            # additions only, the record is ssrhip_lm_w16
