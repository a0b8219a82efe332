"""CPU: the host side of the opt-in e4m3 weight stream (DESIGN.md Part I.18) — the quantiser against one written without torch's float8
cast, the packed layout against its index formula (include/ssrhip.h SSRHIP_W8_INDEX), what the arena quantises and keeps, the pure rule
behind DecodeEngine's stream_w8, the public switch, the command line flag and the contract errors of `ssrhip_gemv_w8` (raised before any
launch)."""
import ctypes as C
import os
import re

import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_w8 as H8
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import (BF16_VALUED, LMWeightsArena, e4m3_codes, e4m3_master, from_w8_order, quantize_e4m3, resolve_prefill_planes,
                                   resolve_w8_stream, to_w8_order, w16_streamable)


def test_the_e4m3_table_is_torchs():
    """the table the independent quantiser rounds to: 254 finite codes whose values are those of torch.float8_e4m3fn (widening is exact)"""
    codes = torch.tensor(H8.FINITE_CODES, dtype=torch.uint8)
    want = torch.tensor([H8.e4m3_value(c) for c in H8.FINITE_CODES], dtype=torch.float32)
    assert torch.equal(codes.view(torch.float8_e4m3fn).float(), want)
    assert want.abs().max() == 448.0 and H8.e4m3_value(0x01) == 2.0 ** -9 and H8.e4m3_value(0x80) == 0.0


def _rows():
    """64 x 2048: standard deviations from 3e-5 to 6, a zero row, a row whose amax has m exactly 0.875, an outlier row, a row whose codes
    are mostly subnormal (|code value| < 2^-6), and exact ties between neighbouring codes"""
    g = torch.Generator().manual_seed(8)
    Wm = torch.randn(64, 2048, generator=g) * torch.logspace(-4.5, 0.78, 64).unsqueeze(1)
    Wm[5] = 0.0
    Wm[6] = Wm[6].clamp(-0.8, 0.8)
    Wm[6, 100] = 0.875                                       # frexp(0.875) = (0.875, 0): the boundary, e = -9 and the code is 448
    Wm[7] = Wm[7].clamp(-0.8, 0.8)
    Wm[7, 100] = 0.875 * (1 + 2.0 ** -23)                    # one ulp above: e = -8
    Wm[8] *= 0.01
    Wm[8, 3] = 37.5                                          # an outlier: the rest of the row falls into the subnormal codes and to zero
    Wm[9] = torch.randn(2048, generator=g) * 2.0 ** -7
    Wm[9, 0] = 400.0                                         # e = 0: |w| < 2^-6 everywhere else, subnormal codes (steps of 2^-9)
    Wm[10, :8] = torch.tensor([17.0, 19.0, -17.0, -19.0, 2.0 ** -10, 3 * 2.0 ** -10, 0.0, -0.0])     # with amax 256 below: ties at e = 0
    Wm[10, 8] = 256.0
    Wm[10, 9:] = Wm[10, 9:].clamp(-200, 200)
    return Wm


def test_quantize_e4m3_against_a_quantiser_written_without_the_cast():
    Wm = _rows()
    codes, scale = quantize_e4m3(Wm)
    want_codes, want_scale, exps = H8.table_quantize(Wm)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32 and scale.shape == (64,)
    assert torch.equal(scale, want_scale)
    bad = (codes != want_codes).nonzero()
    assert bad.numel() == 0, (bad[:4], codes[tuple(bad[0])], want_codes[tuple(bad[0])])
    assert exps[5] == 0 and exps[6] == -9 and exps[7] == -8 and exps[9] == 0 and exps[10] == 0
    assert int(codes[6, 100]) == 0x7e and int(codes[7, 100]) == 0x76                     # 448, and 0.875 * 2^8 = 224
    assert codes[10, :8].tolist() == [0x58, 0x5a, 0xd8, 0xda, 0x00, 0x02, 0x00, 0x80]     # 17 -> 16, 19 -> 20 (even codes), 2^-10 -> 0, 3 * 2^-10 -> 2^-8
    assert not bool(((codes & 0x7f) == 0x7f).any())                                      # no NaN code
    mag = (codes & 0x7f).amax(dim=1)
    nz = Wm.abs().amax(dim=1) > 0
    assert bool((mag[nz] >= 0x76).all()) and int(mag[5]) == 0                            # every non-zero row reaches |code value| >= 224
    assert int(((codes[9] & 0x78) == 0).sum()) > 1500                                     # row 9 lives in the subnormal codes
    master = e4m3_master(codes, scale)
    assert torch.equal(master, codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(1))
    assert torch.equal(master.to(torch.bfloat16).float(), master)                        # bf16-representable
    assert torch.equal(e4m3_codes(master, scale), codes)                                 # codes come back exactly from the master
    rel = float(((master - Wm).pow(2).sum() / Wm.pow(2).sum()).sqrt())
    assert rel < 0.05, rel                                                               # coarse: a few per cent relative rms
    # leading (group) dimensions are carried along
    q2, s2 = quantize_e4m3(torch.stack([Wm, -Wm]))
    assert torch.equal(q2[0], codes) and torch.equal(s2[1], scale) and torch.equal(q2[1] ^ 0x80, codes)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 2.0 ** 100, -(2.0 ** 101)])
def test_quantize_e4m3_refuses_non_finite_and_huge_weights(bad):
    Wm = torch.randn(4, 1024, generator=torch.Generator().manual_seed(2))
    Wm[2, 77] = bad
    with pytest.raises(ValueError):
        quantize_e4m3(Wm)
    args = W.lm_args_tiny(d_model=1024, nhead=8, layers=1, vocab=64)
    sd = dict(W.lm_state_dict(args, seed=3))
    sd["decoder.layers.0.linear2.weight"] = sd["decoder.layers.0.linear2.weight"].clone()
    sd["decoder.layers.0.linear2.weight"][1, 1] = bad
    with pytest.raises(ValueError):
        LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="e4m3")
    quantize_e4m3(torch.full((1, 1024), 2.0 ** 99))                                      # the largest magnitudes that pass


def _header_macro():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssrhip.h")).read()
    m = re.search(r"#define SSRHIP_W8_INDEX\(n, k, K\) \\\n\s*(.*)\n", src)
    assert m, "SSRHIP_W8_INDEX not found in include/ssrhip.h"
    return m.group(1).replace("(size_t)", "").replace("/", "//")


@pytest.mark.parametrize("N,K", [(5, 1024), (3, 2048), (2, 8192)])
def test_to_w8_order_is_the_documented_index_and_has_an_inverse(N, K):
    q = torch.randint(0, 256, (N, K), generator=torch.Generator().manual_seed(N * K), dtype=torch.uint8)
    packed = to_w8_order(q)
    assert packed.dtype == torch.uint8 and packed.shape == (N, K)
    n = torch.arange(N).view(N, 1).expand(N, K)
    k = torch.arange(K).view(1, K).expand(N, K)
    idx = H8.w8_index(n, k, K)
    assert torch.equal(idx.reshape(-1).sort().values, torch.arange(N * K))               # a permutation of the matrix
    assert torch.equal(eval(_header_macro(), {}, dict(n=n, k=k, K=K)), idx)              # the macro says the same
    assert torch.equal(packed.reshape(-1)[idx], q)                                       # every (n, k)
    assert torch.equal(from_w8_order(packed), q)
    # lane l's 16 bytes of a (row, segment) unit: the fp32 kernel's four float4 of that lane, in order
    u = packed.view(N, K // 1024, 64, 16)
    row, s, lane = N - 1, K // 1024 - 1, 37
    f4 = lambda i: q[row, s * 1024 + i * 256 + lane * 4: s * 1024 + i * 256 + lane * 4 + 4]
    assert torch.equal(u[row, s, lane], torch.cat([f4(0), f4(1), f4(2), f4(3)]))
    assert torch.equal(to_w8_order(torch.stack([q, q ^ 1]))[1], to_w8_order(q ^ 1))      # leading dimensions are carried along


def test_e4m3_arena_quantises_the_folded_matrices_and_nothing_else():
    args = W.lm_args_tiny(d_model=1024, nhead=8, layers=1, vocab=64)
    sd = W.lm_state_dict(args, seed=3)
    a32 = LMWeightsArena(args, sd, torch.device("cpu"))
    a16 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    a8 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="e4m3")
    assert a8.weight_dtype == "e4m3" and (a32.bf16_valued, a16.bf16_valued, a8.bf16_valued) == (False, True, True) and BF16_VALUED == ("bf16", "e4m3")
    lay = a8.layers[0]
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        codes, scale, _ = H8.table_quantize(a32.layers[0][name + "_w"])                  # after the fold: what the fp32 arena holds
        assert torch.equal(lay[name + "_w8s"], scale), name
        assert torch.equal(lay[name + "_w"], codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(1)), name
        assert torch.equal(lay[name + "_w"].to(torch.bfloat16).float(), lay[name + "_w"]), name
        assert torch.equal(lay[name + "_b"], a32.layers[0][name + "_b"]), name           # W beta from the unrounded weights
    q1, s1 = quantize_e4m3(a32.head1_w)
    q2, s2 = quantize_e4m3(a32.head2_w)
    assert torch.equal(a8.head1_w, e4m3_master(q1, s1)) and torch.equal(a8.head1_w8s, s1)
    assert torch.equal(a8.head2_w, e4m3_master(q2, s2)) and a8.head2_w8s.shape == a32.head2_w.shape[:2]      # one scale per row of each group
    assert torch.equal(s2[2], H8.table_quantize(a32.head2_w[2])[1])
    for name in ("head1_b", "head2_b", "text_emb", "audio_emb", "pe"):
        assert torch.equal(getattr(a8, name), getattr(a32, name)), name
    # packed codes: an e4m3 arena only, once, and the byte count of a step follows
    for other in (a32, a16):
        with pytest.raises(ValueError):
            other.ensure_w8_copies()
    n32, gen0 = a8.nbytes_per_step(), a8.generation
    assert n32 == a32.nbytes_per_step()
    assert a8.ensure_w8_copies() is True and a8.ensure_w8_copies() is False and a8.generation == gen0 + 1
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        assert torch.equal(from_w8_order(lay[name + "_w8"]), H8.table_quantize(a32.layers[0][name + "_w"])[0]), name
    assert torch.equal(a8.head1_w8, to_w8_order(q1))
    assert a8.head2_w8 is None and not w16_streamable(a8.head2_w.shape[-1])              # K = 32: streams its master
    fams = [lay[n_ + "_w"] for n_ in ("in_proj", "out_proj", "ffn1", "ffn2")] + [a8.head1_w]
    assert a8.nbytes_per_step() == n32 - sum(3 * t.numel() - 4 * t.shape[0] for t in fams)   # 1 byte per weight, one fp32 scale per row
    w = a8.w8_struct()
    assert C.sizeof(w) == 12 * C.sizeof(C.c_void_p)
    assert w.head1_w8 == a8.head1_w8.data_ptr() and w.head1_s == a8.head1_w8s.data_ptr() and not w.head2_w8 and not w.head2_s
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        assert getattr(w, name + "_w8")[0] == lay[name + "_w8"].data_ptr() and getattr(w, name + "_s")[0] == lay[name + "_w8s"].data_ptr(), name
    # a family the kernels do not take: NULL codes AND scales
    argsb = W.lm_args_tiny()                                                              # d_model 128
    ab = LMWeightsArena(argsb, W.lm_state_dict(argsb, seed=1), torch.device("cpu"), weight_dtype="e4m3")
    ab.ensure_w8_copies()
    wb = ab.w8_struct()
    assert not any(bool(getattr(wb, f)) for f, _ in _lib.LMW8._fields_) and ab.nbytes_per_step() == LMWeightsArena(
        argsb, W.lm_state_dict(argsb, seed=1), torch.device("cpu")).nbytes_per_step()


def test_resolve_w8_stream_follows_the_written_rules():
    for rows in (1, 2, 4, 5):
        for dtype in ("fp32", "bf16", "e4m3"):
            for value in (None, "0", "1"):
                env = {"SSRHIP_GEMV_W16": "0" if value != "0" else "1"}                  # another stream's switch is not looked at
                if value is not None:
                    env["SSRHIP_GEMV_W8"] = value
                case = (rows, dtype, value)
                want = dtype == "e4m3" and rows <= 4 and value != "0"
                assert resolve_w8_stream(rows, dtype, None, env) is want, case
                assert resolve_w8_stream(rows, dtype, False, env) is False, case
                if rows <= 4 and dtype == "e4m3":
                    assert resolve_w8_stream(rows, dtype, True, env) is True, case       # asked for: the switch is not read
                    continue
                with pytest.raises(ValueError) as err:
                    resolve_w8_stream(rows, dtype, True, env)
                if rows > 4:                                                             # the rows win over the dtype
                    assert str(err.value) == f"stream_w8: the e4m3 weight stream exists for the <= 4-row decode step only (this engine has {rows} rows)", case
                else:
                    assert str(err.value) == "stream_w8 needs an arena built with weight_dtype='e4m3'", case
    assert resolve_w8_stream(2, "e4m3", None, {"SSRHIP_GEMV_W8": "01"}) is False         # "starts with '0'"


def test_an_e4m3_arena_takes_the_rules_made_for_bf16_masters():
    for env, want in (({}, 1), ({"SSRHIP_PREFILL_W1": "0"}, 3), ({"SSRHIP_PREFILL_W1": "1"}, 1), ({"SSRHIP_PREFILL_SPLIT": "0"}, 0)):
        assert resolve_prefill_planes("e4m3", None, env) == want == resolve_prefill_planes("bf16", None, env), env
    assert resolve_prefill_planes("e4m3", 1, {}) == 1 and resolve_prefill_planes("e4m3", 3, {}) == 3
    with pytest.raises(ValueError):
        resolve_prefill_planes("fp32", 1, {})
    args = W.lm_args_tiny(d_model=1024, nhead=8, layers=1, vocab=64)
    a8 = LMWeightsArena(args, W.lm_state_dict(args, seed=3), torch.device("cpu"), weight_dtype="e4m3")
    assert a8.ensure_wt16_copies() is True                                               # the 2-byte streaming copies of the 5..32-row step
    from ssr_speech_amd.engine import from_wt16_order
    assert torch.equal(from_wt16_order(a8.layers[0]["ffn1_wt16"], a8.layers[0]["ffn1_w"].shape[0]), a8.layers[0]["ffn1_w"])   # exact: bf16-valued


def test_set_weight_dtype_e4m3_switch():
    from ssr_speech_amd.models.ssr import SSR_Speech
    m = SSR_Speech(W.lm_args_tiny())
    m._arena, m._engines = object(), {}
    m.set_weight_dtype("e4m3")
    assert m.weight_dtype == "e4m3" and m._arena is None and m._engines == {}
    m._arena = object()
    m.set_weight_dtype("e4m3")                                                           # no change: nothing is dropped
    assert m._arena is not None
    m.set_weight_dtype("fp32")
    assert m.weight_dtype == "fp32" and m._arena is None


def test_cli_weight_dtype_takes_e4m3():
    from ssr_speech_amd import inference_v2 as cli
    assert cli.parse_args(["--weight_dtype", "e4m3"]).weight_dtype == "e4m3"
    assert cli.parse_args([]).weight_dtype == "fp32"


def test_gemv_w8_contract_errors_need_no_gpu():
    L = _lib.lib()
    a = _lib.GemvArgs()
    assert L.ssrhip_gemv_w8(None, 0x4000, 0x5000, None) < 0 and b"ssrhip_gemv_w8: null argument" in L.ssrhip_last_error()
    a.W, a.y, a.x = 0x1000, 0x2000, 0x3000                  # never dereferenced: refused before any launch
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = 2, 512, 2048, 1, 2048, 512
    assert L.ssrhip_gemv_w8(C.byref(a), None, 0x5000, None) < 0 and b"ssrhip_gemv_w8: null argument" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_w8(C.byref(a), 0x4000, None, None) < 0 and b"ssrhip_gemv_w8: null argument" in L.ssrhip_last_error()
    a.B = 3
    assert L.ssrhip_gemv_w8(C.byref(a), 0x4000, 0x5000, None) < 0
    assert b"ssrhip_gemv_w8" in L.ssrhip_last_error() and b"B=3" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 0 and L.ssrhip_gemv_w8_applicable(None) == 0
    a.B = 2
    assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 1
    for K in (1536, 3072, 512):                             # not 1024 * {1, 2, 4, 8}
        a.K = K
        assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 0, K
    a.K = 1536
    assert L.ssrhip_gemv_w8(C.byref(a), 0x4000, 0x5000, None) == 1                       # does not qualify: answered before any launch
    a.K, a.pro, a.ln_w, a.ln_b = 2048, _lib.PRO_LAYERNORM, 0x5000, 0x6000                # an unfolded LayerNorm
    assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 0
    assert L.ssrhip_lm_set_w8(None, None) < 0 and b"ssrhip_lm_set_w8" in L.ssrhip_last_error()
    assert L.ssrhip_lm_w8_launches(None) == 0


def test_the_w8_record_reports_its_size_through_its_own_call():
    L = _lib.lib()
    assert L.ssrhip_lm_w8_sizeof() == C.sizeof(_lib.LMW8) == 12 * C.sizeof(C.c_void_p)
    assert _lib.LMW8 not in _lib.ABI_STRUCTS and L.ssrhip_sizeof(16) == -1
    assert L.ssrhip_version() == 107                                                     # additions only
