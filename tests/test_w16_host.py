"""CPU: the host side of the opt-in bf16 weight stream (DESIGN.md Part I.10) — the packed layout against its index formula
(include/ssrhip.h SSRHIP_W16_INDEX), the exactness of the shift-unpack, what the arena rounds and when, the public switch, the contract
errors of `ssrhip_gemv_w16` (raised before any launch) and the command line flag."""
import ctypes as C
import re

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import W16_STREAMS, WT16_DEFAULT, WT32_DEFAULT, LMWeightsArena, resolve_w16_stream, to_w16_order, w16_streamable


def w16_index(n, k, K):
    """SSRHIP_W16_INDEX as the header documents it, on integer tensors"""
    r = k % 1024
    i, lane = r // 256, (r % 256) // 4
    return (n * (K // 1024) + k // 1024) * 1024 + (i // 2) * 512 + lane * 8 + (i % 2) * 4 + k % 4


def _header_macro():
    """the macro's own text from include/ssrhip.h, as a Python expression (C's integer `/` on non-negative operands is `//`)"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssrhip.h")).read()
    m = re.search(r"#define SSRHIP_W16_INDEX\(n, k, K\) \\\n\s*(.*)\n", src)
    assert m, "SSRHIP_W16_INDEX not found in include/ssrhip.h"
    return m.group(1).replace("(size_t)", "").replace("/", "//")


def bits_to_f32(packed_i16):
    return ((packed_i16.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)


@pytest.mark.parametrize("N,K", [(5, 1024), (3, 2048), (2, 8192)])
def test_to_w16_order_is_the_documented_index_and_unpacks_exactly(N, K):
    g = torch.Generator().manual_seed(N * K)
    Wt = torch.randn(N, K, generator=g)
    # ties of the rounding: 1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7 and goes to the EVEN one (1);
    # 1 + 3 * 2^-8 lies halfway between 1 + 2^-7 (odd) and 1 + 2^-6 (even) and goes up
    Wt[0, 0], Wt[0, 1], Wt[0, 2], Wt[0, 3] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0
    packed = to_w16_order(Wt)
    assert packed.dtype == torch.int16 and packed.shape == (N, K)
    n = torch.arange(N).view(N, 1).expand(N, K)
    k = torch.arange(K).view(1, K).expand(N, K)
    idx = w16_index(n, k, K)
    assert torch.equal(idx.reshape(-1).sort().values, torch.arange(N * K))               # a permutation of the matrix
    assert torch.equal(eval(_header_macro(), {}, dict(n=n, k=k, K=K)), idx)              # the macro says the same
    want_bits = Wt.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(packed.reshape(-1)[idx], want_bits)                               # element by element
    unpacked = bits_to_f32(packed.reshape(-1)[idx])
    assert torch.equal(unpacked, Wt.to(torch.bfloat16).float())                          # bit for bit (no NaN in the input)
    assert unpacked[0, :4].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 0.0]
    # lane l's 16-byte load j of a (row, segment) unit: the fp32 kernel's float4 #2j then #2j+1 of that lane
    u = packed.view(N, K // 1024, 2, 64, 8)
    row, s, j, lane = N - 1, K // 1024 - 1, 1, 37
    f4 = lambda i: want_bits[row, s * 1024 + i * 256 + lane * 4: s * 1024 + i * 256 + lane * 4 + 4]
    assert torch.equal(u[row, s, j, lane], torch.cat([f4(2 * j), f4(2 * j + 1)]))
    # rounded masters pack to the same bits; leading (group) dimensions are carried along
    assert torch.equal(to_w16_order(Wt.to(torch.bfloat16).float()), packed)
    assert torch.equal(to_w16_order(torch.stack([Wt, -Wt]))[1], to_w16_order(-Wt))


def test_bf16_arena_rounds_the_folded_matrices_and_nothing_else():
    """Masters = fold(W, gamma) rounded ONCE to bf16, after the fold; biases (which carry W beta in fp64), embeddings and the position
    table are untouched; a family whose inner dimension the kernels do not take has no packed copy."""
    args = W.lm_args_tiny(d_model=1024, nhead=8, layers=1, vocab=64)
    sd = W.lm_state_dict(args, seed=3)
    a32 = LMWeightsArena(args, sd, torch.device("cpu"))
    a16 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    assert a32.weight_dtype == "fp32" and a16.weight_dtype == "bf16"
    rnd = lambda t: t.to(torch.bfloat16).float()
    p = "decoder.layers.0."
    want = dict(in_proj_w=rnd(sd[p + "self_attn.in_proj_weight"] * sd[p + "norm1.weight"].unsqueeze(0)),
                out_proj_w=rnd(sd[p + "self_attn.out_proj.weight"]),
                ffn1_w=rnd(sd[p + "linear1.weight"] * sd[p + "norm2.weight"].unsqueeze(0)),
                ffn2_w=rnd(sd[p + "linear2.weight"]))
    for name, t in want.items():
        assert torch.equal(a16.layers[0][name], t), name
        assert not torch.equal(a32.layers[0][name], t), name                 # the fp32 arena keeps the unrounded values
    h1 = torch.cat([sd[f"predict_layer.{k}.0.weight"] for k in range(4)], 0) * sd["decoder.norm.weight"].unsqueeze(0)
    assert torch.equal(a16.head1_w, rnd(h1))
    assert torch.equal(a16.head2_w, rnd(torch.stack([sd[f"predict_layer.{k}.2.weight"] for k in range(4)])))
    for name in ("in_proj_b", "out_proj_b", "ffn1_b", "ffn2_b"):
        assert torch.equal(a16.layers[0][name], a32.layers[0][name]), name
    for name in ("head1_b", "head2_b", "text_emb", "audio_emb", "pe"):
        assert torch.equal(getattr(a16, name), getattr(a32, name)), name
    # packed copies: a bf16 arena only, once, and the byte count of a step follows
    with pytest.raises(ValueError):
        a32.ensure_w16_copies()
    n32, gen0 = a16.nbytes_per_step(), a16.generation
    assert n32 == a32.nbytes_per_step()
    assert a16.ensure_w16_copies() is True and a16.ensure_w16_copies() is False and a16.generation == gen0 + 1
    lay = a16.layers[0]
    for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
        assert torch.equal(lay[name + "_w16"], to_w16_order(lay[name + "_w"])), name
    assert torch.equal(a16.head1_w16, to_w16_order(a16.head1_w))
    assert a16.head2_w16 is None and not w16_streamable(a16.head2_w.shape[-1])           # K = 32: streams its master
    packed = sum(lay[n_ + "_w"].numel() for n_ in ("in_proj", "out_proj", "ffn1", "ffn2")) + a16.head1_w.numel()
    assert a16.nbytes_per_step() == n32 - 2 * packed
    w = a16.w16_struct()
    assert w.head1_w16 == a16.head1_w16.data_ptr() and not w.head2_w16 and w.ffn2_w16[0] == lay["ffn2_w16"].data_ptr()
    with pytest.raises(ValueError):
        LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="fp8")


def test_set_weight_dtype_switch():
    from ssr_speech_amd.models.ssr import SSR_Speech
    m = SSR_Speech(W.lm_args_tiny())
    assert m.weight_dtype == "fp32"
    with pytest.raises(ValueError):
        m.set_weight_dtype("fp8")
    assert m.weight_dtype == "fp32"
    m._arena = object()                                                     # stands for a built arena: the switch must drop it
    m.set_weight_dtype("bf16")
    assert m.weight_dtype == "bf16" and m._arena is None and m._engines == {}
    with pytest.raises(AttributeError):
        m.weight_dtype = "fp32"                                             # read-only
    m.set_weight_dtype("fp32")
    assert m.weight_dtype == "fp32"


def test_resolve_w16_stream_follows_the_written_rules():
    """The pure decision behind DecodeEngine's stream_w16 / stream_wt16 / stream_wt32, against the rules as DecodeEngine.__init__ documents
    them, written out here independently of the table: every row count at a range edge x both arenas x requested None / True / False x the
    switch unset / "0" / "1", for all three streams."""
    rules = dict(w16=(1, 4, "SSRHIP_GEMV_W16", "1"), wt16=(5, 16, "SSRHIP_GEMVM_W16", WT16_DEFAULT), wt32=(17, 32, "SSRHIP_GEMVM_W16", WT32_DEFAULT))
    assert [st.name for st in W16_STREAMS] == list(rules) and WT16_DEFAULT == WT32_DEFAULT == "0"
    other = dict(SSRHIP_GEMV_W16="SSRHIP_GEMVM_W16", SSRHIP_GEMVM_W16="SSRHIP_GEMV_W16")
    for st in W16_STREAMS:
        lo, hi, switch, default = rules[st.name]
        for rows in (1, 2, 4, 5, 16, 17, 32):
            for dtype in ("fp32", "bf16"):
                for value in (None, "0", "1"):
                    env = {} if value is None else {switch: value}
                    env[other[switch]] = "0" if value != "0" else "1"          # the other streams' switch is not looked at
                    case = (st.name, rows, dtype, value)
                    want = dtype == "bf16" and lo <= rows <= hi and (default if value is None else value)[:1] != "0"
                    assert resolve_w16_stream(st, rows, dtype, None, env) is want, case
                    assert resolve_w16_stream(st, rows, dtype, False, env) is False, case
                    if lo <= rows <= hi and dtype == "bf16":
                        assert resolve_w16_stream(st, rows, dtype, True, env) is True, case       # asked for: the switch is not read
                        continue
                    with pytest.raises(ValueError) as err:
                        resolve_w16_stream(st, rows, dtype, True, env)
                    msg = str(err.value)
                    assert msg.startswith("stream_" + st.name), case
                    # rows outside the range win over the dtype, and the message names the stream that takes these rows
                    if rows < lo:
                        taker = "stream_w16" if rows <= 4 else "stream_wt16"
                        assert msg.endswith(f"an engine of {rows} rows takes {taker}") and "bf16'" not in msg, (case, msg)
                    elif rows > hi:
                        assert msg.endswith(f"only (this engine has {rows} rows)") and "bf16'" not in msg, (case, msg)
                    else:
                        assert msg == f"stream_{st.name} needs an arena built with weight_dtype='bf16'", (case, msg)
    # the messages the engine's callers match on, byte for byte
    st = {s_.name: s_ for s_ in W16_STREAMS}
    for name, rows, msg in (("w16", 5, "stream_w16: the bf16 weight stream exists for the <= 4-row decode step only (this engine has 5 rows)"),
                            ("wt16", 4, "stream_wt16 is the bf16 weight stream of the 5..16-row step; an engine of 4 rows takes stream_w16"),
                            ("wt16", 17, "stream_wt16: the bf16 weight stream of the matrix-core step exists for 5..16 rows only (this engine has 17 rows)"),
                            ("wt32", 2, "stream_wt32 is the bf16 weight stream of the 17..32-row step; an engine of 2 rows takes stream_w16"),
                            ("wt32", 16, "stream_wt32 is the bf16 weight stream of the 17..32-row step; an engine of 16 rows takes stream_wt16")):
        for dtype in ("fp32", "bf16"):
            with pytest.raises(ValueError) as err:
                resolve_w16_stream(st[name], rows, dtype, True, {})
            assert str(err.value) == msg, (name, rows, dtype)


def test_gemv_w16_contract_errors_need_no_gpu():
    L = _lib.lib()
    a = _lib.GemvArgs()
    assert L.ssrhip_gemv_w16(None, 0x4000, None) < 0 and b"ssrhip_gemv_w16: null argument" in L.ssrhip_last_error()
    a.W, a.y, a.x = 0x1000, 0x2000, 0x3000                  # never dereferenced: refused before any launch
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = 2, 512, 2048, 1, 2048, 512
    assert L.ssrhip_gemv_w16(C.byref(a), None, None) < 0 and b"ssrhip_gemv_w16: null argument" in L.ssrhip_last_error()
    a.B = 3
    assert L.ssrhip_gemv_w16(C.byref(a), 0x4000, None) < 0
    assert b"ssrhip_gemv_w16" in L.ssrhip_last_error() and b"B=3" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 0 and L.ssrhip_gemv_w16_applicable(None) == 0
    a.B = 2
    assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 1
    for K in (1536, 3072, 512):                             # not 1024 * {1, 2, 4, 8}
        a.K = K
        assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 0, K
    a.K, a.pro, a.ln_w, a.ln_b = 2048, _lib.PRO_LAYERNORM, 0x5000, 0x6000              # an unfolded LayerNorm
    assert L.ssrhip_gemv_w16_applicable(C.byref(a)) == 0
    assert L.ssrhip_lm_set_w16(None, None) < 0 and b"ssrhip_lm_set_w16" in L.ssrhip_last_error()
    assert L.ssrhip_lm_w16_launches(None) == 0


def test_abi_struct_15_is_the_w16_record():
    L = _lib.lib()
    assert _lib.ABI_STRUCTS[15] is _lib.LMW16
    assert L.ssrhip_sizeof(15) == C.sizeof(_lib.LMW16) == 6 * C.sizeof(C.c_void_p)
    assert L.ssrhip_sizeof(16) == -1
    assert L.ssrhip_version() == 107                                        # additions only


def test_cli_weight_dtype_flag():
    from ssr_speech_amd import inference_v2 as cli
    assert cli.parse_args([]).weight_dtype == "fp32"
    assert cli.parse_args(["--weight_dtype", "bf16"]).weight_dtype == "bf16"
    with pytest.raises(SystemExit):
        cli.parse_args(["--weight_dtype", "fp8"])
    assert "--weight_dtype" not in [f for f, _ in cli.REFERENCE_FLAGS]
