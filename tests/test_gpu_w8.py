"""GPU: the opt-in e4m3 weight stream of the <= 4-row decode step (csrc/gemv_w8.hip, DESIGN.md Part I.18).

e4m3 -> fp32 is exact, the per-row scale is a power of two, and the w8 kernels run the fp32 kernels' fmaf sequence in the same order and
scale each (row, segment) partial sum where it is parked; so every comparison with the fp32 kernels on the masters codes * scale is
`torch.equal`: launch by launch against `ssrhip_gemv`, step by step between an engine that streams the codes and one that streams the fp32
masters, and end to end through the public surface. Independent of the fp32 kernel: a launch whose every output is ONE widened code times
its scale (all 254 finite codes, every lane / dword position class), and a torch fp64 product built from the UNPACKED PACKED BUFFER times
the scales, with the bound of the fp32 launch tests of the same shapes (3e-5: fp32, summation order only)."""
import ctypes as C

import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as HC
import helpers_w8 as H8
from helpers_w16 import L, arena16, tiny2048  # noqa: F401  (module-scoped fixtures)
from helpers_w16 import LAYERS, _prompts, _same, _utterance
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena, quantize_e4m3, to_w8_order
from ssr_speech_amd.models.ssr import SSR_Speech
from test_gpu_w16 import GROW, SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arena8(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="e4m3")


def test_every_code_is_widened_and_indexed_as_documented(L):
    """B = 1, N = 512, K = 1024: row n holds the finite code number n mod 254 at column (7 n) mod 1024 and zero codes elsewhere, the
    scales are 2^-(n mod 5), x is all ones, no bias: y[n] = float8_e4m3fn(code).float() * s[n], exactly. Every finite code (both zeros,
    the subnormals), and (7 n) mod 1024 visits every lane and every dword of a lane's 16 bytes."""
    N, K = 512, 1024
    n = torch.arange(N)
    col = (7 * n) % K
    assert len(set((int(c) % 256) // 4 for c in col)) == 64 and len(set(int(c) // 256 for c in col)) == 4 and len(set(int(c) % 4 for c in col)) == 4
    code = torch.tensor(H8.FINITE_CODES, dtype=torch.uint8)[n % 254]
    q = torch.zeros(N, K, dtype=torch.uint8)
    q[n, col] = code
    scale = torch.ldexp(torch.ones(N), -(n % 5)).contiguous()
    want = torch.tensor([H8.e4m3_value(int(c)) for c in code], dtype=torch.float32) * scale      # from the format's definition
    assert torch.equal(want, code.view(torch.float8_e4m3fn).float() * scale)
    master = (q.view(torch.float8_e4m3fn).float() * scale.unsqueeze(1)).cuda()
    packed, d_scale = to_w8_order(q).cuda(), scale.cuda()
    x = torch.ones(1, K, device="cuda")
    y = torch.full((N + H8.PAD,), H8.POISON, device="cuda")
    a = _lib.GemvArgs()
    a.W, a.x, a.y = master.data_ptr(), x.data_ptr(), y.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = 1, N, K, 1, K, N
    assert L.ssrhip_gemv_w8(C.byref(a), packed.data_ptr(), d_scale.data_ptr(), _lib.stream_ptr()) == 0, L.ssrhip_last_error()
    torch.cuda.synchronize()
    got = y[:N].cpu()
    bad = (got != want).nonzero().reshape(-1)
    assert bad.numel() == 0, [(int(i), int(code[i]), float(got[i]), float(want[i])) for i in bad[:6]]
    assert bool((y[N:] == H8.POISON).all())


def test_the_arena_quantises_on_the_gpu_as_on_the_cpu(tiny2048, arena8):
    """torch's float8 cast and frexp on the device give the codes and scales of the CPU (which tests/test_w8_host.py holds against a
    quantiser written without the cast)"""
    args, sd = tiny2048
    a32 = LMWeightsArena(args, {k: v.cpu() for k, v in sd.items()}, torch.device("cpu"))
    for name in ("in_proj", "ffn2"):
        q, s = quantize_e4m3(a32.layers[1][name + "_w"])
        assert torch.equal(arena8.layers[1][name + "_w8s"].cpu(), s), name
        assert torch.equal(arena8.layers[1][name + "_w"].cpu(), q.view(torch.float8_e4m3fn).float() * s.unsqueeze(1)), name
    q, s = quantize_e4m3(a32.head2_w)
    assert torch.equal(arena8.head2_w8s.cpu(), s) and torch.equal(arena8.head2_w.cpu(), q.view(torch.float8_e4m3fn).float() * s.unsqueeze(-1))


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_w8_launch_is_bit_identical_to_the_fp32_launch_on_the_masters(L, B, G, N, K, pro, act, epi):
    H8.check_launch(L, B, G, N, K, pro, act, epi)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("rows", ["offset", "step"])
def test_w8_launch_is_bit_identical_on_ill_conditioned_rows(L, B, rows):
    G, N, K, pro, act, epi = SHAPES[2]                                        # LayerNorm + head-MLP1 + GELU, K = 2048
    H8.check_launch(L, B, G, N, K, pro, act, epi, x=HC.ln_rows(B, K, B)[rows])


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("partials", ["wide", "late_peak"])
def test_w8_launch_is_bit_identical_on_wide_merge_partials(L, B, partials):
    G, N, K, pro, act, epi = SHAPES[4]                                        # split-KV merge + out-projection + residual
    part_ml = HC.ml_cases(B, H8.H, 3, [300, 129, 384, 1][:B], B)[partials]           # check_launch's pages and row lengths
    H8.check_launch(L, B, G, N, K, pro, act, epi, part_ml=part_ml)


@pytest.mark.parametrize("depth", ["0", "2", "8"])
def test_w8_launch_at_every_depth_of_the_straight_line_form(L, monkeypatch, depth):
    """SSRHIP_GEMV_W8_DEPTH is read at every call: the other two rings and the generic form on a shape the straight-line form takes by
    default (LN + FFN1 and FFN2 at 830M), same bits"""
    monkeypatch.setenv("SSRHIP_GEMV_W8_DEPTH", depth)
    for B in (1, 2, 4):
        H8.check_launch(L, B, *SHAPES[1])
        H8.check_launch(L, B, *SHAPES[3])


def test_w8_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    H8.check_refusal(L, B=2, N=256, K=1536)


# ------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("n_utt,use_cfg", [(1, False), (1, True), (2, True)], ids=["1row", "2rows", "4rows"])
def test_w8_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena8, arena16, n_utt, use_cfg):
    H8.check_engine_steps(tiny2048[0], arena8, arena16, n_utt, use_cfg, GROW)


def test_w8_engine_contract(tiny2048, arena8, arena16):
    with pytest.raises(ValueError, match="<= 4-row"):
        DecodeEngine(arena8, 5, False, 256, 64, stream_w8=True)           # 5 rows
    # the C side refuses too (an engine of 5 rows exists; the codes are not for it)
    eng = DecodeEngine(arena8, 5, False, 256, 64)
    try:
        assert eng.stream_w8 is False
        eng._create_ctx()
        arena8.ensure_w8_copies()
        w8 = arena8.w8_struct()
        assert eng.lib.ssrhip_lm_set_w8(eng._ctx, C.byref(w8)) < 0
        assert b"<= 4-row" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    # one packed stream per engine, whichever comes first
    eng = DecodeEngine(arena8, 1, True, 256, 64, stream_w8=True)
    try:
        eng._create_ctx()
        w16 = _lib.LMW16()                                                # refused before the record is read
        assert eng.lib.ssrhip_lm_set_w16(eng._ctx, C.byref(w16)) < 0 and b"e4m3" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="e4m3"):
        DecodeEngine(a32, 1, True, 256, 64, stream_w8=True)               # an fp32 arena has no codes
    with pytest.raises(ValueError, match="e4m3"):
        DecodeEngine(arena16, 1, True, 256, 64, stream_w8=True)           # nor has a bf16 arena
    with pytest.raises(ValueError, match="takes one"):
        DecodeEngine(arena8, 1, True, 256, 64, stream_w8=True, stream_w16=True)
    assert DecodeEngine(a32, 1, True, 256, 64).stream_w8 is False and DecodeEngine(arena16, 1, True, 256, 64).stream_w8 is False


def test_e4m3_prefill_through_one_plane_and_through_three_writes_the_same_kv(tiny2048, monkeypatch):
    """an e4m3 arena is bf16-valued: its prefill GEMMs take ONE plane per matrix (ssrhip_gemm_w1) by default and three under
    SSRHIP_PREFILL_W1=0; the whole poisoned KV pool and the tokens behind it are the same"""
    args, sd = tiny2048
    got = {}
    for w1 in ("1", "0"):
        monkeypatch.setenv("SSRHIP_PREFILL_W1", w1)
        arena = LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="e4m3")
        eng = DecodeEngine(arena, 1, True, 256, 64)
        try:
            assert eng.prefill_planes == (1 if w1 == "1" else 3) and eng.stream_w8 is True
            eng.kv_pool.fill_(H8.POISON)
            rows, cols, knobs = _prompts(args, 1, True, True, GROW)
            n0 = eng.lib.ssrhip_gemm_w1_launches()
            eng.start(rows, cols, knobs, noise=None)
            torch.cuda.synchronize()
            assert eng.lib.ssrhip_gemm_w1_launches() - n0 == (4 * arena.L if w1 == "1" else 0)   # launched, not the silent fp32-chain fallback
            pool = eng.kv_pool.clone()
            eng.decode(8, use_graph=True)
            torch.cuda.synchronize()
            got[w1] = (pool, eng.generated[:, :8].clone())
        finally:
            eng.close()
    assert bool((got["1"][0] != H8.POISON).any())
    assert torch.equal(got["1"][0], got["0"][0]) and torch.equal(got["1"][1], got["0"][1])


# ------------------------------------------------------------------------------------------ public surface
def test_set_weight_dtype_e4m3_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    for name in ("SSRHIP_GEMV_W8", "SSRHIP_GEMVM_W16", "SSRHIP_PREFILL_W1"):
        monkeypatch.delenv(name, raising=False)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    x, y, unc, mi = _utterance(args, 21)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    call = lambda: m.inference(x.cuda(), torch.LongTensor([x.shape[1]]), x.cuda(), torch.LongTensor([x.shape[1]]), y.cuda(), y.cuda(), mi.cuda(),
                               uncond_x=unc, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    rebuild = lambda: (m.set_weight_dtype("fp32"), m.set_weight_dtype("e4m3"))           # the switches are read when arena / engine are built
    r_fp32 = call()
    assert eng_of().stream_w8 is False and eng_of().w8_launches_per_step == 0 and m.weight_dtype == "fp32"
    m.set_weight_dtype("e4m3")
    r_w8 = call()
    e = eng_of()
    assert m.weight_dtype == "e4m3" and e.stream_w8 is True and e.w8_launches_per_step == 4 * LAYERS + 2 and e.stream_w16 is False
    assert e.a.bf16_valued and e.prefill_planes == 1 and e.pairing is False and "e4m3" in e.pairing_why
    # the same call with the switch off: the 2-row engine streams the fp32 masters (and may pair) — same res, marks, masks
    monkeypatch.setenv("SSRHIP_GEMV_W8", "0")
    rebuild()
    r_masters = call()
    assert eng_of().stream_w8 is False and eng_of().w8_launches_per_step == 0 and eng_of().a.weight_dtype == "e4m3"
    assert _same(r_w8, r_masters)
    monkeypatch.delenv("SSRHIP_GEMV_W8")
    # prefill through three planes instead of one: the same result (the KV cache itself: the test below)
    monkeypatch.setenv("SSRHIP_PREFILL_W1", "0")
    rebuild()
    r_three = call()
    assert eng_of().prefill_planes == 3 and eng_of().stream_w8 is True
    assert _same(r_w8, r_three)
    monkeypatch.delenv("SSRHIP_PREFILL_W1")
    # a 16-row engine of the e4m3 model: the matrix-core step on the masters or on their 2-byte streaming copies, same tokens
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(8))]
    bkw = {k: kw[k] for k in ("top_k", "top_p", "temperature", "stop_repetition", "cfg_coef", "cfg_stride")}
    outs = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("SSRHIP_GEMVM_W16", sw)
        rebuild()
        outs[sw] = m.inference_batch(utts, aug_text=True, group=8, seed=3, **bkw)
        e = eng_of()
        assert len(outs[sw]) == 8 and e.B == 16 and e.stream_w8 is False and e.w8_launches_per_step == 0
        assert e.stream_wt16 is (sw == "1") and e.wt16_launches_per_step == (4 * LAYERS + 2 if sw == "1" else 0)
    assert all(_same(a, b) for a, b in zip(outs["1"], outs["0"]))
    monkeypatch.delenv("SSRHIP_GEMVM_W16")
    # back to fp32: today's tokens, bit for bit
    m.set_weight_dtype("fp32")
    assert _same(call(), r_fp32)
    assert eng_of().a.weight_dtype == "fp32" and eng_of().stream_w8 is False
