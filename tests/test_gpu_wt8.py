"""GPU: the e4m3 weight stream of the 5..16-row decode step (csrc/gemv_mfma_w8.hip, DESIGN.md Part I.22).

A code is widened exactly and multiplied by its row's power-of-two scale before it enters the MFMA — that product is the fp32 master — and
the kernels run the fp32 kernels' MFMA sequence on the same launch plan, so every comparison between the two is `torch.equal`: launch by
launch against `ssrhip_gemv` on the fp32 streaming-order copy of code * scale (whole output buffers with a poisoned pad behind them, whole KV
pools), step by step between an engine that streams the codes, one that streams the masters and one that streams the 2-byte copies, and end
to end through the public surface. The launch-level outputs are also held against a torch fp64 product built from the UNPACKED PACKED BUFFER
TIMES THE SCALES (a check that does not depend on the fp32 kernel) with the bound the fp32 launch tests of these shapes use (3e-5); the fp32
launch on the same inputs is held to the same bound in the same test, so a failure of both points at the inputs and not at the new kernel."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as HC
import helpers_w16 as H
import helpers_wt8 as H8
from helpers_w16 import L, arena16, tiny2048  # noqa: F401  (module-scoped fixtures)
from helpers_w16 import LAYERS, _same, _utterance
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

LN, NONE = _lib.PRO_LAYERNORM, _lib.PRO_NONE
QKV = (1, 6144, 2048, LN, _lib.ACT_NONE, _lib.EPI_QKV_APPEND)         # 3 units per workgroup: a full tile + an 8-row duplicate tile, cross-tile refill, KV append
PAIR_XREG = (1, 2048, 2048, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL)   # pair form, x in registers
PAIR_STREAM = (1, 2048, 8192, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL)  # pair form, streaming
PADDED = (2, 52, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE)           # N % 8 = 4: zero-padded unit, partial 4-row store, 2 groups
# (G, N, K, prologue, activation, epilogue): the shapes of tests/test_gpu_wt16.py with every K a whole number of octets
SHAPES = [
    QKV,
    (1, 8192, 2048, LN, _lib.ACT_RELU, _lib.EPI_STORE),            # FFN1
    (1, 4096, 2048, LN, _lib.ACT_GELU_ERF, _lib.EPI_STORE),        # head-MLP1
    PAIR_XREG,
    PAIR_STREAM,
    (4, 2056, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # groups, 4 waves, 257 units
    PADDED,
    (1, 2064, 2176, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain streaming form (258 units > CUs); 136 k-steps: wave 4 holds one octet, waves 5..7 none
    (1, 24, 4096, LN, _lib.ACT_NONE, _lib.EPI_STORE),              # SPWX = 32 with the LayerNorm
    (1, 24, 4096, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # the streaming kernel over two 16-step groups per wave
    (1, 24, 1920, LN, _lib.ACT_NONE, _lib.EPI_STORE),              # x in registers, 120 k-steps: a partial last wave slice under the LayerNorm
]
KV_POS = [127, 128, 5, 255, 0, 129, 64, 126, 200, 1, 130, 254, 77, 128, 127, 3]     # both sides of the page edge at 128
GROW = (4, 6)                 # prompt lengths of the engine-level tests: 9 + 4u text tokens, 21 + 6u audio frames


@pytest.fixture(scope="module")
def arena8(tiny2048):
    args, sd = tiny2048
    return LMWeightsArena(args, sd, torch.device("cuda"), weight_dtype="e4m3")


# ------------------------------------------------------------------------------------------ 1. launch level
@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [5, 11, 16])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_wt8_launch_is_bit_identical_to_the_fp32_launch_on_code_times_scale(L, B, G, N, K, pro, act, epi, tiled):
    H8.check_launch(L, B, G, N, K, pro, act, epi, tiled, KV_POS)


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [5, 16])
@pytest.mark.parametrize("rows", ["offset", "step"])
def test_wt8_launch_is_bit_identical_on_ill_conditioned_rows(L, B, rows, tiled):
    """LayerNorm + head-MLP1 + GELU at K = 2048 on rows with a large common offset / a step between slices (helpers_conditioning.ln_rows)"""
    G, N, K, pro, act, epi = (1, 4096, 2048, LN, _lib.ACT_GELU_ERF, _lib.EPI_STORE)
    H8.check_launch(L, B, G, N, K, pro, act, epi, tiled, KV_POS, x=HC.ln_rows(B, K, B)[rows])


# ------------------------------------------------------------------------------------------ 2. scale placement
@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [5, 16])
@pytest.mark.parametrize("G,N,K,pro,act,epi", [QKV, PAIR_XREG, PAIR_STREAM, PADDED], ids=["qkv3units", "pair_xreg", "pair_stream", "n52_2groups"])
def test_wt8_every_row_meets_its_own_scale(L, B, G, N, K, pro, act, epi, tiled):
    """Row n of the raw draw is multiplied by 2^((5n mod 13) - 9) before it is quantised: every 16-row tile holds >= 8 distinct scale
    exponents (asserted where the weights are built), so a kernel that applied a neighbouring row's, the other unit's or the other group's
    scale would be off by a power of two."""
    H8.check_launch(L, B, G, N, K, pro, act, epi, tiled, KV_POS, spread=True)


# ------------------------------------------------------------------------------------------ 3. bf16 KV cache
def test_wt8_qkv_launch_appends_to_a_bf16_cache_like_the_fp32_weights_launch(L):
    B, (G, N, K, pro, act, _) = 11, QKV
    max_pages = 2
    Wf, packed, scale, _, bias = H8.shape_weights(G, N, K)
    g = torch.Generator().manual_seed(B + N)
    xbuf = H.to_tiled((torch.randn(B, K, generator=g) * 1.5 + 0.3).cuda())
    table = torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32).cuda()
    pos = torch.tensor(KV_POS[:B], dtype=torch.int32).cuda()
    pool0 = torch.full((B * max_pages + 1, H.N_LAYER, 2, H.H, _lib.PAGE, H.HD), H.POISON, dtype=torch.bfloat16, device="cuda")

    def run(use_packed):
        y, pool = torch.full((B * K + H.PAD,), H.POISON, device="cuda"), pool0.clone()
        a = H8.gemv_args(Wf, bias, xbuf, y, B, G, N, K, K, pro, act, _lib.EPI_QKV_APPEND16, 1, 0, (pool, table, max_pages, pos))
        if use_packed:
            rc = L.ssrhip_gemv_wt8(C.byref(a), packed.data_ptr(), scale.data_ptr(), _lib.stream_ptr())
            assert rc == 0, (rc, L.ssrhip_last_error())
        else:
            _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y, pool.view(torch.int16)

    y8, pool8 = run(True)
    y32, pool32 = run(False)
    assert torch.equal(y8, y32) and torch.isfinite(y8[:B * K]).all()
    assert torch.equal(pool8, pool32)                                     # the whole 2-byte pool
    assert not torch.equal(pool8, pool0.view(torch.int16))                # ... and something was appended


# ------------------------------------------------------------------------------------------ 4. refusal
def test_wt8_refuses_what_it_does_not_take_and_launches_nothing(L):
    B, N, K = 8, 64, 1088                                                 # K % 64 == 0: the bf16 stream takes it; no whole octets
    a, x, y, master = H8.check_refusal(L, B, N, K)
    assert L.ssrhip_gemv_wt16_applicable(C.byref(a)) == 1
    _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))              # the caller's fallback takes it
    torch.cuda.synchronize()
    torch.testing.assert_close(y[:B * N].view(B, N).cpu(), F.linear(x.cpu(), master.cpu()), rtol=H.TOL, atol=H.TOL)
    assert bool((y[B * N:] == H.POISON).all())
    for rows in (4, 17):                                                  # the other row ranges' launches
        H8.check_refusal(L, rows, 64, 1024)


# ------------------------------------------------------------------------------------------ 5. engine level
@pytest.mark.parametrize("n_utt,use_cfg", [(5, False), (8, True)], ids=["5rows", "16rows"])
def test_wt8_engine_steps_are_bit_identical_to_the_masters_and_the_wt16_engine(tiny2048, arena8, arena16, n_utt, use_cfg):
    H8.check_engine_steps(tiny2048[0], arena8, arena16, n_utt, use_cfg, GROW)


def test_wt8_engine_with_a_bf16_kv_cache_equals_the_masters_engine_with_the_same_cache(tiny2048, arena8):
    args = tiny2048[0]
    mk = lambda **kw: DecodeEngine(arena8, 8, True, 256, 64, debug_logits=True, kv_dtype="bf16", **kw)
    engines = dict(packed=mk(stream_wt8=True), masters=mk(stream_wt8=False, stream_wt16=False))
    try:
        out = {name: H._trace(e, args, 8, True, True, True, None, GROW) for name, e in engines.items()}
        e = engines["packed"]
        assert e.B == 16 and e.kv_dtype == "bf16" and e.kv16_launches_per_step == LAYERS and e.wt8_launches_per_step == 4 * LAYERS + 2
        assert engines["masters"].wt8_launches_per_step == 0
        for s in range(H.STEPS):
            assert torch.equal(out["packed"][0][s], out["masters"][0][s]), s
        assert torch.equal(out["packed"][1], out["masters"][1]) and out["packed"][2] == 0
    finally:
        for e in engines.values():
            e.close()


# ------------------------------------------------------------------------------------------ 6. contract
def test_wt8_engine_contract(tiny2048, arena8, arena16):
    args = tiny2048[0]
    with pytest.raises(ValueError, match="takes stream_w8"):
        DecodeEngine(arena8, 2, True, 256, 64, stream_wt8=True)           # 4 rows: that is stream_w8's engine
    with pytest.raises(ValueError, match="5..16 rows only"):
        DecodeEngine(arena8, 17, False, 256, 64, stream_wt8=True)         # 17 rows
    with pytest.raises(ValueError, match="weight_dtype='e4m3'"):
        DecodeEngine(arena16, 5, False, 256, 64, stream_wt8=True)         # a bf16 arena has no codes
    with pytest.raises(ValueError, match="an engine takes one"):
        DecodeEngine(arena8, 5, False, 256, 64, stream_wt8=True, stream_wt16=True)
    assert DecodeEngine(arena8, 5, False, 256, 64).stream_wt8 is False    # the switch is unset: off
    assert DecodeEngine(arena8, 17, False, 256, 64).stream_wt8 is False
    arena8.ensure_wt8_copies()
    rec = arena8.wt8_struct()
    # the C side refuses the other row counts and names their setter
    for n_utt, use_cfg, kw, setter in ((1, True, dict(stream_w8=False), b"ssrhip_lm_set_w8 "), (17, False, {}, b"ssrhip_lm_set_wt32")):
        eng = DecodeEngine(arena8, n_utt, use_cfg, 256, 64, **kw)
        try:
            eng._create_ctx()
            assert eng.lib.ssrhip_lm_set_wt8(eng._ctx, C.byref(rec)) < 0
            assert setter in eng.lib.ssrhip_last_error(), eng.lib.ssrhip_last_error()
            assert eng.lib.ssrhip_lm_wt8_launches(eng._ctx) == 0
        finally:
            eng.close()
    # ... and an engine of its own rows once the step is captured
    eng = DecodeEngine(arena8, 5, False, 256, 64, stream_wt8=False, stream_wt16=False)
    try:
        rows, cols, knobs = H._prompts(args, 5, False, True, GROW)
        eng.start(rows, cols, knobs)
        eng.decode(1, use_graph=True)
        torch.cuda.synchronize()
        assert eng.lib.ssrhip_lm_set_wt8(eng._ctx, C.byref(rec)) < 0
        assert b"already captured" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    # ssrhip_lm_set_w8 keeps refusing more than 4 rows and now names the setter of these rows
    eng = DecodeEngine(arena8, 5, False, 256, 64)
    try:
        eng._create_ctx()
        arena8.ensure_w8_copies()
        w8 = arena8.w8_struct()
        assert eng.lib.ssrhip_lm_set_w8(eng._ctx, C.byref(w8)) < 0
        assert b"<= 4-row" in eng.lib.ssrhip_last_error() and b"ssrhip_lm_set_wt8" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ 7. public surface
def test_e4m3_model_streams_wt8_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5)
    # 10 ragged utterances on 8 slots: a 16-row engine whose slots are refilled as utterances end
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(10))]
    batch = lambda: m.inference_batch(utts, aug_text=True, group=8, seed=3, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    monkeypatch.delenv("SSRHIP_GEMVM_W16", raising=False)
    monkeypatch.setenv("SSRHIP_GEMVM_W8", "1")                            # the switch is read when an engine is built
    m.set_weight_dtype("e4m3")
    r_on = batch()
    e = eng_of()
    assert e.B == 16 and e.n_refills >= 2 and e.a.weight_dtype == "e4m3"
    assert e.stream_wt8 is True and e.wt8_launches_per_step == 4 * LAYERS + 2
    assert e.stream_wt16 is False and e.wt16_launches_per_step == 0 and e.stream_w8 is False and e.w8_launches_per_step == 0
    assert getattr(m._arena, "_wt8_ready", False) and not getattr(m._arena, "_wt16_ready", False)
    monkeypatch.delenv("SSRHIP_GEMVM_W8")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("e4m3")
    r_off = batch()
    e = eng_of()
    assert e.B == 16 and e.stream_wt8 is False and e.wt8_launches_per_step == 0 and e.a.weight_dtype == "e4m3"
    assert not getattr(m._arena, "_wt8_ready", False)                     # unset: the packed codes are not built either
    assert len(r_on) == len(r_off) == 10
    for a, b in zip(r_on, r_off):
        assert _same(a, b)                                                # res, marks, masks and intervals
