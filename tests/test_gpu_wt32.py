"""GPU: the bf16 weight stream of the 17..32-row decode step (csrc/gemv_mfma32_w16.hip, DESIGN.md Part I.12).

bf16 -> fp32 is a 16-bit shift and exact, and the bf16-stream kernels run the two-panel fp32 kernels' MFMA sequence on the same launch plan,
so every comparison between the two is `torch.equal`: launch by launch against `ssrhip_gemv` at the same row count on the fp32
streaming-order copy of the rounded master (whole output buffers with a poisoned pad behind them, whole KV pools), step by step between an
engine that streams the packed copies and one that streams the masters, and end to end through the public surface. The launch-level
outputs are also held against a torch fp64 product built from the UNPACKED PACKED BUFFER (a check that does not depend on the fp32 kernel)
with the bound tests/test_gpu_kernels.py::test_gemv_mfma_rows_matches_torch and tests/test_gpu_rows32.py apply to these kernels in fp32
(3e-5); the fp32 launch on the same inputs is held to the same bound in the same test, so a failure of both points at the inputs and not at
the new kernel."""
import ctypes as C

import pytest
import torch

import ssr_speech_amd  # noqa: F401
import helpers_conditioning as HC
import helpers_w16 as H
from helpers_w16 import L, arena16, tiny2048  # noqa: F401  (module-scoped fixtures)
from helpers_w16 import LAYERS, _same, _utterance
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeEngine, LMWeightsArena
from ssr_speech_amd.models.ssr import SSR_Speech

pytestmark = pytest.mark.gpu

LN, NONE = _lib.PRO_LAYERNORM, _lib.PRO_NONE
# (G, N, K, prologue, activation, epilogue): the shapes of tests/test_gpu_wt16.py that 17..32 rows take (no LayerNorm beyond K = 2048) —
# the smallest that reach each kernel form on 256 CUs, and the step's own
SHAPES = [
    (1, 6144, 2048, LN, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),       # 3 units per workgroup: a full tile + an 8-row duplicate tile, cross-tile refill, KV append
    (1, 8192, 2048, LN, _lib.ACT_RELU, _lib.EPI_STORE),            # FFN1
    (1, 4096, 2048, LN, _lib.ACT_GELU_ERF, _lib.EPI_STORE),        # head-MLP1
    (1, 2048, 2048, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, x in registers
    (1, 2048, 8192, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, streaming
    (4, 2056, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain form without prologue: groups, 4 waves, 257 units
    (2, 52, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # N % 8 = 4: zero-padded unit, partial 4-row store
    (1, 2064, 2112, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain streaming form (258 units > CUs); 132 k-steps: partial / empty wave slices
    (1, 24, 4096, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # the streaming pair form over two 16-step groups per wave
]
KV_POS = [127, 128, 5, 255, 0, 129, 64, 126, 200, 1, 130, 254, 77, 128, 127, 3,
          128, 127, 129, 0, 255, 126, 31, 128, 2, 127, 199, 254, 130, 65, 127, 128]


WT32 = H.Stream("wt32", "wt32.", (H.to_panels, H.from_panels), KV_POS, 2, hold_fp32=True)
GROW = (2, 3)                 # prompt lengths of the engine-level tests: 9 + 2u text tokens, 21 + 3u audio frames


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "paneled"])
@pytest.mark.parametrize("B", [17, 27, 32])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_wt32_launch_is_bit_identical_to_the_fp32_launch_on_the_rounded_weights(L, B, G, N, K, pro, act, epi, tiled):
    H.check_launch(L, WT32, B, G, N, K, pro, act, epi, tiled)


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [17, 32])
@pytest.mark.parametrize("rows", ["offset", "step"])
def test_wt32_launch_is_bit_identical_on_ill_conditioned_rows(L, B, rows, tiled):
    """LayerNorm + head-MLP1 + GELU at K = 2048 on rows with a large common offset / a step between slices (helpers_conditioning.ln_rows)"""
    G, N, K, pro, act, epi = SHAPES[2]
    H.check_launch(L, WT32, B, G, N, K, pro, act, epi, tiled, x=HC.ln_rows(B, K, B)[rows])


def test_wt32_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    H.check_refusal(L, WT32, B=32, N=64, K=1040)                          # K % 16 == 0 (ssrhip_gemv takes it) but no whole quads


# ------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("n_utt,use_cfg", [(17, False), (16, True)], ids=["17rows", "32rows"])
def test_wt32_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena16, n_utt, use_cfg):
    H.check_engine_steps("wt32", tiny2048[0], arena16, n_utt, use_cfg, GROW)


def test_wt32_engine_contract(tiny2048, arena16, monkeypatch):
    monkeypatch.delenv("SSRHIP_GEMVM_W16", raising=False)
    with pytest.raises(ValueError, match="stream_w16"):
        DecodeEngine(arena16, 2, True, 256, 64, stream_wt32=True)         # 4 rows: that is stream_w16's engine
    with pytest.raises(ValueError, match="stream_wt16"):
        DecodeEngine(arena16, 8, True, 256, 64, stream_wt32=True)         # 16 rows: stream_wt16's
    with pytest.raises(ValueError, match="5..16"):
        DecodeEngine(arena16, 17, False, 256, 64, stream_wt16=True)       # and stream_wt16 keeps refusing 17 rows
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(a32, 17, False, 256, 64, stream_wt32=True)           # an fp32 arena has no rounded masters
    assert DecodeEngine(a32, 17, False, 256, 64).stream_wt32 is False
    assert DecodeEngine(arena16, 17, False, 256, 64).stream_wt32 is False  # the variable unset: WT32_DEFAULT = "0"
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")
    assert DecodeEngine(arena16, 17, False, 256, 64).stream_wt32 is True
    # the C side refuses a 16-row engine and names its setter
    eng = DecodeEngine(arena16, 8, True, 256, 64, stream_wt16=False)
    try:
        assert eng.stream_wt32 is False and eng.stream_wt16 is False
        eng._create_ctx()
        wt16 = arena16.wt16_struct()
        assert eng.lib.ssrhip_lm_set_wt32(eng._ctx, C.byref(wt16)) < 0
        assert b"ssrhip_lm_set_wt16" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
def test_bf16_model_streams_wt32_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5)
    # 20 ragged utterances on 16 slots: a 32-row engine whose slots are refilled as utterances end
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(20))]
    batch = lambda: m.inference_batch(utts, aug_text=True, group=16, seed=3, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    monkeypatch.delenv("SSRHIP_GEMVM_W16", raising=False)
    r_fp32 = batch()
    assert eng_of().B == 32 and eng_of().stream_wt32 is False and eng_of().wt32_launches_per_step == 0 and m.weight_dtype == "fp32"
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")                           # the switch is read when an engine is built
    m.set_weight_dtype("bf16")
    r_on = batch()
    e = eng_of()
    assert e.B == 32 and e.n_refills >= 2 and e.a.weight_dtype == "bf16"
    assert e.stream_wt32 is True and e.wt32_launches_per_step == 4 * LAYERS + 2
    assert e.stream_wt16 is False and e.wt16_launches_per_step == 0 and e.stream_w16 is False and e.w16_launches_per_step == 0
    assert getattr(m._arena, "_wt16_ready", False)
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "0")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("bf16")
    r_off = batch()
    assert eng_of().B == 32 and eng_of().stream_wt32 is False and eng_of().wt32_launches_per_step == 0 and eng_of().a.weight_dtype == "bf16"
    assert not getattr(m._arena, "_wt16_ready", False)                    # switched off: the packed copies are not built either
    assert len(r_on) == len(r_off) == 20
    for a, b in zip(r_on, r_off):
        assert _same(a, b)                                                # res, marks, masks and intervals
    # back to fp32: the arena (and the packed copies with it) is dropped, today's tokens come back bit for bit
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")
    m.set_weight_dtype("fp32")
    assert m._arena is None and m._engines == {}
    r_back = batch()
    assert eng_of().stream_wt32 is False and eng_of().a.weight_dtype == "fp32" and not getattr(m._arena, "_wt16_ready", False)
    for a, b in zip(r_back, r_fp32):
        assert _same(a, b)
