"""GPU: the opt-in bf16 weight stream of the <= 4-row decode step (csrc/gemv_w16.hip, DESIGN.md Part I.10).

bf16 -> fp32 is a 16-bit shift and exact, and the w16 kernels run the fp32 kernels' fmaf sequence in the same order, so every comparison
between the two is `torch.equal`: launch by launch against `ssrhip_gemv` on the rounded weights, step by step between an engine that streams
the packed copies and one that streams the fp32 masters, and end to end through the public surface. The launch-level outputs are also held
against a torch fp64 product built from the UNPACKED PACKED BUFFER (a check that does not depend on the fp32 kernel), with the tolerance the
fp32 launch tests of the same shapes use in tests/test_gpu_kernels.py (3e-5: fp32, summation order only)."""
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

# (G, N, K, prologue, activation, epilogue): the six launches of the 830M step, a ragged workgroup split, S = 4
SHAPES = [
    (1, 6144, 2048, _lib.PRO_LAYERNORM, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),
    (1, 8192, 2048, _lib.PRO_LAYERNORM, _lib.ACT_RELU, _lib.EPI_STORE),
    (1, 4096, 2048, _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
    (1, 2048, 8192, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    (1, 2048, 2048, _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    (4, 2056, 1024, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_STORE),
    (1, 520, 1024, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_STORE),
    (1, 1024, 4096, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
]
# row-major activations only; K / V appended at 130, 7, 383, 256 of 3 pages; the master and its bias are drawn per case
W16 = H.Stream("w16", "w16.", None, [130, 7, 383, 256], 3, hold_fp32=False)
GROW = (4, 6)                 # prompt lengths of the engine-level tests: 9 + 4u text tokens, 21 + 6u audio frames


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_w16_launch_is_bit_identical_to_the_fp32_launch_on_the_rounded_weights(L, B, G, N, K, pro, act, epi):
    H.check_launch(L, W16, B, G, N, K, pro, act, epi)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("rows", ["offset", "step"])
def test_w16_launch_is_bit_identical_on_ill_conditioned_rows(L, B, rows):
    """LayerNorm + head-MLP1 + GELU at K = 2048 on rows with a large common offset / a step between slices (helpers_conditioning.ln_rows)"""
    G, N, K, pro, act, epi = SHAPES[2]
    H.check_launch(L, W16, B, G, N, K, pro, act, epi, x=HC.ln_rows(B, K, B)[rows])


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("partials", ["wide", "late_peak"])
def test_w16_launch_is_bit_identical_on_wide_merge_partials(L, B, partials):
    """the split-KV merge prologue with partial maxima spread over +-180 / a peak of 150 on the row's last page (helpers_conditioning.ml_cases)"""
    G, N, K, pro, act, epi = SHAPES[4]
    part_ml = HC.ml_cases(B, H.H, W16.max_pages, [300, 129, 384, 1][:B], B)[partials]     # the row lengths check_launch merges
    H.check_launch(L, W16, B, G, N, K, pro, act, epi, part_ml=part_ml)


def test_w16_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    H.check_refusal(L, W16, B=2, N=256, K=1536)


# ------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("n_utt,use_cfg", [(1, False), (1, True), (2, True)], ids=["1row", "2rows", "4rows"])
def test_w16_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena16, n_utt, use_cfg):
    H.check_engine_steps("w16", tiny2048[0], arena16, n_utt, use_cfg, GROW, masters_kw=dict(pair_mode=1), unpairs=True)


def test_w16_engine_contract(tiny2048, arena16):
    args, sd = tiny2048
    with pytest.raises(ValueError, match="<= 4-row"):
        DecodeEngine(arena16, 5, False, 256, 64, stream_w16=True)         # 5 rows
    # the C side refuses too (an engine of 5 rows exists; the packed copies are not for it)
    eng = DecodeEngine(arena16, 5, False, 256, 64)
    try:
        assert eng.stream_w16 is False
        eng._create_ctx()
        w16 = arena16.w16_struct()
        assert eng.lib.ssrhip_lm_set_w16(eng._ctx, C.byref(w16)) < 0
        assert b"<= 4-row" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(a32, 1, True, 256, 64, stream_w16=True)              # an fp32 arena has no rounded masters
    assert DecodeEngine(a32, 1, True, 256, 64).stream_w16 is False


# ------------------------------------------------------------------------------------------ public surface
def test_set_weight_dtype_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    monkeypatch.delenv("SSRHIP_GEMV_W16", raising=False)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    x, y, unc, mi = _utterance(args, 21)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    call = lambda: m.inference(x.cuda(), torch.LongTensor([x.shape[1]]), x.cuda(), torch.LongTensor([x.shape[1]]), y.cuda(), y.cuda(), mi.cuda(),
                               uncond_x=unc, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    r_fp32 = call()
    assert eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0 and m.weight_dtype == "fp32"
    m.set_weight_dtype("bf16")
    r_w16 = call()
    assert m.weight_dtype == "bf16" and eng_of().stream_w16 is True and eng_of().w16_launches_per_step == 4 * LAYERS + 2
    # the same call with the switch off: the 2-row engine streams the rounded fp32 masters (and may pair) — same res, marks, masks
    monkeypatch.setenv("SSRHIP_GEMV_W16", "0")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("bf16")                                            # the switch is read when an engine is built
    r_masters = call()
    assert eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0 and eng_of().a.weight_dtype == "bf16"
    assert _same(r_w16, r_masters)
    monkeypatch.delenv("SSRHIP_GEMV_W16")
    # a 16-row engine of the bf16 model: the matrix-core step on the rounded masters, no packed stream
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(8))]
    outs = m.inference_batch(utts, aug_text=True, group=8, seed=3, **{k: kw[k] for k in ("top_k", "top_p", "temperature", "stop_repetition", "cfg_coef", "cfg_stride")})
    assert len(outs) == 8 and eng_of().B == 16 and eng_of().stream_w16 is False and eng_of().w16_launches_per_step == 0
    # back to fp32: today's tokens, bit for bit
    m.set_weight_dtype("fp32")
    assert _same(call(), r_fp32)
    assert eng_of().a.weight_dtype == "fp32"
    with pytest.raises(ValueError):
        m.set_weight_dtype("fp8")
