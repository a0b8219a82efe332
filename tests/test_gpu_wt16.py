"""GPU: the bf16 weight stream of the 5..16-row decode step (csrc/gemv_mfma_w16.hip, DESIGN.md Part I.11).

bf16 -> fp32 is a 16-bit shift and exact, and the bf16-stream kernels run the fp32 kernels' MFMA sequence on the same launch plan, so every
comparison between the two is `torch.equal`: launch by launch against `ssrhip_gemv` on the fp32 streaming-order copy of the rounded master
(whole output buffers with a poisoned pad behind them, whole KV pools), step by step between an engine that streams the packed copies and one
that streams the masters, and end to end through the public surface. The launch-level outputs are also held against a torch fp64 product
built from the UNPACKED PACKED BUFFER (a check that does not depend on the fp32 kernel) with the bound
tests/test_gpu_kernels.py::test_gemv_mfma_rows_matches_torch applies to these kernels in fp32 (3e-5); the fp32 launch on the same inputs is
held to the same bound in the same test, so a failure of both points at the inputs and not at the new kernel."""
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
# (G, N, K, prologue, activation, epilogue): the smallest shapes that reach each code path on 256 CUs, and the step's own
SHAPES = [
    (1, 6144, 2048, LN, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),       # 3 units per workgroup: a full tile + an 8-row duplicate tile, cross-tile refill, KV append
    (1, 8192, 2048, LN, _lib.ACT_RELU, _lib.EPI_STORE),            # FFN1
    (1, 4096, 2048, LN, _lib.ACT_GELU_ERF, _lib.EPI_STORE),        # head-MLP1
    (1, 2048, 2048, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, x in registers
    (1, 2048, 8192, NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),       # pair form, streaming
    (4, 2056, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # groups, 4 waves, 257 units
    (2, 52, 1024, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # N % 8 = 4: zero-padded unit, partial 4-row store
    (1, 2064, 2112, NONE, _lib.ACT_NONE, _lib.EPI_STORE),          # plain streaming form (258 units > CUs); 132 k-steps: partial / empty wave slices
    (1, 24, 4096, LN, _lib.ACT_NONE, _lib.EPI_STORE),              # SPWX = 32 with the LayerNorm
    (1, 24, 4096, NONE, _lib.ACT_NONE, _lib.EPI_STORE),            # the streaming kernel over two 16-step groups per wave
]
KV_POS = [127, 128, 5, 255, 0, 129, 64, 126, 200, 1, 130, 254, 77, 128, 127, 3]     # both sides of the page edge at 128
WT16 = H.Stream("wt16", "wt16.", (H.to_tiled, H.from_tiled), KV_POS, 2, hold_fp32=True)
GROW = (4, 6)                 # prompt lengths of the engine-level tests: 9 + 4u text tokens, 21 + 6u audio frames


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [5, 11, 16])
@pytest.mark.parametrize("G,N,K,pro,act,epi", SHAPES)
def test_wt16_launch_is_bit_identical_to_the_fp32_launch_on_the_rounded_weights(L, B, G, N, K, pro, act, epi, tiled):
    H.check_launch(L, WT16, B, G, N, K, pro, act, epi, tiled)


@pytest.mark.parametrize("tiled", [0, 1], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B", [5, 16])
@pytest.mark.parametrize("rows", ["offset", "step"])
def test_wt16_launch_is_bit_identical_on_ill_conditioned_rows(L, B, rows, tiled):
    """LayerNorm + head-MLP1 + GELU at K = 2048 on rows with a large common offset / a step between slices (helpers_conditioning.ln_rows)"""
    G, N, K, pro, act, epi = SHAPES[2]
    H.check_launch(L, WT16, B, G, N, K, pro, act, epi, tiled, x=HC.ln_rows(B, K, B)[rows])


@pytest.mark.parametrize("N,act,epi", [(6144, _lib.ACT_NONE, _lib.EPI_QKV_APPEND), (8192, _lib.ACT_RELU, _lib.EPI_STORE)], ids=["qkv", "ffn1"])
def test_wt16_all_at_entry_form_is_bit_identical_to_the_ring_form(L, monkeypatch, N, act, epi):
    """SSRHIP_GEMVM_W16_DEPTH=16 (read at every launch): the LayerNorm launches whose workgroups own exactly two tiles (3 or 4 units on 256
    CUs) request all 16 loads of a wave at entry instead of rolling a ring of 8. Same MFMA sequence, same bits — q, the appended K / V
    rows, the FFN hidden."""
    B, K = 16, 2048
    Wt, packed, _, bias = H.shape_weights(WT16.prefix, 1, N, K)
    g = torch.Generator().manual_seed(N + 5)
    qkv = epi == _lib.EPI_QKV_APPEND
    x = H.to_tiled((torch.randn(B, K, generator=g) * 1.5 + 0.3).cuda())
    n_y = B * K if qkv else 16 * N
    table = torch.randperm(B * WT16.max_pages, generator=g).view(B, WT16.max_pages).to(torch.int32).cuda()
    pos = torch.tensor(KV_POS[:B], dtype=torch.int32).cuda()

    def run(depth):
        if depth is None:
            monkeypatch.delenv("SSRHIP_GEMVM_W16_DEPTH", raising=False)
        else:
            monkeypatch.setenv("SSRHIP_GEMVM_W16_DEPTH", depth)
        y, pool = torch.full((n_y + H.PAD,), H.POISON, device="cuda"), H.kv_pool(B, WT16.max_pages, qkv)
        a = _lib.GemvArgs()
        a.W, a.bias, a.x, a.y = Wt.data_ptr(), bias.data_ptr(), x.data_ptr(), y.data_ptr()
        a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, K if qkv else N
        a.pro, a.act, a.epi, a.ln_eps = LN, act, epi, 1e-5
        a.x_tiled, a.y_tiled, a.w_tiled = 1, 0 if qkv else 1, 1
        if qkv:
            a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), WT16.max_pages, H.N_LAYER, H.H, H.HD)
            a.layer, a.kv_pos = H.LAYER, pos.data_ptr()
        rc = L.ssrhip_gemv_wt16(C.byref(a), packed.data_ptr(), _lib.stream_ptr())
        assert rc == 0, (rc, L.ssrhip_last_error())
        torch.cuda.synchronize()
        return y, pool

    y8, pool8 = run(None)
    y16, pool16 = run("16")
    assert torch.isfinite(y8[:n_y]).all()
    assert torch.equal(y8, y16) and torch.equal(pool8, pool16)


def test_wt16_refuses_a_shape_it_does_not_take_and_launches_nothing(L):
    H.check_refusal(L, WT16, B=8, N=64, K=1040)                          # K % 16 == 0 (ssrhip_gemv takes it) but no whole quads


# ------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("n_utt,use_cfg", [(5, False), (8, True)], ids=["5rows", "16rows"])
def test_wt16_engine_steps_are_bit_identical_to_the_fp32_master_engine(tiny2048, arena16, n_utt, use_cfg):
    H.check_engine_steps("wt16", tiny2048[0], arena16, n_utt, use_cfg, GROW)


def test_wt16_engine_contract(tiny2048, arena16):
    with pytest.raises(ValueError, match="stream_w16"):
        DecodeEngine(arena16, 2, True, 256, 64, stream_wt16=True)         # 4 rows: that is stream_w16's engine
    with pytest.raises(ValueError, match="5..16"):
        DecodeEngine(arena16, 17, False, 256, 64, stream_wt16=True)       # 17 rows
    a32 = LMWeightsArena(W.lm_args_tiny(), W.lm_state_dict(W.lm_args_tiny(), seed=1, device="cuda"), torch.device("cuda"))
    with pytest.raises(ValueError, match="bf16"):
        DecodeEngine(a32, 5, False, 256, 64, stream_wt16=True)            # an fp32 arena has no rounded masters
    assert DecodeEngine(a32, 5, False, 256, 64).stream_wt16 is False
    assert DecodeEngine(arena16, 17, False, 256, 64).stream_wt16 is False  # 17..32 rows keep streaming the fp32 masters
    # the C side refuses a 2-row engine too
    arena16.ensure_wt16_copies()
    eng = DecodeEngine(arena16, 1, True, 256, 64, stream_w16=False)
    try:
        assert eng.stream_wt16 is False
        eng._create_ctx()
        wt16 = arena16.wt16_struct()
        assert eng.lib.ssrhip_lm_set_wt16(eng._ctx, C.byref(wt16)) < 0
        assert b"ssrhip_lm_set_w16" in eng.lib.ssrhip_last_error()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ public surface
def test_bf16_model_streams_wt16_through_the_public_surface(tiny2048, monkeypatch):
    args, sd = tiny2048
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5)
    # 10 ragged utterances on 8 slots: a 16-row engine whose slots are refilled as utterances end
    utts = [dict(x=u[0], y=u[1], mask_interval=u[3]) for u in (_utterance(args, 30 + i, Lt=8 + i % 3, T=12 + i) for i in range(10))]
    batch = lambda: m.inference_batch(utts, aug_text=True, group=8, seed=3, **kw)
    eng_of = lambda: next(iter(m._engines.values()))
    r_fp32 = batch()
    assert eng_of().B == 16 and eng_of().stream_wt16 is False and eng_of().wt16_launches_per_step == 0 and m.weight_dtype == "fp32"
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")                           # the switch is read when an engine is built
    m.set_weight_dtype("bf16")
    r_on = batch()
    e = eng_of()
    assert e.B == 16 and e.n_refills >= 2 and e.a.weight_dtype == "bf16"
    assert e.stream_wt16 is True and e.wt16_launches_per_step == 4 * LAYERS + 2
    assert e.stream_w16 is False and e.w16_launches_per_step == 0
    arena_on = m._arena
    assert getattr(arena_on, "_wt16_ready", False)
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "0")
    m.set_weight_dtype("fp32")
    m.set_weight_dtype("bf16")
    r_off = batch()
    assert eng_of().B == 16 and eng_of().stream_wt16 is False and eng_of().wt16_launches_per_step == 0 and eng_of().a.weight_dtype == "bf16"
    assert not getattr(m._arena, "_wt16_ready", False)                    # switched off: the packed copies are not built either
    assert len(r_on) == len(r_off) == 10
    for a, b in zip(r_on, r_off):
        assert _same(a, b)                                                # res, marks, masks and intervals
    # back to fp32: the arena (and the packed copies with it) is dropped, today's tokens come back bit for bit
    monkeypatch.setenv("SSRHIP_GEMVM_W16", "1")
    m.set_weight_dtype("fp32")
    assert m._arena is None and m._engines == {}
    r_back = batch()
    assert eng_of().stream_wt16 is False and eng_of().a.weight_dtype == "fp32" and not getattr(m._arena, "_wt16_ready", False)
    for a, b in zip(r_back, r_fp32):
        assert _same(a, b)
