"""GPU: stream synthesis. The LSTM layer's continuation contract at B = 1 (kernel level), `WMEncodecModel.decode_stream` bit for bit
against `decode`, `SSR_Speech.inference_stream` against `inference`, and `inference_one_sample_stream` against
`inference_one_sample` on the tiny LM + tiny codec of tests/test_gpu_pipeline.py."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel, _device_mallocs
from ssr_speech_amd.data.tokenizer import AudioTokenizer, write_wav
from ssr_speech_amd.inference_scale import inference_one_sample, inference_one_sample_stream
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import codec as OC
import helpers_codec as H

pytestmark = pytest.mark.gpu

LSTM_TOL = 2e-5                     # tests/test_gpu_codec_kernels.py's bar for the fp32 LSTM step kernels against float64


# ----------------------------------------------------------------------------------------------- ssrhip_lstm_layer: t_begin > 0
@pytest.mark.parametrize("Cc", [128, 256])          # 128: the matrix-core step kernel; 256: the small-batch kernel
def test_lstm_layer_continues_from_the_state_the_previous_call_left(Cc):
    """One call over [0, 37) and calls over [0, 1) [1, 17) [17, 37) on the same buffers (T = the buffers' capacity) write the same bits."""
    L = _lib.lib()
    B, T = 1, 37
    g = torch.Generator().manual_seed(4000 + Cc)
    gin, skip, whh = torch.randn(B, T, 4 * Cc, generator=g), torch.randn(B, T, Cc, generator=g), H.lstm_weights(Cc, seed=Cc)
    want = H.lstm_ref(gin, whh, skip, True)
    packed = int(Cc == 128)
    w = (H.pack_whh(whh) if packed else whh).cuda().contiguous()
    dgin, dskip = gin.cuda(), skip.cuda()
    outs = []
    for windows in ([(0, T)], [(0, 1), (1, 17), (17, T)]):
        out = torch.full((B, T, Cc), float("nan"), device="cuda")
        hbuf, cbuf = torch.full((2, 16, Cc), float("nan"), device="cuda"), torch.full((B, Cc), float("nan"), device="cuda")
        for t0, t1 in windows:
            a = _lib.LstmArgs()
            a.gin, a.w_hh, a.out, a.skip = dgin.data_ptr(), w.data_ptr(), out.data_ptr(), dskip.data_ptr()
            a.hbuf, a.cbuf, a.gates = hbuf.data_ptr(), cbuf.data_ptr(), 0
            a.B, a.T, a.C = B, T, Cc
            a.gin_bstride, a.out_bstride, a.skip_bstride = T * 4 * Cc, T * Cc, T * Cc
            a.t_begin, a.t_end, a.w_packed, a.out_act = t0, t1, packed, _lib.ACT_ELU
            _lib.check(L.ssrhip_lstm_layer(C.byref(a), _lib.stream_ptr()), "ssrhip_lstm_layer")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    for o in outs:
        print(f"C={Cc}: max |kernel - fp64| = {float((o.double() - want).abs().max()):.3g}")
        torch.testing.assert_close(o.double(), want, rtol=LSTM_TOL, atol=LSTM_TOL)
    assert torch.equal(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------- decode_stream == decode
CODECS = {
    "tiny_reflect": lambda: W.CodecConfig(dimension=64, n_filters=8, ratios=(4, 3, 2, 2), bins=64, pad_mode="reflect"),
    "tiny_const": lambda: W.CodecConfig(dimension=64, n_filters=8, ratios=(4, 3, 2, 2), bins=64),
    "r8542_c128": lambda: W.CodecConfig(dimension=64, n_filters=8, ratios=(8, 5, 4, 2), bins=64),       # LSTM C = 128
    "r8542_c256": lambda: W.CodecConfig(dimension=64, n_filters=16, ratios=(8, 5, 4, 2), bins=64),      # LSTM C = 256
}
TS = (1, 2, 5, 6, 17, 61)


@functools.lru_cache(maxsize=None)
def _codec(name):
    cfg = CODECS[name]()
    sd = W.codec_state_dict(cfg, seed=7)
    return cfg, sd, WMEncodecModel(cfg, sd, "cuda")


@functools.lru_cache(maxsize=None)
def _decoded(name, T):
    """(codes [1, K, T] on the CPU, `decode` of them) — computed once per shape, never modified"""
    cfg, _, codec = _codec(name)
    codes = torch.randint(0, cfg.bins, (1, cfg.n_q, T), generator=torch.Generator().manual_seed(100 + T))
    return codes, codec.decode(codes.cuda()).clone()


def _streamed(codec, codes, push, prefix=0, max_frames=None):
    T = codes.shape[-1]
    st = codec.decode_stream(max_frames if max_frames is not None else T + 3)
    chunks = []
    if prefix:
        assert st.push(codes[..., :prefix].cuda(), emit=False).shape == (1, 1, 0)
    for t in range(prefix, T, push):
        chunks.append(st.push(codes[..., t: t + push].cuda()))
    chunks.append(st.finish())
    assert all(c.dim() == 3 and c.shape[:2] == (1, 1) and c.shape[-1] % st.hop == 0 for c in chunks)
    return torch.cat(chunks, -1), st, chunks


@pytest.mark.parametrize("push", [1, 7, 16, 10 ** 6])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", sorted(CODECS))
def test_decode_stream_is_bit_identical_to_decode(name, T, push):
    _, _, codec = _codec(name)
    codes, want = _decoded(name, T)
    got, st, chunks = _streamed(codec, codes, push)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"max |stream - decode| = {float((got - want).abs().max()):.3g}"
    if T == 61 and push == 7 and name.startswith("r8542"):
        # (the tiny codecs' 61 frames are 2928 samples: whether `decode` takes the few-output kernel for its last layer — from 4096
        # samples on — is known at finish() only, and the stream holds its windows back until then)
        assert sum(c.shape[-1] > 0 for c in chunks[:-1]) >= 3, "nothing left the stream before finish()"


def test_decode_stream_with_a_prefix_that_is_not_emitted():
    """The TTS prompt: 20 frames pass through the LSTM only; the first emitted window takes its left margin from their output."""
    _, _, codec = _codec("r8542_c128")
    codes, want = _decoded("r8542_c128", 61)
    got, st, _ = _streamed(codec, codes, 7, prefix=20)
    assert torch.equal(got, want[..., 20 * st.hop:])
    s2 = codec.decode_stream(8)
    s2.push(codes[..., :2].cuda())
    with pytest.raises(ValueError):
        s2.push(codes[..., 2:4].cuda(), emit=False)          # un-emitted frames only in front


def test_decode_stream_meets_the_oracle():
    cfg, sd, codec = _codec("r8542_c128")
    codes, _ = _decoded("r8542_c128", 61)
    got, _, _ = _streamed(codec, codes, 16)
    with torch.no_grad():
        ref = OC.decode(sd, codes, cfg)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=0, atol=5e-4)      # tests/test_gpu_pipeline.py's bound


def test_decode_stream_allocates_nothing_after_it_was_created():
    _, _, codec = _codec("r8542_c128")
    codes, want = _decoded("r8542_c128", 61)
    dcodes = codes.cuda()
    st = codec.decode_stream(64)
    n0 = _device_mallocs(codec.device)
    chunks = [st.push(dcodes[..., t: t + 7]) for t in range(0, 61, 7)] + [st.finish()]
    assert _device_mallocs(codec.device) == n0
    assert torch.equal(torch.cat(chunks, -1), want)


def test_decode_stream_refuses_what_decode_refuses():
    cfg, _, codec = _codec("tiny_const")
    st = codec.decode_stream(4)
    with pytest.raises(IndexError):
        st.push(torch.full((1, cfg.n_q, 2), cfg.bins, dtype=torch.long))
    with pytest.raises(ValueError):
        codec.decode_stream(4).push(torch.zeros(1, cfg.n_q, 5, dtype=torch.long))
    tok = AudioTokenizer(device="cuda", config=cfg, state_dict=W.codec_state_dict(cfg, seed=7))
    with pytest.raises(ValueError, match="watermark"):
        tok.decode_stream(4, use_watermark=True)


# ----------------------------------------------------------------------------------------------- inference_stream == inference
@functools.lru_cache(maxsize=None)
def _lm():
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = SSR_Speech(args)
    m.load_state_dict(W.lm_state_dict(args, seed=8))
    return args, m.to("cuda").eval()


LM_CASES = {
    "tts_greedy": dict(mi=[[40, 40]], kw=dict(top_k=1, top_p=1.0, stop_repetition=2, aug_text=True, cfg_stride=2)),
    "edit_3span_greedy": dict(mi=[[4, 9], [15, 20], [30, 36]], kw=dict(top_k=1, top_p=1.0, stop_repetition=2, aug_text=True, cfg_stride=1)),
    "tts_sampled": dict(mi=[[40, 40]], kw=dict(top_k=40, top_p=0.8, stop_repetition=2, aug_text=True, cfg_stride=2)),
    "aug_context": dict(mi=[[10, 18]], kw=dict(top_k=1, top_p=1.0, stop_repetition=2, aug_text=True, cfg_stride=2, aug_context=True)),
}


@pytest.mark.parametrize("name", sorted(LM_CASES))
def test_inference_stream_equals_inference(name):
    args, m = _lm()
    case = LM_CASES[name]
    g = torch.Generator().manual_seed(11)
    L, T, Lp, Tp = 20, 40, 7, 12
    x = torch.randint(0, args.text_vocab_size, (1, L), generator=g).cuda()
    y = torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g).cuda()
    px = torch.randint(0, args.text_vocab_size, (1, Lp), generator=g).cuda()
    py = torch.randint(0, args.audio_vocab_size, (1, Tp, 4), generator=g).cuda()
    mi = torch.LongTensor([case["mi"]]).cuda()
    call = (x, torch.LongTensor([L]).cuda(), px, torch.LongTensor([Lp]).cuda(), y, py, mi)
    torch.manual_seed(5)
    want = m.inference(*call, **case["kw"])
    rng_want, run_want = torch.get_rng_state(), dict(m.last_run)
    torch.manual_seed(5)
    it = m.inference_stream(*call, **case["kw"])
    incs = list(it)
    assert torch.equal(torch.get_rng_state(), rng_want), "the streamed run left the CPU generator elsewhere"
    got = it.result
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3]
    assert all(i.codes.device.type == "cuda" and i.codes.shape[0] == 4 for i in incs)
    assert torch.equal(torch.cat([i.codes for i in incs], 1), want[0][0])
    assert np.array_equal(np.concatenate([i.marks for i in incs]), want[1][0].numpy())
    assert all(m.last_run[k] == run_want[k] for k in ("steps", "done", "span_end", "prefill_rows"))
    if run_want["steps"] > 16:
        assert len(incs) >= 2, "every frame came out in one piece"


# ----------------------------------------------------------------------------------------------- inference_one_sample_stream
class FakePhonemizer:
    def __call__(self, texts):
        return [[c for c in t if c != " "] for t in texts]


@functools.lru_cache(maxsize=None)
def _pipeline():
    """the models of tests/test_gpu_pipeline.py::test_inference_one_sample_matches_oracle"""
    ccfg = W.CodecConfig(dimension=64, n_filters=8, ratios=(8, 5, 4, 2), bins=64)
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    lsd = W.lm_state_dict(args, seed=8)
    for k in range(4):   # a random-weight LM would emit special ids (>= vocab) that RVQ decode rejects, as in the reference: bias them away
        lsd[f"predict_layer.{k}.2.bias"][64:] = -30.0
    m = SSR_Speech(args)
    m.load_state_dict(lsd)
    return args, m.to("cuda").eval(), AudioTokenizer(device="cuda", config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=7))


def _one_sample_args(tmp_path, tts, use_watermark=False):
    args, m, tok = _pipeline()
    n_frames = 20
    wav = torch.randn(1, n_frames * 320 - 7, generator=torch.Generator().manual_seed(1)) * 0.2
    fn = str(tmp_path / "prompt.wav")
    write_wav(fn, wav, 16000)
    phn2num = {c: i for i, c in enumerate("abcdefghijklmnopqrstuvwxyz")}
    mi = torch.LongTensor([[n_frames, n_frames]]) if tts else torch.LongTensor([[6, 11]])
    decode_config = {"top_k": 1, "top_p": 1.0, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    return m, (m, argparse.Namespace(**vars(args)), phn2num, FakePhonemizer(), tok, fn, "hello world", "hello world again", mi,
               1.5, 2, True, False, use_watermark, tts, "cuda", decode_config)


@pytest.mark.parametrize("tts", [True, False])
def test_inference_one_sample_stream_equals_inference_one_sample(tmp_path, tts):
    m, call = _one_sample_args(tmp_path, tts)
    torch.manual_seed(5)
    want = inference_one_sample(*call).clone()
    steps = int(m.last_run["steps"])
    assert steps > 48, f"the run is too short ({steps} steps) to show audio leaving before it ends"
    torch.manual_seed(5)
    chunks, enqueued_at_first = [], None
    for chunk in inference_one_sample_stream(*call):
        if enqueued_at_first is None:
            enqueued_at_first = next(iter(m._engines.values()))._steps_enqueued
        assert chunk.dim() == 3 and chunk.shape[:2] == (1, 1) and chunk.shape[-1] > 0
        chunks.append(chunk)
    assert int(m.last_run["steps"]) == steps
    assert enqueued_at_first < steps, f"the first chunk came after {enqueued_at_first} of {steps} steps"
    got = torch.cat(chunks, -1)
    assert got.shape == want.shape and torch.equal(got, want), f"max |stream - one pass| = {float((got - want).abs().max()):.3g}"


def test_inference_one_sample_stream_refuses_the_watermarked_decode(tmp_path):
    _, call = _one_sample_args(tmp_path, True, use_watermark=True)
    with pytest.raises(ValueError, match="watermark"):
        next(inference_one_sample_stream(*call))
