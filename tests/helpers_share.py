"""Shared by the tests of prompt sharing (DESIGN.md Part I.15; tests/test_share_host.py, tests/test_gpu_share.py): launch arguments whose
pointers are never dereferenced, utterances with a prompt of a chosen length, and the inputs of N samples of ONE utterance."""
import ctypes as C
import math

from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd.engine import DecodeKnobs, pack_prefill_rows

from helpers_w16 import _utterance


def fake_attn_args(R, max_pages=4, hd=64, out_tiled=0):
    """ssrhip_attn_args for the host tests: every call made with them is answered before any HIP call"""
    a = _lib.AttnArgs()
    a.q, a.q_stride = 0x1000, 0
    a.kv = _lib.KV(0x2000, 0x3000, max_pages, 1, 2, hd)
    a.layer, a.row_seq, a.row_len = 0, 0, 0x4000
    a.R, a.max_splits, a.scale, a.out_tiled = R, max_pages, 1.0 / math.sqrt(hd), out_tiled
    return a


def fake_engine(L, B, max_pages=4):
    """An `ssrhip_lm` over fake pointers (d_model 128, 2 heads, 2 layers): `ssrhip_lm_create` makes no HIP call unless B == 2, the setters
    only look at the records, and `ssrhip_lm_destroy` of an engine that never stepped frees host memory only. Never step it."""
    d = _lib.LMDims(128, 2, 2, 512, 4, 64, 64, 32, max_pages * _lib.PAGE, 1)
    layer = (C.c_void_p * 2)(0x10000, 0x20000)
    w = _lib.LMWeights()
    for name in ("ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln2_w", "ln2_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b"):
        setattr(w, name, C.cast(layer, C.POINTER(C.c_void_p)))
    b = _lib.LMBuffers()
    b.B, b.n_utt, b.max_splits, b.pair_mode = B, max(B // 2, 1), max_pages, 1
    b.kv = _lib.KV(0x2000, 0x3000, max_pages, 2, 2, 64)
    ctx = C.c_void_p()
    _lib.check(L.ssrhip_lm_create(C.byref(d), C.byref(w), C.byref(b), C.byref(ctx)), "ssrhip_lm_create")
    return ctx


def prompt_len(args, seed, Lt, T):
    """the sequence length the prefill of `_utterance(args, seed, Lt, T)` leaves (text + laid-out audio columns)"""
    x, y, _, mi = _utterance(args, seed, Lt, T)
    cated = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)[0]
    return int(pack_prefill_rows([(0, x[0].numpy(), cated)], args.n_codebooks)["lens"][0])


def utterance_of_len(args, seed, n, Lt=40):
    """(Lt, T) of an utterance whose prompt is exactly n positions long (the length is linear in T)"""
    T = 18 + n - prompt_len(args, seed, Lt, 18)
    assert T > 0 and prompt_len(args, seed, Lt, T) == n, (n, T)
    return Lt, T


def sample_inputs(args, seed, n_samples, Lt=10, T=18, own_uncond=True):
    """(text rows, audio columns, knobs) of DecodeEngine.start for n_samples samples of utterance `seed` under CFG: the conditional rows
    (0, 2, 4, ...) are equal; own_uncond: every sample's unconditional row has its own text (what `aug_text` draws), else they are equal
    too. Greedy, so every sample decodes what the utterance decodes alone."""
    x, y, unc, mi = _utterance(args, seed, Lt, T)
    cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)
    rows, cols, knobs = [], [], []
    for i in range(n_samples):
        u = unc[0].numpy().copy()
        if own_uncond:
            u[0] = (int(u[0]) % args.text_vocab_size + i) % args.text_vocab_size   # n_samples <= the vocabulary: no two rows are equal
        rows += [x[0].numpy(), u]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, use_cfg=True,
                                 text_len=x.shape[1], n_spans=num_task, seed=i))
    return rows, cols, knobs
