"""Shared by the tests of the bf16 KV cache of the 1/2/4-row decode step (DESIGN.md Part I.23; tests/test_kv16_small_host.py,
tests/test_gpu_kv16_small.py): the engine configurations and utterance seeds of the engine-level comparison, their oracle traces with and
without bf16-valued K / V (computed once per configuration, seed and CFG mode, shared, never modified), the engine inputs, and a numpy
model of the addresses the landing cache is written and read at."""
import numpy as np
import torch

from oracle import lm as O
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeKnobs

import helpers_kv16 as HK
from helpers_w16 import _utterance

PAGE = _lib.PAGE
LOGIT_ATOL = HK.LOGIT_ATOL                 # 2e-4, the project's bound on the engine's logits against its oracle
MIN_GAP = 2 * LOGIT_ATOL                   # what rounding K / V must move the oracle's logits by, so that an fp32 cache cannot pass
STEPS = HK.STEPS
# d128 / d1024: the configurations of tests/helpers_kv16.py (head_dim 64); d256h2: head_dim 128 (the kernels' other instantiation)
CONFIGS = dict(HK.CONFIGS, d256h2=dict(d_model=256, nhead=2, layers=2, vocab=64))
# rows -> (utterances, CFG): 1 row is one utterance without CFG, 2 rows one utterance under CFG, 4 rows two utterances under CFG
ROWS = {1: (1, False), 2: (1, True), 4: (2, True)}
# the utterance seeds per configuration: `cfg` the two utterances decoded under CFG (the 2-row engine takes the first), `plain` the one
# decoded without. Chosen so that every one meets MIN_GAP (asserted on the CPU in tests/test_kv16_small_host.py, which prints the gaps).
# Measured over seeds 1..6: 7.1e-4..1.1e-3 under CFG and 5.6e-4..7.9e-4 without, in all three configurations; these are the larger ones.
SEEDS = {"d128": dict(cfg=(2, 3), plain=2), "d1024": dict(cfg=(1, 3), plain=6), "d256h2": dict(cfg=(1, 5), plain=3)}

_MODELS, _TRACES = {}, {}


def model_cpu(cfg: str):
    if cfg not in _MODELS:
        args = W.lm_args_tiny(**CONFIGS[cfg])
        _MODELS[cfg] = (args, W.lm_state_dict(args, seed=HK.SD_SEED))
    return _MODELS[cfg]


def seeds_of(cfg: str, rows: int):
    n_utt, use_cfg = ROWS[rows]
    return list(SEEDS[cfg]["cfg"][:n_utt]) if use_cfg else [SEEDS[cfg]["plain"]]


def oracle_trace(monkeypatch, cfg: str, seed: int, kv16: bool, use_cfg: bool):
    """(post-edit logits [steps][K][card], samples [steps][K]) of the oracle on utterance `seed` alone, under CFG or without; kv16: with
    the oracle module's `F` replaced by the rounding shim of tests/helpers_kv16.py for the duration of the run"""
    key = (cfg, seed, kv16, use_cfg)
    if key not in _TRACES:
        args, sd = model_cpu(cfg)
        x, y, unc, mi = _utterance(args, seed)
        trace = {}
        kw = dict(HK.KW, aug_text=use_cfg)
        with monkeypatch.context() as mp:
            if kv16:
                mp.setattr(O, "F", HK.kv16_functional())
            O.inference(O.reference_params(sd), args, x, y, mi, uncond_x=unc if use_cfg else None, max_steps=STEPS, trace=trace, **kw)
        _TRACES[key] = (torch.stack(trace["edited_logits"]).numpy(), torch.stack(trace["samples"]).numpy())
    return _TRACES[key]


def oracle_gap(monkeypatch, cfg: str, seed: int, use_cfg: bool):
    """(max |shimmed - plain| over the finite post-edit logits of the common steps, same tokens?)"""
    lg16, tok16 = oracle_trace(monkeypatch, cfg, seed, True, use_cfg)
    lg32, tok32 = oracle_trace(monkeypatch, cfg, seed, False, use_cfg)
    n = min(lg16.shape[0], lg32.shape[0])
    finite = np.isfinite(lg32[:n]) & np.isfinite(lg16[:n])
    return float(np.abs(np.where(finite, lg16[:n] - lg32[:n], 0.0)).max()), bool(np.array_equal(tok16[:n], tok32[:n]))


def engine_inputs(args, seeds, use_cfg: bool):
    """(text rows, audio columns, knobs) of DecodeEngine.start for the utterances `seeds`"""
    rows, cols, knobs = [], [], []
    for u, seed in enumerate(seeds):
        x, y, unc, mi = _utterance(args, seed)
        cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)
        rows += [x[0].numpy(), unc[0].numpy()] if use_cfg else [x[0].numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, use_cfg=use_cfg,
                                 text_len=x.shape[1], n_spans=num_task, seed=u))
    return rows, cols, knobs


# ------------------------------------------------------------------------------------------ the address model (element offsets)
def landing_descriptor(B, n_layer, n_head, head_dim, layer):
    """What StepShapes::qkv_args hands the QKV launch of `layer` (csrc/engine.hip): the cache record, the layer index, and the contents
    of the table and of this layer's slice of land_pos"""
    kv = dict(max_pages=1, n_layer=1, n_head=n_head, head_dim=head_dim)
    return kv, 0, np.arange(B, dtype=np.int64), np.full(B, layer, dtype=np.int64)


def append_offset_bases(kv, layer, table, kv_pos, b, which, h):
    """kv_append_bases (csrc/gemv_shared.h): the head-0 base of row b, then head h's row behind it (h * SSRHIP_PAGE * head_dim)"""
    pos = kv_pos[b]
    page = table[b * kv["max_pages"] + pos // PAGE]
    base = ((((page * kv["n_layer"] + layer) * 2 + which) * kv["n_head"]) * PAGE + pos % PAGE) * kv["head_dim"]
    return base + h * PAGE * kv["head_dim"]


def append_offset_kv_addr(kv, layer, table, kv_pos, b, which, h):
    """kv_addr (csrc/common.h), as csrc/gemv.hip calls it: head 0, then the head's stride"""
    pos = kv_pos[b]
    page = table[b * kv["max_pages"] + pos // PAGE]
    off = ((((page * kv["n_layer"] + layer) * 2 + which) * kv["n_head"] + 0) * PAGE + pos % PAGE)
    return off * kv["head_dim"] + h * PAGE * kv["head_dim"]


def append_offset_pair_edge(kv, layer, table, kv_pos, b, which, h):
    """pair_edge_role (csrc/gemv_pair.h): kvoff[lane * 2 + which], as element offsets"""
    pos = kv_pos[b]
    page = table[b * kv["max_pages"] + pos // PAGE]
    k0 = ((((page * kv["n_layer"] + layer) * 2 + which) * kv["n_head"]) * PAGE + pos % PAGE)
    return k0 * kv["head_dim"] + h * PAGE * kv["head_dim"]


WRITER_FORMS = (append_offset_bases, append_offset_kv_addr, append_offset_pair_edge)


def reader_offset(n_head, head_dim, layer, r, which, h):
    """attn_decode_kernel<.., KV16 = true> (csrc/attn.hip): the landing entry of (row, head), arithmetic on kernel arguments only"""
    return (((r * 2 + which) * n_head + h) * PAGE + layer) * head_dim
