"""Shared by the tests of the opt-in bf16 KV cache (tests/test_kv16_host.py, tests/test_gpu_kv16.py): the rounding helper in integer
arithmetic, the oracle shim whose attention sees bf16-valued K / V, and the prompts and oracle traces of the engine-level comparisons
(computed once per configuration and utterance, shared, never modified)."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import lm as O
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import DecodeKnobs

from helpers_w16 import _utterance

LOGIT_ATOL = 2e-4            # the bound tests/test_gpu_lm.py holds the fp32 engine to against the reference
STEPS = 24
SD_SEED = 11
CONFIGS = {"d128": dict(d_model=128, nhead=2, layers=2, vocab=64), "d1024": dict(d_model=1024, nhead=16, layers=2, vocab=64)}
KW = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=2, aug_text=True)


def bf16_bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> the 16 bits of the bf16 entry (int16), round to nearest even in integer arithmetic: what the kernels do. A finite value
    above the largest bf16 carries into the exponent (inf); a NaN keeps its upper bits and gets the quiet bit."""
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    out = torch.where(nan, (u >> 16) | 0x40, rounded) & 0xFFFF
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def widen(bits: torch.Tensor) -> torch.Tensor:
    """int16 / bfloat16 entries -> fp32 by the 16-bit shift (exact)"""
    if bits.dtype == torch.bfloat16:
        bits = bits.view(torch.int16)
    return ((bits.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    return widen(bf16_bits(t))


SPECIAL_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties, towards the even neighbour below and above
                0x3F808001, 0x3F807FFF,                              # just above / below a tie
                0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,    # +-0 and denormals (ties among them)
                0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,      # the largest finite fp32 and the tie below inf: overflow to inf
                0x7F800000, 0xFF800000]                              # +-inf


def special_values() -> torch.Tensor:
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in SPECIAL_BITS], dtype=torch.int64).to(torch.int32).view(torch.float32)


def kv16_functional():
    """torch.nn.functional with a scaled_dot_product_attention that rounds k and v to bf16 and back first. Rounding is idempotent, so
    re-rounding the concatenated `past` at every step is exactly "every K / V entry is rounded once, when it is written"."""
    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})

    def sdpa(q, k, v, *a, **kw):
        return F.scaled_dot_product_attention(q, k.to(torch.bfloat16).to(k.dtype), v.to(torch.bfloat16).to(v.dtype), *a, **kw)

    ns.scaled_dot_product_attention = sdpa
    return ns


@functools.lru_cache(maxsize=None)
def model_cpu(cfg: str):
    args = W.lm_args_tiny(**CONFIGS[cfg])
    return args, W.lm_state_dict(args, seed=SD_SEED)


_TRACES = {}


def oracle_trace(monkeypatch, cfg: str, seed: int, kv16: bool):
    """(post-edit logits [STEPS][K][card], samples [STEPS][K]) of the oracle on utterance `seed` alone, computed once; kv16: with the
    module's `F` replaced by the shim for the duration of the run (oracle/ itself is not edited)"""
    key = (cfg, seed, kv16)
    if key not in _TRACES:
        args, sd = model_cpu(cfg)
        x, y, unc, mi = _utterance(args, seed)
        trace = {}
        with monkeypatch.context() as mp:
            if kv16:
                mp.setattr(O, "F", kv16_functional())
            O.inference(O.reference_params(sd), args, x, y, mi, uncond_x=unc, max_steps=STEPS, trace=trace, **KW)
        _TRACES[key] = (torch.stack(trace["edited_logits"]).numpy(), torch.stack(trace["samples"]).numpy())
    return _TRACES[key]


def engine_inputs(args, seeds):
    """(text rows, audio columns, knobs) of DecodeEngine.start for the utterances `seeds` under CFG"""
    rows, cols, knobs = [], [], []
    for u, seed in enumerate(seeds):
        x, y, unc, mi = _utterance(args, seed)
        cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)
        rows += [x[0].numpy(), unc[0].numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, use_cfg=True,
                                 text_len=x.shape[1], n_spans=num_task, seed=u))
    return rows, cols, knobs
