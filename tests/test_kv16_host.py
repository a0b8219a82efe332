"""The opt-in bf16 KV cache on the host (no GPU): the pure rule that decides an engine's cache type, the public switch and the CLI flag,
the contract errors of the C side that are answered before any launch, the rounding helper of the GPU tests against torch's own
conversion, and the oracle shim those tests compare with."""
import ctypes as C

import numpy as np
import pytest
import torch

from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E
from ssr_speech_amd import weights as W

import helpers_kv16 as HK
from helpers_w16 import fake_gemv_args


@pytest.mark.parametrize("rows", [1, 2, 4, 5, 16, 17, 32])
def test_resolve_kv_dtype(rows):
    fits = rows >= 5
    for model_default in E.KV_DTYPES:
        assert E.resolve_kv_dtype(rows, None, model_default) == (model_default if fits else "fp32")
        assert E.resolve_kv_dtype(rows, "fp32", model_default) == "fp32"
        if fits:
            assert E.resolve_kv_dtype(rows, "bf16", model_default) == "bf16"
            assert E.resolve_kv_dtype(rows, "bf16", model_default, max_pages=256) == "bf16"
            with pytest.raises(ValueError, match="256 pages"):
                E.resolve_kv_dtype(rows, "bf16", model_default, max_pages=257)
            assert E.resolve_kv_dtype(rows, None, model_default, max_pages=257) == "fp32"
        else:
            with pytest.raises(ValueError, match="5..32 rows"):
                E.resolve_kv_dtype(rows, "bf16", model_default)
    for bad in ("fp16", "BF16", ""):
        with pytest.raises(ValueError, match="not in"):
            E.resolve_kv_dtype(rows, bad, "fp32")
        with pytest.raises(ValueError, match="not in"):
            E.resolve_kv_dtype(rows, None, bad)
    assert E.KV_DTYPES == ("fp32", "bf16")


def test_set_kv_dtype_takes_the_two_names_only():
    from ssr_speech_amd.models.ssr import SSR_Speech
    m = SSR_Speech(W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64))
    assert m.kv_dtype == "fp32"
    m.set_kv_dtype("bf16")
    assert m.kv_dtype == "bf16" and m.weight_dtype == "fp32"              # independent of the weight type
    m.set_weight_dtype("bf16")
    assert m.kv_dtype == "bf16"
    for bad in ("fp16", "bfloat16", None, 16):
        with pytest.raises(ValueError):
            m.set_kv_dtype(bad)
    assert m.kv_dtype == "bf16"
    m.set_kv_dtype("fp32")
    assert m.kv_dtype == "fp32"


def test_cli_flag_parses():
    from ssr_speech_amd import inference_v2 as CLI
    flags = dict(CLI.EXTRA_FLAGS)
    assert flags["--kv_dtype"]["choices"] == ["fp32", "bf16"] and flags["--kv_dtype"]["default"] == "fp32"
    names = [f for f, _ in CLI.EXTRA_FLAGS]
    assert names.index("--kv_dtype") == names.index("--weight_dtype") + 1
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv_dtype", **flags["--kv_dtype"])
    assert ap.parse_args([]).kv_dtype == "fp32" and ap.parse_args(["--kv_dtype", "bf16"]).kv_dtype == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(["--kv_dtype", "fp8"])


@pytest.mark.parametrize("B", [1, 2, 4])
def test_the_two_byte_append_is_a_contract_error_at_four_rows_and_below(B):
    """answered before any HIP call: the pointers of these arguments are never dereferenced"""
    L = _lib.lib()
    a = fake_gemv_args(B, N=3 * 2048, K=2048, w_tiled=0, pro=_lib.PRO_LAYERNORM)
    a.epi = _lib.EPI_QKV_APPEND16
    a.kv = _lib.KV(0x4000, 0x5000, 2, 2, 16, 128)
    a.kv_pos = 0x6000
    assert L.ssrhip_gemv(C.byref(a), None) < 0 and b"5..32 rows" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_w16(C.byref(a), 0x7000, None) < 0 and b"5..32 rows" in L.ssrhip_last_error()
    b = fake_gemv_args(B, N=2048, K=8192, w_tiled=0)
    b.epi = _lib.EPI_RESIDUAL
    assert L.ssrhip_gemv_pair(C.byref(b), C.byref(a), 0x8000, 0, 1, None) < 0 and b"5..32 rows" in L.ssrhip_last_error()


def test_rounding_helper_equals_torch():
    sp = HK.special_values()
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(1 << 16, generator=g) * torch.exp(torch.randn(1 << 16, generator=g) * 8)
    every_upper_half = (torch.arange(1 << 16, dtype=torch.int64) << 16 | 0x8000)             # a tie behind every bf16 value
    every_upper_half = torch.where(every_upper_half >= (1 << 31), every_upper_half - (1 << 32), every_upper_half).to(torch.int32).view(torch.float32)
    for t in (sp, rnd, every_upper_half):
        ref = t.to(torch.bfloat16)
        got = HK.bf16_bits(t)
        finite_or_inf = ~torch.isnan(t)
        assert torch.equal(got[finite_or_inf], ref.view(torch.int16)[finite_or_inf])
        assert torch.isnan(HK.widen(got)[~finite_or_inf]).all()                               # NaN stays NaN
        assert torch.equal(HK.widen(ref)[finite_or_inf], ref.float()[finite_or_inf])          # the widening is the 16-bit shift
        assert torch.equal(HK.bf16_bits(HK.widen(got)), got)                                  # idempotent
    w = HK.round_bf16(sp)
    bits = dict(zip(HK.SPECIAL_BITS, (int(v) & 0xFFFF for v in HK.bf16_bits(sp))))
    assert bits[0x3F808000] == 0x3F80 and bits[0x3F818000] == 0x3F82 and bits[0xBF808000] == 0xBF80 and bits[0xBF818000] == 0xBF82
    assert bits[0x00000000] == 0x0000 and bits[0x80000000] == 0x8000 and bits[0x00008000] == 0x0000 and bits[0x00018000] == 0x0002
    assert bits[0x7F7FFFFF] == 0x7F80 and bits[0xFF7FFFFF] == 0xFF80 and bits[0x7F7F7FFF] == 0x7F7F
    assert bits[0x7F800000] == 0x7F80 and bits[0xFF800000] == 0xFF80 and torch.isinf(w[-2:]).all()


@pytest.mark.parametrize("cfg", sorted(HK.CONFIGS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_shim_moves_the_logits_but_not_the_tokens(monkeypatch, cfg, seed):
    """On the inputs of the GPU comparison (tests/test_gpu_kv16.py) the shimmed oracle differs from the plain one by more than LOGIT_ATOL
    somewhere — an engine with an fp32 cache cannot pass that comparison — and picks the same greedy tokens, so the margins are wide."""
    from oracle import lm as O
    plain_F = O.F
    lg16, tok16 = HK.oracle_trace(monkeypatch, cfg, seed, True)
    assert O.F is plain_F                                                                     # the shim is gone again
    lg32, tok32 = HK.oracle_trace(monkeypatch, cfg, seed, False)
    assert lg16.shape == lg32.shape and lg16.shape[0] == HK.STEPS
    finite = np.isfinite(lg32) & np.isfinite(lg16)
    assert np.array_equal(np.isfinite(lg32), np.isfinite(lg16))
    diff = np.abs(np.where(finite, lg16 - lg32, 0.0)).max()
    print(f"{cfg} seed {seed}: max |shimmed - plain| logit = {diff:.2e}")
    assert diff > HK.LOGIT_ATOL, diff
    assert np.array_equal(tok16, tok32)
