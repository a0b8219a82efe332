"""CPU: the host side of the one-plane prefill GEMM (DESIGN.md Part I.13) — who decides how many bf16 planes an arena's `*_ws` buffers
hold, that the count stays with the buffers, the answers `ssrhip_gemm_w1` gives before any launch, and that the C ABI only grew."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E
from ssr_speech_amd import weights as W
from ssr_speech_amd.engine import LMWeightsArena, resolve_prefill_planes
from ssr_speech_amd.models.ssr import SSR_Speech

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssrhip_gemm_w1", "ssrhip_lm_set_prefill_w1", "ssrhip_lm_score_w1", "ssrhip_gemm_w1_launches")
FAMILIES = ("in_proj", "out_proj", "ffn1", "ffn2")


def test_the_switch_function_for_every_combination():
    """(dtype, SSRHIP_PREFILL_SPLIT, SSRHIP_PREFILL_W1, explicit argument) -> 0, 1 or 3 planes, or a ValueError"""
    assert E.PREFILL_W1_DEFAULT in ("0", "1")
    default_bf16 = 1 if E.PREFILL_W1_DEFAULT == "1" else 3
    for dtype, split, w1, req in itertools.product(("fp32", "bf16"), (None, "0", "1", "0x"), (None, "0", "1", "00", "yes"), (None, 1, 3)):
        env = {k: v for k, v in (("SSRHIP_PREFILL_SPLIT", split), ("SSRHIP_PREFILL_W1", w1)) if v is not None}
        case = (dtype, split, w1, req)
        if req == 1 and dtype == "fp32":                                   # named before the environment is looked at
            with pytest.raises(ValueError, match="one plane per matrix needs an arena built with weight_dtype='bf16'"):
                resolve_prefill_planes(dtype, req, env)
            continue
        got = resolve_prefill_planes(dtype, req, env)
        if split is not None and split[:1] == "0":
            assert got == 0, case                                          # SSRHIP_PREFILL_SPLIT=0: no planes at all, whatever else is asked
        elif req is not None:
            assert got == req, case
        elif dtype == "fp32":
            assert got == 3, case                                          # an fp32 arena always has three
        elif w1 is None:
            assert got == default_bf16, case
        else:
            assert got == (3 if w1[:1] == "0" else 1), case
    for bad in (0, 2, 6, "1"):
        with pytest.raises(ValueError, match="split planes come as 1 or 3 per matrix"):
            resolve_prefill_planes("bf16", bad, {})


def _tiny():
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=1, vocab=64)
    return args, W.lm_state_dict(args, seed=3)


def test_a_bf16_arena_builds_one_plane_per_matrix_and_keeps_the_count(monkeypatch):
    """The one plane is a conversion, no kernel: it can be built (and looked at) without a GPU."""
    args, sd = _tiny()
    monkeypatch.delenv("SSRHIP_PREFILL_SPLIT", raising=False)
    monkeypatch.setenv("SSRHIP_PREFILL_W1", "1")
    a = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    assert a.split_planes == 3 and a.split_plane_bytes() == 0              # nothing built, nothing decided
    gen0 = a.generation
    assert a.ensure_split_planes() is True and a.ensure_split_planes() is False and a.generation == gen0 + 1
    assert a.split_planes == 1
    monkeypatch.setenv("SSRHIP_PREFILL_W1", "0")                           # read once, where the planes were built: the head planes follow the arena
    assert a.ensure_head_split_planes() is True and a.ensure_head_split_planes() is False and a.split_planes == 1
    n = 0
    for name in FAMILIES:
        Wm, ws = a.layers[0][name + "_w"], a.layers[0][name + "_ws"]
        assert ws.dtype == torch.int16 and ws.numel() == Wm.numel() and ws.is_contiguous()
        assert torch.equal(((ws.to(torch.int32) & 0xFFFF) << 16).view(torch.float32).view_as(Wm), Wm), name      # the weight itself
        n += Wm.numel()
    for ws, Wm in ((a.head1_ws, a.head1_w), (a.head2_ws, a.head2_w)):      # head2: [K][card][Hh], codebook after codebook
        assert torch.equal(((ws.to(torch.int32) & 0xFFFF) << 16).view(torch.float32), Wm.reshape(-1))
        n += Wm.numel()
    assert a.split_plane_bytes() == 2 * n
    w = a.c_struct()
    assert w.in_proj_ws[0] == a.layers[0]["in_proj_ws"].data_ptr()
    with pytest.raises(ValueError, match="already come 1 per matrix; 3 asked for"):
        a.ensure_split_planes(planes=3)
    assert a.ensure_split_planes(planes=1) is False


def test_explicit_requests_and_the_fp32_arena(monkeypatch):
    args, sd = _tiny()
    monkeypatch.delenv("SSRHIP_PREFILL_SPLIT", raising=False)
    monkeypatch.setenv("SSRHIP_PREFILL_W1", "1")
    a32 = LMWeightsArena(args, sd, torch.device("cpu"))
    with pytest.raises(ValueError, match="one plane per matrix needs an arena built with weight_dtype='bf16'"):
        a32.ensure_split_planes(planes=1)
    with pytest.raises(ValueError, match="one plane per matrix needs an arena built with weight_dtype='bf16'"):
        a32.ensure_head_split_planes(planes=1)
    assert a32.split_planes == 3 and not getattr(a32, "_ws_ready", False)
    assert resolve_prefill_planes("fp32", None, os.environ) == 3           # the switch means nothing to an fp32 arena
    monkeypatch.setenv("SSRHIP_PREFILL_W1", "0")
    a16 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    assert a16.ensure_split_planes(planes=1) is True and a16.split_planes == 1      # the argument beats the switch
    monkeypatch.setenv("SSRHIP_PREFILL_SPLIT", "0")
    b16 = LMWeightsArena(args, sd, torch.device("cpu"), weight_dtype="bf16")
    assert b16.ensure_split_planes(planes=1) is False and b16.ensure_head_split_planes() is False
    assert not getattr(b16, "_ws_ready", False) and b16.split_plane_bytes() == 0 and not b16.c_struct().in_proj_ws


def test_set_weight_dtype_round_trip_leaves_no_planes_behind(monkeypatch):
    args, sd = _tiny()
    monkeypatch.delenv("SSRHIP_PREFILL_SPLIT", raising=False)
    m = SSR_Speech(args)
    m.load_state_dict(sd)
    m.set_weight_dtype("bf16")
    m._arena = LMWeightsArena(args, m.state_dict(), torch.device("cpu"), weight_dtype=m.weight_dtype)      # what `score` builds on first use
    assert m._arena.ensure_split_planes(planes=1) and m._arena.ensure_head_split_planes() and m._arena.split_planes == 1
    m.set_weight_dtype("fp32")
    assert m._arena is None and m._engines == {} and m.weight_dtype == "fp32"
    fresh = LMWeightsArena(args, m.state_dict(), torch.device("cpu"), weight_dtype=m.weight_dtype)
    assert fresh.split_planes == 3 and fresh.split_plane_bytes() == 0 and not any(k.endswith("_ws") for k in fresh.layers[0])
    assert torch.equal(fresh.layers[0]["ffn1_w"], LMWeightsArena(args, sd, torch.device("cpu")).layers[0]["ffn1_w"])   # the unrounded masters again


def _fake_gemm(N=256, K=64, act_in=0):
    """launch arguments whose pointers are never dereferenced: every call made with them is answered before any HIP call"""
    a = _lib.GemmArgs()
    a.A, a.W, a.C, a.W_split = 0x1000, 0x2000, 0x3000, 0x4000
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = 200, N, K, K, N, act_in
    return a


def test_gemm_w1_answers_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_gemm_w1(None, None) < 0 and b"ssrhip_gemm_w1: null argument" in L.ssrhip_last_error()
    a = _fake_gemm()
    a.W_split = 0
    assert L.ssrhip_gemm_w1(C.byref(a), None) < 0 and b"W_split is NULL" in L.ssrhip_last_error()
    a = _fake_gemm(K=66)
    assert L.ssrhip_gemm_w1(C.byref(a), None) < 0 and b"multiples of 4" in L.ssrhip_last_error()     # ssrhip_gemm's own contract
    n0 = L.ssrhip_gemm_w1_launches()
    for kw in (dict(N=64), dict(N=33), dict(K=68), dict(act_in=_lib.ACT_ELU)):
        a = _fake_gemm(**kw)
        assert L.ssrhip_gemm_w1(C.byref(a), None) == 1, kw                   # does not qualify, nothing launched
    assert L.ssrhip_gemm_w1_launches() == n0                               # the counter counts launches, not calls
    assert L.ssrhip_lm_set_prefill_w1(None, 1) < 0 and b"ssrhip_lm_set_prefill_w1" in L.ssrhip_last_error()
    assert L.ssrhip_lm_score_w1(None, None, None, None) < 0


def test_gemm_split_0_makes_every_call_answer_1():
    """SSRHIP_GEMM_SPLIT=0 (read once per process): a fresh child, a call that would qualify."""
    code = ("import ctypes as C, ssr_speech_amd\nfrom ssr_speech_amd import _lib\nL = _lib.lib()\na = _lib.GemmArgs()\n"
            "a.A, a.W, a.C, a.W_split = 0x1000, 0x2000, 0x3000, 0x4000\na.M, a.N, a.K, a.lda, a.ldc = 200, 256, 64, 64, 256\n"
            "print('answer', L.ssrhip_gemm_w1(C.byref(a), None))\n")
    import sys
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SSRHIP_GEMM_SPLIT="0"), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "answer 1" in out.stdout, out.stdout + out.stderr


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint(?:64_t)? " + name + r"\(", header), name
        assert name in bound, name
        assert getattr(raw, name) is not None, name
    L = _lib.lib()
    assert L.ssrhip_version() == 107 == _lib.ABI_VERSION and "#define SSRHIP_VERSION 107" in header      # additions only
    assert "the LM prefill does not" not in header                        # (the W_split comment said so long after the prefill took the planes)
