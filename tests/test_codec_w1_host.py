"""CPU: the host surface of the opt-in bf16-rounded codec (DESIGN I.30) — the `weight_dtype` keyword and its defaults, the `codec_w1`
knob, the CLI flag, the rounding helper, and the new library entries' answers that need no GPU (they come before any HIP call)."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import inference_v2
from ssr_speech_amd.codec import wmencodec as WM
from ssr_speech_amd.data.tokenizer import AudioTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssrhip_codec_gemm_w1", "ssrhip_resblock_w1", "ssrhip_codec_w1_launches")


def test_the_keyword_is_keyword_only_behind_state_dict_and_defaults_to_fp32():
    for fn in (WM.WMEncodecModel.__init__, AudioTokenizer.__init__):
        p = inspect.signature(fn).parameters
        assert p["weight_dtype"].kind is inspect.Parameter.KEYWORD_ONLY and p["weight_dtype"].default == "fp32", fn
        names = list(p)
        assert names.index("weight_dtype") > names.index("state_dict"), names
    assert WM.CODEC_WEIGHT_DTYPES == ("fp32", "bf16")


@pytest.mark.parametrize("bad", ["int8", "e4m3", "BF16", "", None])
def test_any_other_weight_dtype_raises_before_anything_else(bad):
    """The check comes first: in front of the device check, so it needs no GPU and no weights."""
    with pytest.raises(ValueError, match="weight_dtype"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype=bad)
    with pytest.raises(ValueError, match="weight_dtype"):
        AudioTokenizer("cpu", config=object(), state_dict={}, weight_dtype=bad)


def test_the_knob_is_in_the_table_and_unset_means_on():
    row = [k for k in WM._ENV_KNOBS if k[0] == "codec_w1"]
    assert len(row) == 1
    attr, switch, unset, parse = row[0]
    assert switch == "SSRHIP_CODEC_W1" and unset == "1"
    assert parse("1") is True and parse("") is True and parse("0") is False            # as SSRHIP_PREFILL_W1: off iff "0"
    assert "SSRHIP_CODEC_W1" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_one_plane_needs_a_bf16_model_and_the_knob():
    m = object.__new__(WM.WMEncodecModel)                                             # the property reads two attributes and nothing else
    for wdt, knob, want in (("bf16", True, True), ("bf16", False, False), ("fp32", True, False), ("fp32", False, False)):
        m.weight_dtype, m.codec_w1 = wdt, knob
        assert m.one_plane is want, (wdt, knob)


def test_rounding_is_nearest_even_to_a_bf16_value_kept_in_fp32():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(64, 48, generator=g)
    r = WM._round_w(w, "bf16")
    assert r.dtype == torch.float32 and torch.equal(r, w.to(torch.bfloat16).float()) and not torch.equal(r, w)
    assert torch.equal(r.view(torch.int32) & 0xFFFF, torch.zeros(64, 48, dtype=torch.int32))       # the low 16 bits are gone
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])                         # halfway between two bf16 values: to the even one
    assert WM._round_w(tie, "bf16").tolist() == [1.0, 1.0 + 2.0 ** -6]
    assert WM._round_w(w, "fp32") is w                                                  # the default touches nothing


def test_the_cli_flag_is_the_projects_own():
    assert "--codec_weight_dtype" not in [f for f, _ in inference_v2.REFERENCE_FLAGS]
    flags = dict(inference_v2.EXTRA_FLAGS)
    assert flags["--codec_weight_dtype"]["choices"] == ["fp32", "bf16"] and flags["--codec_weight_dtype"]["default"] == "fp32"
    order = [f for f, _ in inference_v2.EXTRA_FLAGS]
    assert order.index("--codec_weight_dtype") == order.index("--weight_dtype") - 1     # next to --weight_dtype (--kv_dtype keeps its place behind it)


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in bound, name
        assert getattr(raw, name) is not None
    assert _lib.lib().ssrhip_version() == 107 == _lib.ABI_VERSION                      # no struct changed


def _fake_gemm(N=256, K=64, act_in=0):
    """launch arguments whose pointers are never dereferenced: every call made with them is answered before any HIP call"""
    a = _lib.GemmArgs()
    a.A, a.W, a.C, a.W_split = 0x1000, 0x2000, 0x3000, 0x4000
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = 200, N, K, K, N, act_in
    return a


def _fake_res(Cc=128):
    a = _lib.ResblockArgs()
    a.x, a.y, a.w3, a.b3, a.w1, a.b1 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    a.B, a.T, a.C, a.x_bstride, a.y_bstride = 2, 100, Cc, 102 * Cc, 100 * Cc
    a.w3_split, a.w1_split = 0x7000, 0x8000
    return a


def test_codec_gemm_w1_answers_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_codec_gemm_w1(None, None) < 0 and b"ssrhip_codec_gemm_w1: null argument" in L.ssrhip_last_error()
    a = _fake_gemm()
    a.W_split = 0
    assert L.ssrhip_codec_gemm_w1(C.byref(a), None) < 0 and b"W_split is NULL" in L.ssrhip_last_error()
    a = _fake_gemm(K=66)
    assert L.ssrhip_codec_gemm_w1(C.byref(a), None) < 0 and b"multiples of 4" in L.ssrhip_last_error()
    n0, g0 = L.ssrhip_codec_w1_launches(), L.ssrhip_gemm_w1_launches()
    for kw in (dict(N=64), dict(N=33), dict(K=68), dict(N=64, act_in=_lib.ACT_ELU)):
        a = _fake_gemm(**kw)
        assert L.ssrhip_codec_gemm_w1(C.byref(a), None) == 1, kw                       # does not qualify, nothing launched
    assert L.ssrhip_codec_w1_launches() == n0 and L.ssrhip_gemm_w1_launches() == g0    # the counters count launches, not calls


def test_resblock_w1_answers_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_resblock_w1(None, None) < 0 and b"ssrhip_resblock_w1: null argument" in L.ssrhip_last_error()
    for drop in ("w3_split", "w1_split"):                                              # one plane pointer without the other
        a = _fake_res()
        setattr(a, drop, 0)
        assert L.ssrhip_resblock_w1(C.byref(a), None) < 0 and b"both required" in L.ssrhip_last_error(), drop
    a = _fake_res()
    a.T = 0
    assert L.ssrhip_resblock_w1(C.byref(a), None) < 0
    n0 = L.ssrhip_codec_w1_launches()
    for Cc in (256, 512, 32):
        assert L.ssrhip_resblock_w1(C.byref(_fake_res(Cc)), None) == 1, Cc             # another C: nothing launched
    assert L.ssrhip_codec_w1_launches() == n0


@pytest.mark.parametrize("switch", ["SSRHIP_GEMM_SPLIT", "SSRHIP_RESBLOCK_DMA"])
def test_with_the_dma_kernel_switched_off_every_call_answers_1(switch):
    """Both switches are read once per process: a fresh child, calls that would qualify. SSRHIP_RESBLOCK_DMA=0 concerns the residual block
    alone."""
    code = ("import ctypes as C, ssr_speech_amd\nfrom ssr_speech_amd import _lib\nL = _lib.lib()\n"
            "a = _lib.GemmArgs()\na.A, a.W, a.C, a.W_split = 0x1000, 0x2000, 0x3000, 0x4000\n"
            "a.M, a.N, a.K, a.lda, a.ldc = 200, 256, 64, 64, 256\n"
            "r = _lib.ResblockArgs()\nr.x, r.y, r.w3, r.b3, r.w1, r.b1 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000\n"
            "r.B, r.T, r.C, r.x_bstride, r.y_bstride = 2, 100, 128, 102 * 128, 100 * 128\nr.w3_split, r.w1_split = 0x7000, 0x8000\n"
            "print('res', L.ssrhip_resblock_w1(C.byref(r), None))\n"
            "if '%s' == 'SSRHIP_GEMM_SPLIT': print('gemm', L.ssrhip_codec_gemm_w1(C.byref(a), None))\n"
            "print('launches', L.ssrhip_codec_w1_launches())\n" % switch)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{switch: "0"}), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "res 1" in out.stdout and "launches 0" in out.stdout, out.stdout + out.stderr
    assert switch != "SSRHIP_GEMM_SPLIT" or "gemm 1" in out.stdout, out.stdout
