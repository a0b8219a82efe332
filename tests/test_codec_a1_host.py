"""CPU: the host surface of the opt-in bf16 codec activations (DESIGN I.32) — the `act_dtype` keyword, its defaults and refusals, the CLI
flag, the `bf16_acts` property, and the new library entries' answers that need no GPU (they come before any HIP call)."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import inference_v2
from ssr_speech_amd.codec import wmencodec as WM
from ssr_speech_amd.data.tokenizer import AudioTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssrhip_codec_gemm_a1", "ssrhip_resblock_a1", "ssrhip_codec_a1_launches")


def test_the_keyword_is_keyword_only_and_defaults_to_fp32():
    for fn in (WM.WMEncodecModel.__init__, AudioTokenizer.__init__):
        p = inspect.signature(fn).parameters
        assert p["act_dtype"].kind is inspect.Parameter.KEYWORD_ONLY and p["act_dtype"].default == "fp32", fn
        names = list(p)
        assert names.index("act_dtype") > names.index("weight_dtype"), names
    assert WM.CODEC_ACT_DTYPES == ("fp32", "bf16")


@pytest.mark.parametrize("bad", ["fp16", "e4m3", "BF16", "", None])
@pytest.mark.parametrize("wdt", ["fp32", "bf16"])
def test_any_other_act_dtype_raises_before_anything_is_built(bad, wdt):
    """In front of the device check: it needs no GPU and no weights."""
    with pytest.raises(ValueError, match="act_dtype"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype=wdt, act_dtype=bad)
    with pytest.raises(ValueError, match="act_dtype"):
        AudioTokenizer("cpu", config=object(), state_dict={}, weight_dtype=wdt, act_dtype=bad)


def test_bf16_activations_need_bf16_weights():
    with pytest.raises(ValueError, match=r"act_dtype='bf16' needs weight_dtype='bf16'"):
        WM.WMEncodecModel(None, {}, "cpu", act_dtype="bf16")
    with pytest.raises(ValueError, match=r"act_dtype='bf16' needs weight_dtype='bf16'"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype="fp32", act_dtype="bf16")
    with pytest.raises(ValueError, match=r"act_dtype='bf16' needs weight_dtype='bf16'"):
        AudioTokenizer("cpu", config=object(), state_dict={}, act_dtype="bf16")


def test_bf16_activations_need_the_one_plane_kernels(monkeypatch):
    monkeypatch.setenv("SSRHIP_CODEC_W1", "0")
    with pytest.raises(ValueError, match="SSRHIP_CODEC_W1=0"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype="bf16", act_dtype="bf16")
    with pytest.raises(ValueError, match="SSRHIP_CODEC_W1=0"):
        AudioTokenizer("cpu", config=object(), state_dict={}, weight_dtype="bf16", act_dtype="bf16")
    # with the switch on (or unset) the keyword pair is accepted: the next check, the device's, is the one that answers
    monkeypatch.setenv("SSRHIP_CODEC_W1", "1")
    with pytest.raises(RuntimeError, match="ROCm GPU device"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype="bf16", act_dtype="bf16")
    monkeypatch.delenv("SSRHIP_CODEC_W1")
    with pytest.raises(RuntimeError, match="ROCm GPU device"):
        WM.WMEncodecModel(None, {}, "cpu", weight_dtype="bf16", act_dtype="bf16")


def test_the_valid_defaults_reach_the_device_check():
    """act_dtype="fp32" goes with either weight_dtype, whatever the switch says."""
    for wdt in ("fp32", "bf16"):
        with pytest.raises(RuntimeError, match="ROCm GPU device"):
            WM.WMEncodecModel(None, {}, "cpu", weight_dtype=wdt, act_dtype="fp32")


def test_bf16_acts_needs_a_one_plane_model_built_with_the_keyword():
    m = object.__new__(WM.WMEncodecModel)                                             # the property reads three attributes and nothing else
    for wdt, knob, adt, want in (("bf16", True, "bf16", True), ("bf16", True, "fp32", False), ("bf16", False, "bf16", False),
                                 ("fp32", True, "bf16", False), ("fp32", True, "fp32", False)):
        m.weight_dtype, m.codec_w1, m.act_dtype = wdt, knob, adt
        assert m.bf16_acts is want, (wdt, knob, adt)
    assert "bf16_acts" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_cli_flag_is_the_projects_own():
    assert "--codec_act_dtype" not in [f for f, _ in inference_v2.REFERENCE_FLAGS]
    flags = dict(inference_v2.EXTRA_FLAGS)
    assert flags["--codec_act_dtype"]["choices"] == ["fp32", "bf16"] and flags["--codec_act_dtype"]["default"] == "fp32"
    order = [f for f, _ in inference_v2.EXTRA_FLAGS]
    assert abs(order.index("--codec_act_dtype") - order.index("--codec_weight_dtype")) == 1       # next to --codec_weight_dtype


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in bound, name
        assert getattr(raw, name) is not None
    assert _lib.lib().ssrhip_version() == 107 == _lib.ABI_VERSION                      # additions only: no struct changed
    assert WM._NoLaunch().ssrhip_codec_gemm_a1(None, None) == 0 and WM._NoLaunch().ssrhip_resblock_a1(None, None) == 0     # the sizing pass's stand-in


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


def test_codec_gemm_a1_answers_as_its_twin_without_a_gpu():
    L = _lib.lib()
    assert L.ssrhip_codec_gemm_a1(None, None) < 0 and b"ssrhip_codec_gemm_a1: null argument" in L.ssrhip_last_error()
    a = _fake_gemm()
    a.W_split = 0
    assert L.ssrhip_codec_gemm_a1(C.byref(a), None) < 0 and b"W_split is NULL" in L.ssrhip_last_error()
    a = _fake_gemm(K=66)
    assert L.ssrhip_codec_gemm_a1(C.byref(a), None) < 0 and b"multiples of 4" in L.ssrhip_last_error()
    n0, w0 = L.ssrhip_codec_a1_launches(), L.ssrhip_codec_w1_launches()
    for kw in (dict(N=64), dict(N=33), dict(K=68), dict(N=64, act_in=_lib.ACT_ELU)):
        assert L.ssrhip_codec_gemm_a1(C.byref(_fake_gemm(**kw)), None) == 1, kw         # does not qualify, nothing launched
        assert L.ssrhip_codec_gemm_w1(C.byref(_fake_gemm(**kw)), None) == 1, kw         # ... exactly where the twin says so
    assert L.ssrhip_codec_a1_launches() == n0 and L.ssrhip_codec_w1_launches() == w0    # the counters count launches, not calls


def test_resblock_a1_answers_as_its_twin_without_a_gpu():
    L = _lib.lib()
    assert L.ssrhip_resblock_a1(None, None) < 0 and b"ssrhip_resblock_a1: null argument" in L.ssrhip_last_error()
    for drop in ("w3_split", "w1_split"):                                              # one plane pointer without the other
        a = _fake_res()
        setattr(a, drop, 0)
        assert L.ssrhip_resblock_a1(C.byref(a), None) < 0 and b"both required" in L.ssrhip_last_error(), drop
    a = _fake_res()
    a.T = 0
    assert L.ssrhip_resblock_a1(C.byref(a), None) < 0
    n0 = L.ssrhip_codec_a1_launches()
    for Cc in (256, 512, 32):
        assert L.ssrhip_resblock_a1(C.byref(_fake_res(Cc)), None) == 1, Cc             # another C: nothing launched
    assert L.ssrhip_codec_a1_launches() == n0


@pytest.mark.parametrize("switch", ["SSRHIP_GEMM_SPLIT", "SSRHIP_RESBLOCK_DMA"])
def test_with_the_dma_kernel_switched_off_every_call_answers_1(switch):
    """Both switches are read once per process: a fresh child, calls that would qualify. SSRHIP_RESBLOCK_DMA=0 concerns the residual block
    alone."""
    code = ("import ctypes as C, ssr_speech_amd\nfrom ssr_speech_amd import _lib\nL = _lib.lib()\n"
            "a = _lib.GemmArgs()\na.A, a.W, a.C, a.W_split = 0x1000, 0x2000, 0x3000, 0x4000\n"
            "a.M, a.N, a.K, a.lda, a.ldc = 200, 256, 64, 64, 256\n"
            "r = _lib.ResblockArgs()\nr.x, r.y, r.w3, r.b3, r.w1, r.b1 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000\n"
            "r.B, r.T, r.C, r.x_bstride, r.y_bstride = 2, 100, 128, 102 * 128, 100 * 128\nr.w3_split, r.w1_split = 0x7000, 0x8000\n"
            "print('res', L.ssrhip_resblock_a1(C.byref(r), None))\n"
            "if '%s' == 'SSRHIP_GEMM_SPLIT': print('gemm', L.ssrhip_codec_gemm_a1(C.byref(a), None))\n"
            "print('launches', L.ssrhip_codec_a1_launches())\n" % switch)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{switch: "0"}), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "res 1" in out.stdout and "launches 0" in out.stdout, out.stdout + out.stderr
    assert switch != "SSRHIP_GEMM_SPLIT" or "gemm 1" in out.stdout, out.stdout
