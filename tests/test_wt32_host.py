"""CPU: the host side of the bf16 weight stream of the 17..32-row decode step (DESIGN.md Part I.12) — the answers `ssrhip_gemv_wt32` and the
engine's setter give before any launch, and that the C ABI only grew."""
import ctypes as C
import os
import re

import ssr_speech_amd  # noqa: F401
from helpers_w16 import fake_gemv_args
from ssr_speech_amd import _lib

NEW_SYMBOLS = ("ssrhip_gemv_wt32", "ssrhip_gemv_wt32_applicable", "ssrhip_lm_set_wt32", "ssrhip_lm_wt32_launches")


def _fake_args(B=32, **kw):
    return fake_gemv_args(B, **kw)


def test_gemv_wt32_refusals_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_gemv_wt32(None, 0x4000, None) < 0 and b"ssrhip_gemv_wt32: null argument" in L.ssrhip_last_error()
    a = _fake_args()
    assert L.ssrhip_gemv_wt32(C.byref(a), None, None) < 0 and b"ssrhip_gemv_wt32: null argument" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_wt32_applicable(None) == 0
    for kw in (dict(B=16), dict(B=33), dict(B=4), dict(w_tiled=0), dict(K=1040)):
        a = _fake_args(**kw)
        assert L.ssrhip_gemv_wt32(C.byref(a), 0x4000, None) == 1, kw          # does not qualify, nothing launched
        assert L.ssrhip_gemv_wt32_applicable(C.byref(a)) == 0, kw
    # what ssrhip_gemv refuses at these rows is a contract error here too: two panels of 32 k-steps do not fit, no LayerNorm beyond K = 2048
    a = _fake_args(B=32, K=4096, pro=_lib.PRO_LAYERNORM)
    assert L.ssrhip_gemv_wt32(C.byref(a), 0x4000, None) < 0
    assert b"LayerNorm prologue needs K=4096 <= 2048" in L.ssrhip_last_error()
    assert L.ssrhip_gemv_wt32_applicable(C.byref(a)) == 0
    for B in (17, 32):
        a = _fake_args(B=B)
        assert L.ssrhip_gemv_wt32_applicable(C.byref(a)) == 1, B
        assert L.ssrhip_gemv_wt16_applicable(C.byref(a)) == 0, B              # the 5..16-row entry keeps refusing these rows
        assert L.ssrhip_gemv_wt16(C.byref(a), 0x4000, None) == 1, B


def test_lm_wt32_entry_points_and_the_abi():
    L = _lib.lib()
    assert L.ssrhip_lm_wt32_launches(None) == 0
    assert L.ssrhip_lm_set_wt32(None, None) < 0 and b"ssrhip_lm_set_wt32" in L.ssrhip_last_error()
    assert L.ssrhip_version() == 107 and L.ssrhip_sizeof(16) == -1            # additions only, the record is ssrhip_lm_w16


def test_the_new_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssrhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in bound, name
