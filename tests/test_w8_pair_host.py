"""CPU: the host side of the opt-in pair launches over the e4m3 weight stream (DESIGN.md Part I.20) — the pure rule behind
DecodeEngine's `pair_w8`, the new names in the binding and the header, and the contract errors of `ssrhip_gemv_pair_w8`, which are
answered before any HIP call (fake pointers, never dereferenced)."""
import ctypes as C
import os
import re

import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import W8_PAIR_DEFAULT, resolve_w8_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssrhip_gemv_pair_w8", "ssrhip_gemv_pair_w8_applicable", "ssrhip_lm_set_w8_pair", "ssrhip_lm_w8_pair_launches")


def test_resolve_w8_pair_truth_table():
    """requested None: on iff 2 rows, the engine streams w8, pair_mode != 1 and the switch (unset = W8_PAIR_DEFAULT = off) does not start
    with '0'. False: off. True: on, or a ValueError — another row count is named first, then the missing stream, then pair_mode 1."""
    assert W8_PAIR_DEFAULT == "0"
    for rows in (1, 2, 4, 16):
        for stream in (False, True):
            for pair_mode in (0, 1, 2):
                for value in (None, "0", "1", "01", "2"):
                    env = {"SSRHIP_GEMV_W8": "0", "SSRHIP_GEMV_PAIR": "0", "SSRHIP_GEMV_W16_PAIR": "1"}      # other switches are not looked at
                    if value is not None:
                        env["SSRHIP_GEMV_W8_PAIR"] = value
                    case = (rows, stream, pair_mode, value)
                    want = rows == 2 and stream and pair_mode != 1 and value is not None and value[0] != "0"
                    assert resolve_w8_pair(rows, stream, pair_mode, None, env) is want, case
                    assert resolve_w8_pair(rows, stream, pair_mode, False, env) is False, case
                    if rows == 2 and stream and pair_mode != 1:
                        assert resolve_w8_pair(rows, stream, pair_mode, True, env) is True, case      # asked for: the switch is not read
                        continue
                    with pytest.raises(ValueError) as err:
                        resolve_w8_pair(rows, stream, pair_mode, True, env)
                    msg = str(err.value)
                    if rows != 2:
                        assert msg == f"pair_w8: pair launches exist for the 2-row decode step only (this engine has {rows} rows)", case
                    elif not stream:
                        assert msg == "pair_w8 needs an engine that streams e4m3 weights (stream_w8)", case
                    else:
                        assert msg == "pair_w8 with pair_mode=1: the caller switched pair launches off", case


def test_new_names_are_in_the_binding_and_the_header():
    names = [s[0] for s in _lib.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert names.count(name) == 1, name
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert hasattr(L, name), name
    sym = dict((s[0], s) for s in _lib.SYMBOLS)
    assert len(sym["ssrhip_gemv_pair_w8"][2]) == 10 and len(sym["ssrhip_gemv_pair_w16"][2]) == 8     # codes AND scales of both matrices
    assert len(sym["ssrhip_gemv_pair_w8_applicable"][2]) == 2
    assert len(sym["ssrhip_lm_set_w8_pair"][2]) == 2 and len(sym["ssrhip_lm_w8_pair_launches"][2]) == 1
    assert L.ssrhip_version() == 107 == _lib.ABI_VERSION                                            # additions only
    assert L.ssrhip_sizeof(16) == -1                                                                # and no new struct


def _pair_args():
    """an (a, b) of the FFN2 form with fake pointers"""
    a, b = _lib.GemvArgs(), _lib.GemvArgs()
    a.W, a.x, a.y = 0x1000, 0x2000, 0x3000
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = 2, 2048, 8192, 1, 8192, 2048
    a.pro, a.act, a.epi = _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL
    b.W, b.x, b.y = 0x4000, 0x3000, 0x5000
    b.B, b.N, b.K, b.groups, b.x_stride, b.y_stride = 2, 4096, 2048, 1, 2048, 4096
    b.pro, b.act, b.epi, b.ln_eps = _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE, 1e-5
    return a, b


PACKED = (0x6000, 0x6800, 0x7000, 0x7800)                        # Wa8, scale_a, Wb8, scale_b


def test_gemv_pair_w8_contract_errors_need_no_gpu():
    L = _lib.lib()
    a, b = _pair_args()
    ws = 0x8000
    err = lambda: L.ssrhip_last_error()
    good = (C.byref(a), C.byref(b)) + PACKED + (ws,)
    for hole in range(len(good)):                                # every pointer argument in turn
        args = good[:hole] + (None,) + good[hole + 1:]
        assert L.ssrhip_gemv_pair_w8(*args, 0, 1, None) < 0, hole
        assert b"ssrhip_gemv_pair_w8: null argument" in err(), hole
    for buf, nxt in ((-1, 0), (3, 0), (0, 3), (0, -1), (1, 1)):
        assert L.ssrhip_gemv_pair_w8(*good, buf, nxt, None) < 0
        assert f"ssrhip_gemv_pair_w8: granule buffers {buf} -> {nxt} (0..2, different)".encode() in err()
    for which in (a, b):
        keep = which.epi
        which.epi = _lib.EPI_QKV_APPEND16
        assert L.ssrhip_gemv_pair_w8(*good, 0, 1, None) < 0
        assert b"ssrhip_gemv_pair_w8: the 2-byte KV append (EPI_QKV_APPEND16) exists for 5..32 rows only" in err()
        which.epi = keep
    assert L.ssrhip_gemv_pair_w8_applicable(None, C.byref(b)) == 0 and L.ssrhip_gemv_pair_w8_applicable(C.byref(a), None) == 0
    # the engine-level setters answer a null engine before anything else
    assert L.ssrhip_lm_set_w8_pair(None, 1) < 0 and b"ssrhip_lm_set_w8_pair: null engine" in err()
    assert L.ssrhip_lm_w8_pair_launches(None) == 0


def test_gemv_pair_w8_never_qualifies_where_gemv_pair_does_not():
    """Whatever device this runs on (none, here): the packed pair never answers yes where the fp32 pair or the single packed launch says no,
    and a shape outside the pair forms answers 1 (nothing launched), not an error."""
    L = _lib.lib()
    a, b = _pair_args()
    ok = L.ssrhip_gemv_pair_w8_applicable(C.byref(a), C.byref(b))
    assert ok in (0, 1)
    if ok:
        assert L.ssrhip_gemv_pair_applicable(C.byref(a), C.byref(b)) == 1
        assert L.ssrhip_gemv_w8_applicable(C.byref(a)) == 1 and L.ssrhip_gemv_w8_applicable(C.byref(b)) == 1
    for change in (dict(B=4), dict(N=5120)):
        a2, b2 = _pair_args()
        for k, v in change.items():
            if k == "B":
                a2.B = b2.B = v
            else:
                setattr(b2, k, v)
                b2.y_stride = v
        assert L.ssrhip_gemv_pair_applicable(C.byref(a2), C.byref(b2)) == 0, change
        assert L.ssrhip_gemv_pair_w8_applicable(C.byref(a2), C.byref(b2)) == 0, change
        assert L.ssrhip_gemv_pair_w8(C.byref(a2), C.byref(b2), *PACKED, 0x8000, 0, 1, None) == 1, change
