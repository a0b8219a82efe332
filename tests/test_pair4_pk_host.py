"""CPU: the host side of the opt-in 4-row pair launches over the packed weight streams (DESIGN.md Part I.26) — the pure rule behind
DecodeEngine's `pair4_pk`, the new names in the binding and the header, the contract errors of `ssrhip_gemv_pair4_w16` /
`ssrhip_gemv_pair4_w8`, which are answered before any HIP call (fake pointers, never dereferenced), and what the older rules keep
answering for 4-row packed engines."""
import ctypes as C
import os
import re

import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd.engine import (PAIR4_DEFAULT, PAIR4_PK_DEFAULT, W8_PAIR_DEFAULT, W16_PAIR_DEFAULT, resolve_pair4, resolve_pair4_pk, resolve_w8_pair,
                                   resolve_w16_pair)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssrhip_gemv_pair4_w16", "ssrhip_gemv_pair4_w16_applicable", "ssrhip_gemv_pair4_w8", "ssrhip_gemv_pair4_w8_applicable",
       "ssrhip_lm_set_pair4_pk", "ssrhip_lm_pair4_pk_launches")


def test_resolve_pair4_pk_truth_table():
    """requested None: on iff 4 rows, a packed stream (w16 or w8), pair_mode != 1 and the switch (unset = PAIR4_PK_DEFAULT = off) does not
    start with '0'. False: off. True: on, or a ValueError — another row count is named first, then the missing stream, then pair_mode 1."""
    assert PAIR4_PK_DEFAULT == "0"
    for rows in (1, 2, 4, 5, 16, 32):
        for w16, w8 in ((False, False), (True, False), (False, True)):
            for pair_mode in (0, 1, 2):
                for value in (None, "0", "1", "01", "2"):
                    env = {"SSRHIP_GEMV_PAIR": "0", "SSRHIP_GEMV_PAIR4": "1", "SSRHIP_GEMV_W16_PAIR": "1", "SSRHIP_GEMV_W8_PAIR": "1"}   # other switches are not looked at
                    if value is not None:
                        env["SSRHIP_GEMV_PAIR4_PK"] = value
                    case = (rows, w16, w8, pair_mode, value)
                    ok = rows == 4 and (w16 or w8) and pair_mode != 1
                    want = ok and value is not None and value[0] != "0"
                    assert resolve_pair4_pk(rows, w16, w8, pair_mode, None, env) is want, case
                    assert resolve_pair4_pk(rows, w16, w8, pair_mode, False, env) is False, case
                    if ok:
                        assert resolve_pair4_pk(rows, w16, w8, pair_mode, True, env) is True, case      # asked for: the switch is not read
                        continue
                    with pytest.raises(ValueError) as err:
                        resolve_pair4_pk(rows, w16, w8, pair_mode, True, env)
                    msg = str(err.value)
                    if rows != 4:
                        assert msg == f"pair4_pk: the 4-row pair launches exist for the 4-row decode step only (this engine has {rows} rows)", case
                    elif not (w16 or w8):
                        assert msg.startswith("pair4_pk needs an engine that streams packed weights") and "stream_w16" in msg and "stream_w8" in msg, case
                    else:
                        assert msg == "pair4_pk with pair_mode=1: the caller switched pair launches off", case


def test_resolve_pair4_pk_reads_nothing_but_its_arguments(monkeypatch):
    monkeypatch.setenv("SSRHIP_GEMV_PAIR4_PK", "1")              # the process environment is not what the rule reads
    assert resolve_pair4_pk(4, True, False, 0, None, {}) is False
    assert resolve_pair4_pk(4, False, True, 0, None, {}) is False
    assert resolve_pair4_pk(4, True, False, 0, None, {"SSRHIP_GEMV_PAIR4_PK": "1"}) is True
    assert resolve_pair4_pk(4, False, True, 0, None, {"SSRHIP_GEMV_PAIR4_PK": "1"}) is True


def test_the_older_rules_answer_as_before_for_four_row_packed_engines():
    """existing behaviour, restated: a 4-row engine with a packed stream gets neither the fp32 4-row pairs nor the 2-row packed pairs,
    whatever the new switch says"""
    assert (PAIR4_DEFAULT, W16_PAIR_DEFAULT, W8_PAIR_DEFAULT) == ("0", "0", "0")
    env = {"SSRHIP_GEMV_PAIR4": "1", "SSRHIP_GEMV_W16_PAIR": "1", "SSRHIP_GEMV_W8_PAIR": "1", "SSRHIP_GEMV_PAIR4_PK": "1"}
    for w16, w8 in ((True, False), (False, True)):
        assert resolve_pair4(4, w16, w8, 0, None, env) is False
        with pytest.raises(ValueError, match="read fp32 weights"):
            resolve_pair4(4, w16, w8, 0, True, env)
    assert resolve_pair4(4, False, False, 0, None, env) is True                    # the fp32 4-row engine is not the new switch's business
    assert resolve_w16_pair(4, True, 0, None, env) is False and resolve_w8_pair(4, True, 0, None, env) is False
    with pytest.raises(ValueError, match="2-row decode step only"):
        resolve_w16_pair(4, True, 0, True, env)
    with pytest.raises(ValueError, match="2-row decode step only"):
        resolve_w8_pair(4, True, 0, True, env)
    assert resolve_w16_pair(2, True, 0, None, env) is True and resolve_w8_pair(2, True, 0, None, env) is True


def test_new_names_are_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in bound, name
    assert re.search(r"#define SSRHIP_VERSION 107\b", hdr) and _lib.ABI_VERSION == 107     # additions only: the ABI version stays
    assert _lib.lib().ssrhip_version() == 107


def _fake(B, N, K, pro=_lib.PRO_NONE, epi=_lib.EPI_STORE):
    a = _lib.GemvArgs()
    a.W, a.y, a.x = 0x1000, 0x2000, 0x3000
    a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, 1, K, N
    a.pro, a.epi = pro, epi
    return a


def test_contract_errors_come_before_any_hip_call():
    """built library, no GPU needed: a null pointer, granule buffers outside 0..2 or equal, and the 2-byte KV append are < 0 with a text"""
    lib = _lib.lib()
    a, b = _fake(4, 2048, 8192, epi=_lib.EPI_RESIDUAL), _fake(4, 4096, 2048, pro=_lib.PRO_LAYERNORM)
    b16 = _fake(4, 6144, 2048, pro=_lib.PRO_LAYERNORM, epi=_lib.EPI_QKV_APPEND16)
    ws, p = C.c_void_p(0x4000), [C.c_void_p(0x5000 + 0x1000 * i) for i in range(4)]
    pa, pb = C.byref(a), C.byref(b)
    w16 = lambda *args: lib.ssrhip_gemv_pair4_w16(*args)
    w8 = lambda *args: lib.ssrhip_gemv_pair4_w8(*args)
    for who, call, full in ((b"ssrhip_gemv_pair4_w16", w16, [pa, pb, p[0], p[1], ws, 0, 1, None]),
                            (b"ssrhip_gemv_pair4_w8", w8, [pa, pb, p[0], p[1], p[2], p[3], ws, 0, 1, None])):
        n_ptr = len(full) - 3
        for i in range(n_ptr):                                   # each pointer in turn: the descriptors, the packed weights, the scales, the workspace
            args = list(full)
            args[i] = None
            assert call(*args) < 0, (who, i)
            err = lib.ssrhip_last_error()
            assert who in err and b"null argument" in err, (who, i, err)
        for buf, nxt in ((0, 0), (3, 0), (0, -1)):
            args = list(full)
            args[n_ptr], args[n_ptr + 1] = buf, nxt
            assert call(*args) < 0 and b"granule buffers" in lib.ssrhip_last_error(), (who, buf, nxt)
        args = list(full)
        args[1] = C.byref(b16)
        assert call(*args) < 0 and b"EPI_QKV_APPEND16" in lib.ssrhip_last_error(), who
    assert lib.ssrhip_gemv_pair4_w16_applicable(None, pb) == 0 and lib.ssrhip_gemv_pair4_w16_applicable(pa, None) == 0
    assert lib.ssrhip_gemv_pair4_w8_applicable(None, pb) == 0 and lib.ssrhip_gemv_pair4_w8_applicable(pa, None) == 0
    assert lib.ssrhip_lm_set_pair4_pk(None, 1) < 0 and b"null engine" in lib.ssrhip_last_error()
    assert lib.ssrhip_lm_pair4_pk_launches(None) == 0
