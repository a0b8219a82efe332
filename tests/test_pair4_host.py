"""CPU: the host side of the opt-in pair launches of the 4-row decode step (DESIGN.md Part I.24) — the pure rule behind DecodeEngine's
`pair4`, the new names in the binding and the header, the workspace size on both sides, and the contract errors of `ssrhip_gemv_pair4`,
which are answered before any HIP call (fake pointers, never dereferenced)."""
import ctypes as C
import os
import re

import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E
from ssr_speech_amd.engine import PAIR4_DEFAULT, PAIR4_WS_BYTES, resolve_pair4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssrhip_gemv_pair4", "ssrhip_gemv_pair4_applicable", "ssrhip_gemv_pair4_status", "ssrhip_lm_set_pair4", "ssrhip_lm_pair4_launches")


def test_resolve_pair4_truth_table():
    """requested None: on iff 4 rows, no packed stream, pair_mode != 1 and the switch (unset = PAIR4_DEFAULT = off) does not start with
    '0'. False: off. True: on, or a ValueError — another row count is named first, then the packed stream, then pair_mode 1."""
    assert PAIR4_DEFAULT == "0"
    for rows in (1, 2, 4, 5, 16, 32):
        for w16, w8 in ((False, False), (True, False), (False, True)):
            for pair_mode in (0, 1, 2):
                for value in (None, "0", "1", "01", "2"):
                    env = {"SSRHIP_GEMV_PAIR": "0", "SSRHIP_GEMV_W16_PAIR": "1", "SSRHIP_GEMV_W8_PAIR": "1"}      # other switches are not looked at
                    if value is not None:
                        env["SSRHIP_GEMV_PAIR4"] = value
                    case = (rows, w16, w8, pair_mode, value)
                    ok = rows == 4 and not w16 and not w8 and pair_mode != 1
                    want = ok and value is not None and value[0] != "0"
                    assert resolve_pair4(rows, w16, w8, pair_mode, None, env) is want, case
                    assert resolve_pair4(rows, w16, w8, pair_mode, False, env) is False, case
                    if ok:
                        assert resolve_pair4(rows, w16, w8, pair_mode, True, env) is True, case      # asked for: the switch is not read
                        continue
                    with pytest.raises(ValueError) as err:
                        resolve_pair4(rows, w16, w8, pair_mode, True, env)
                    msg = str(err.value)
                    if rows != 4:
                        assert msg == f"pair4: the 4-row pair launches exist for the 4-row decode step only (this engine has {rows} rows)", case
                    elif w16 or w8:
                        assert "read fp32 weights" in msg and ("stream_w16" if w16 else "stream_w8") in msg and ("bf16" if w16 else "e4m3") in msg, case
                    else:
                        assert msg == "pair4 with pair_mode=1: the caller switched pair launches off", case


def test_resolve_pair4_reads_nothing_but_its_arguments(monkeypatch):
    monkeypatch.setenv("SSRHIP_GEMV_PAIR4", "1")                 # the process environment is not what the rule reads
    assert resolve_pair4(4, False, False, 0, None, {}) is False
    assert resolve_pair4(4, False, False, 0, None, {"SSRHIP_GEMV_PAIR4": "1"}) is True


def test_workspace_bytes_agree_between_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    m = re.search(r"#define SSRHIP_PAIR4_WS_BYTES \((\d+) \* (\d+) \* (\d+) \+ (\d+)\)", hdr)
    assert m, "SSRHIP_PAIR4_WS_BYTES not found in include/ssrhip.h"
    a, b, c, d = (int(x) for x in m.groups())
    assert (a, b, c, d) == (3, 8192, 8, 64)                      # three buffers of 4 x 2048 8-byte granules + the give-up flag's line
    assert a * b * c + d == PAIR4_WS_BYTES == E.PAIR4_WS_BYTES
    two = re.search(r"#define SSRHIP_PAIR_WS_BYTES \((\d+) \* (\d+) \* (\d+) \+ (\d+)\)", hdr)
    assert two and [int(x) for x in two.groups()] == [3, 4096, 8, 64]         # the 2-row workspace keeps its size
    assert re.search(r"#define SSRHIP_VERSION 107\b", hdr) and _lib.ABI_VERSION == 107     # additions only: the ABI version stays


def test_new_names_are_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in bound, name


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
    ws = C.c_void_p(0x4000)
    assert lib.ssrhip_gemv_pair4(None, C.byref(b), ws, 0, 1, None) < 0 and b"null argument" in lib.ssrhip_last_error()
    assert lib.ssrhip_gemv_pair4(C.byref(a), C.byref(b), None, 0, 1, None) < 0 and b"null argument" in lib.ssrhip_last_error()
    for buf, nxt in ((0, 0), (3, 0), (0, -1)):
        assert lib.ssrhip_gemv_pair4(C.byref(a), C.byref(b), ws, buf, nxt, None) < 0 and b"granule buffers" in lib.ssrhip_last_error(), (buf, nxt)
    b16 = _fake(4, 6144, 2048, pro=_lib.PRO_LAYERNORM, epi=_lib.EPI_QKV_APPEND16)
    assert lib.ssrhip_gemv_pair4(C.byref(a), C.byref(b16), ws, 0, 1, None) < 0 and b"EPI_QKV_APPEND16" in lib.ssrhip_last_error()
    assert lib.ssrhip_gemv_pair4_status(None, None) < 0 and b"null workspace" in lib.ssrhip_last_error()
    assert lib.ssrhip_gemv_pair4_applicable(None, C.byref(b)) == 0
