"""CPU: the host surface of the one-plane LSTM recurrence step (DESIGN I.31, csrc/lstm_w1.hip) — the one-plane packer against the
three-plane one, a lane-level replay of the kernel's addressing in the style of tests/test_lstm_split_layout_model.py, the two library
entries and their answers that need no GPU (they come before any HIP call), and the `lstm_w1` knob."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd.codec import wmencodec as WM
from test_lstm_split_layout_model import frag_block, produce_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssrhip_lstm_layer_w1", "ssrhip_lstm_w1_launches")
LSTM_W1_DEFAULT = "1"            # DESIGN.md Part I.31: the measurement met its gate (profiles/lstm_w1_ab.md)
H_PIECES = (2, 1, 0)             # the h pieces plane 0 of W_hh meets, in the kernel's order (PB of lstm_step_w1_kernel)


def exact_split(w: torch.Tensor) -> torch.Tensor:
    """ssrhip_split_weights on the host: w = p0 + p1 + p2 with p_q = bf16_rne of what is left; int16 bit patterns [3][...]"""
    planes, rest = [], w.clone()
    for _ in range(3):
        p = rest.to(torch.bfloat16)
        planes.append(p.view(torch.int16))
        rest = rest - p.float()
    assert not rest.any()
    return torch.stack(planes)


@pytest.mark.parametrize("Cc", [128, 256, 512])
def test_one_plane_pack_is_plane_0_of_the_three_plane_pack_and_the_other_planes_are_zero(Cc):
    g = torch.Generator().manual_seed(Cc)
    w = (torch.randn(4 * Cc, Cc, generator=g) / Cc ** 0.5).to(torch.bfloat16)          # a matrix of bf16 values
    planes = exact_split(w.float())
    assert not planes[1].any() and not planes[2].any()                                 # what the three-plane step streams and multiplies
    three = WM.pack_lstm_whh_planes(planes)                                            # ub, w, s, mb, q, lh, li, e
    one = WM.pack_lstm_whh_plane(w)
    assert one.dtype == torch.bfloat16 and one.is_contiguous() and tuple(one.shape) == (Cc // 16, 4, Cc // 64, 2, 2, 32, 8)
    assert torch.equal(one.view(torch.int16), three[:, :, :, :, 0])
    assert not three[:, :, :, :, 1:].any()
    assert one.numel() * 3 == three.numel()


def w1_block(ub, wave, ks, s, mb):                                  # lstm_w1.hip w1_block(): in bf16 elements
    return (((ub * 4 + wave) * ks + s) * 2 + mb) * 512


def replay_w1_kernel(wflat, hflat, B, C):
    """gates[b][g C + j] as lstm_step_w1_kernel's workgroups compute them (without gin), and how many (W element, h element) pairs a lane
    multiplies whose k indices differ: the block address + lane * 8 + element on both sides, decoded back through the two layouts"""
    ks, nbg = C // 64, (B + 63) // 64
    gates = np.zeros((nbg * 64, 4 * C))
    for ub in range(C // 16):
        for bg in range(nbg):
            D = np.zeros((64, 64))
            for wave in range(4):
                for s in range(ks):
                    for qb in H_PIECES:
                        for mb in range(2):
                            for nb in range(2):
                                a0, b0 = w1_block(ub, wave, ks, s, mb), frag_block(bg, wave, ks, s, nb, qb)
                                A = wflat[a0:a0 + 512].reshape(2, 32, 8)           # [lh][li][e]: lane = 32 lh + li, 8 elements per lane
                                Bm = hflat[b0:b0 + 512].reshape(2, 32, 8)
                                D[mb * 32:mb * 32 + 32, nb * 32:nb * 32 + 32] += np.einsum("hme,hne->mn", A, Bm)
            for m in range(64):
                g, u = divmod(m, 16)
                gates[bg * 64:bg * 64 + 64, g * C + ub * 16 + u] = D[m, :]
    return gates


@pytest.mark.parametrize("B,C", [(70, 128), (64, 256)])
def test_the_one_plane_w_block_a_lane_reads_pairs_with_the_h_blocks_it_reads(B, C):
    """The W operand tagged with its own k index, h tagged with its k index (planes q: k + 1000 q): every lane of every block of every
    k-step must read W[.][k] beside h[.][k] — 0 mismatches — and with small integers the gates are the three products' exact sum."""
    ks, nbg = C // 64, (B + 63) // 64
    ktag = torch.arange(C, dtype=torch.float32).repeat(4 * C, 1)                       # W[r][k] = k (all bf16 values for C <= 256)
    wk = WM.pack_lstm_whh_plane(ktag.to(torch.bfloat16)).float().numpy().reshape(-1)
    hk = produce_h([np.tile(np.arange(C, dtype=np.float64), (B, 1)) + 1000 * q for q in range(3)], B, C)
    mismatches = 0
    for ub in range(C // 16):
        for wave in range(4):
            for s in range(ks):
                for mb in range(2):
                    A = wk[w1_block(ub, wave, ks, s, mb):][:512].reshape(2, 32, 8)
                    assert np.array_equal(A, np.broadcast_to((wave * (C // 4) + 16 * s + 8 * np.arange(2)[:, None, None] + np.arange(8)), (2, 32, 8)))
                    for nb in range(2):
                        for q in H_PIECES:
                            Bm = hk[frag_block(0, wave, ks, s, nb, q):][:512].reshape(2, 32, 8)
                            mismatches += int((A[:, :1, :] + 1000 * q != Bm).sum())     # bg = 0 holds 64 full rows in both shapes
    assert mismatches == 0
    rng = np.random.default_rng(B + C)
    w0 = rng.integers(-3, 4, size=(4 * C, C)).astype(np.float64)
    hq = [rng.integers(-3, 4, size=(B, C)).astype(np.float64) for _ in range(3)]
    packed = WM.pack_lstm_whh_plane(torch.from_numpy(w0).to(torch.bfloat16))
    gates = replay_w1_kernel(packed.float().numpy().astype(np.float64).reshape(-1), produce_h(hq, B, C), B, C)
    assert np.array_equal(gates[:B], sum(hq[q] @ w0.T for q in H_PIECES))
    assert not gates[B:].any()                                                         # batch rows past B: their h planes stay zero
    assert nbg == (2 if B > 64 else 1)


def test_packer_rejects_what_the_kernel_cannot_take():
    with pytest.raises(AssertionError):
        WM.pack_lstm_whh_plane(torch.zeros(4 * 48, 48, dtype=torch.bfloat16))
    with pytest.raises(AssertionError):
        WM.pack_lstm_whh_plane(torch.zeros(4 * 128, 128, dtype=torch.float32))            # the values have to BE bf16 values


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ssrhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in bound, name
        assert getattr(raw, name) is not None
    assert _lib.lib().ssrhip_version() == 107 == _lib.ABI_VERSION                      # no struct changed


def _fake_lstm(B=64, Cc=256, T=4):
    """launch arguments whose pointers are never dereferenced: every call made with them here is answered before any HIP call"""
    a = _lib.LstmArgs()
    a.gin, a.w_hh, a.out, a.hbuf, a.cbuf = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.w_split, a.hsplit = 0x6000, 0x7000
    a.B, a.T, a.C = B, T, Cc
    a.gin_bstride, a.out_bstride, a.skip_bstride = T * 4 * Cc, T * Cc, T * Cc
    return a


def test_contract_errors_need_no_gpu_and_are_negative():
    L = _lib.lib()
    assert L.ssrhip_lstm_layer_w1(None, None) < 0 and b"ssrhip_lstm_layer_w1: null argument" in L.ssrhip_last_error()
    for drop in ("gin", "w_hh", "out", "hbuf", "cbuf"):
        a = _fake_lstm()
        setattr(a, drop, 0)
        assert L.ssrhip_lstm_layer_w1(C.byref(a), None) < 0 and b"null argument" in L.ssrhip_last_error(), drop
    for drop in (("w_split",), ("hsplit",), ("w_split", "hsplit")):                   # half-set pointers, and none: this entry has no other path
        a = _fake_lstm()
        for d in drop:
            setattr(a, d, 0)
        assert L.ssrhip_lstm_layer_w1(C.byref(a), None) < 0 and b"w_split and hsplit" in L.ssrhip_last_error(), drop
    for t0, t1 in ((-1, 2), (2, 2), (3, 2), (0, 5)):
        a = _fake_lstm()
        a.t_begin, a.t_end = t0, t1
        assert L.ssrhip_lstm_layer_w1(C.byref(a), None) < 0 and b"bad time window" in L.ssrhip_last_error(), (t0, t1)
    a = _fake_lstm(Cc=200)
    assert L.ssrhip_lstm_layer_w1(C.byref(a), None) < 0                                # C % 16, as ssrhip_lstm_layer


def test_answer_1_launches_nothing_and_counts_nothing():
    L = _lib.lib()
    n0, c0 = L.ssrhip_lstm_w1_launches(), L.ssrhip_codec_w1_launches()
    for kw in (dict(B=31), dict(Cc=192), dict(B=4, Cc=512), dict(B=1, Cc=256), dict(B=31, Cc=128), dict(Cc=64)):
        assert L.ssrhip_lstm_layer_w1(C.byref(_fake_lstm(**kw)), None) == 1, kw
    assert L.ssrhip_lstm_w1_launches() == n0 and L.ssrhip_codec_w1_launches() == c0    # launches, not calls


def test_the_knob_is_in_the_table_and_unset_means_the_documented_default():
    row = [k for k in WM._ENV_KNOBS if k[0] == "lstm_w1"]
    assert len(row) == 1
    attr, switch, unset, parse = row[0]
    assert switch == "SSRHIP_LSTM_W1" and unset == LSTM_W1_DEFAULT
    assert parse("1") is True and parse("") is True and parse("0") is False            # as SSRHIP_CODEC_W1: off iff "0"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "SSRHIP_LSTM_W1" in doc and "SSRHIP_LSTM_W1_DEPTH" in doc
    row = [ln for ln in doc.splitlines() if ln.startswith("| `SSRHIP_LSTM_W1=1`")]
    assert len(row) == 1 and row[0].split("|")[2].strip() == LSTM_W1_DEFAULT, row      # §4's "unset" column names the same default


def test_the_knob_is_ignored_for_an_fp32_model_without_codec_w1_and_without_the_split_step():
    m = object.__new__(WM.WMEncodecModel)                                             # the property reads four attributes and nothing else
    for wdt, w1, split, knob, want in (("bf16", True, True, True, True), ("bf16", True, True, False, False), ("fp32", True, True, True, False),
                                       ("bf16", False, True, True, False), ("bf16", True, False, True, False), ("fp32", False, True, True, False)):
        m.weight_dtype, m.codec_w1, m.lstm_split, m.lstm_w1 = wdt, w1, split, knob
        assert m.lstm_one_plane is want, (wdt, w1, split, knob)


class _Recorder:
    """stands in for the library: records the entry and what it was handed, answers as told"""

    def __init__(self, w1_answer):
        self.calls, self.w1_answer = [], w1_answer

    def __getattr__(self, name):
        def entry(ref, stream):
            a = ref._obj
            self.calls.append((name, int(a.w_split or 0), int(a.hsplit or 0)))
            return self.w1_answer if name == "ssrhip_lstm_layer_w1" else 0
        return entry


class _Buf:
    def __init__(self, ptr, dtype=None):
        self.ptr, self.dtype = ptr, dtype

    def data_ptr(self):
        return self.ptr


@pytest.mark.parametrize("dtype,answer,want", [
    (torch.bfloat16, 0, [("ssrhip_lstm_layer_w1", 0x60, 0x70)]),
    (torch.bfloat16, 1, [("ssrhip_lstm_layer_w1", 0x60, 0x70), ("ssrhip_lstm_layer", 0, 0)]),      # answer 1: the fp32 pipe, WITHOUT planes
    (torch.int16, 0, [("ssrhip_lstm_layer", 0x60, 0x70)]),                                         # three planes: today's entry
])
def test_lstm_steps_picks_the_entry_from_the_buffer_it_holds(monkeypatch, dtype, answer, want):
    """Never a one-plane buffer in the three-plane entry: the dtype of the pack decides, whatever the knob says now."""
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    m = object.__new__(WM.WMEncodecModel)
    m.lib, m.n_launches, m.lstm_packed, m.lstm_w1 = _Recorder(answer), 0, True, dtype != torch.bfloat16     # the knob says the opposite
    Lq = object.__new__(WM._Lstm)
    Lq.C, Lq.layers, Lq.packed, Lq.split = 256, [(None, _Buf(0x10), None)], [_Buf(0x20)], [_Buf(0x60, dtype)]
    m._lstm_steps(Lq, 0, _Buf(0x30), _Buf(0x40), _Buf(0x50), _Buf(0x70), 0x80, 1024, 0, 0, 64, 4, 0, 4, False)
    assert m.lib.calls == want
    m.lib.calls.clear()
    m._lstm_steps(Lq, 0, _Buf(0x30), _Buf(0x40), _Buf(0x50), None, 0x80, 1024, 0, 0, 64, 4, 0, 4, False)    # no hsplit: no planes at all
    assert m.lib.calls == [("ssrhip_lstm_layer", 0, 0)]
