"""GPU: the one-plane LSTM recurrence step (DESIGN I.31) — `ssrhip_lstm_layer_w1` / `lstm_step_w1_kernel` (csrc/lstm_w1.hip) and the codec
wired to it.

A recurrent matrix that IS a matrix of bf16 values splits exactly into itself and two planes of zeros. `lstm_step_split_kernel` streams
the three planes and issues six matrix products per k-step, three of them against zeros; the one-plane step streams the one plane and
issues the other three in the same order, and shares every line outside its k-loop with the three-plane step. The claim is IDENTITY:
`torch.equal` on whole poisoned buffers — `out`, `cbuf` and both `hsplit` buffers — from one launch up to every entry point of a
full-size codec, with the two entries taking turns inside one sequence. Both are also held to the fp64 cell within the three-plane
kernel test's bound. Every weight here is rounded to bf16; every activation is finite."""
import ctypes as C
import math
import os

import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel, pack_lstm_whh_plane, pack_lstm_whh_planes
from helpers_codec import lstm_ref, pack_whh

pytestmark = pytest.mark.gpu

POISON = -777.25
PAD = 64                      # poisoned floats behind `out`
TOL = 2e-5                    # tests/test_gpu_kernels.py::test_lstm_split_step_matches_fp64's bound
NAN16 = 0x7FC0                # a bf16 NaN in every piece of h: the library has to zero `hsplit` at t = 0
SHAPES = [(70, 128, 6),       # KS = 2: DEPTH 2; a second batch group that is not full
          (64, 256, 4),       # KS = 4: DEPTH 4
          (33, 512, 3),       # KS = 8: DEPTH 4 here, DEPTH 8 in a test of its own below
          (33, 1024, 3)]      # KS = 16
EPILOGUES = [(False, 0), (True, _lib.ACT_ELU)]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def _case(B, Cc, T, skip, out_act):
    """seeded layer: W_hh = randn / sqrt(C) rounded to bf16, its three-plane and one-plane packs on the device, gin, the skip input, and the
    fp64 cell's output"""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(B + Cc + T + int(skip))
    whh = (torch.randn(4 * Cc, Cc, generator=g) / math.sqrt(Cc)).to(torch.bfloat16).float()
    gin = torch.randn(B, T, 4 * Cc, generator=g)
    xs = torch.randn(B, T, Cc, generator=g)
    want = lstm_ref(gin, whh, xs if skip else None, bool(out_act))
    dw = whh.cuda()
    planes = torch.empty(3, 4 * Cc, Cc, dtype=torch.int16, device="cuda")
    _lib.check(lib.ssrhip_split_weights(dw.data_ptr(), planes.data_ptr(), dw.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert not bool(planes[1:].any())                                      # the planes the three-plane step streams for nothing
    three = pack_lstm_whh_planes(planes)
    one = pack_lstm_whh_plane(dw.to(torch.bfloat16))
    assert torch.equal(one.view(torch.int16), three[:, :, :, :, 0]) and one.numel() * 3 == three.numel()
    return dict(B=B, C=Cc, T=T, skip=skip, out_act=out_act, want=want, gin=gin.cuda(), xs=xs.cuda(), packed=pack_whh(whh).cuda(),
                three=three, one=one)


def _state(c):
    B, Cc, T = c["B"], c["C"], c["T"]
    return dict(out=torch.full((B * T * Cc + PAD,), POISON, device="cuda"), cbuf=torch.full((B, Cc), float("nan"), device="cuda"),
                hbuf=torch.zeros(2, (B + 15) // 16 * 16, Cc, device="cuda"),
                hs=torch.full((2 * ((B + 63) // 64) * 64 * Cc * 3,), NAN16, dtype=torch.int16, device="cuda"))


def _args(c, st, t0, t1, one_plane):
    B, Cc, T = c["B"], c["C"], c["T"]
    a = _lib.LstmArgs()
    a.gin, a.w_hh, a.out = c["gin"].data_ptr(), c["packed"].data_ptr(), st["out"].data_ptr()
    a.w_packed = 1
    a.skip = c["xs"].data_ptr() if c["skip"] else 0
    a.hbuf, a.cbuf, a.gates = st["hbuf"].data_ptr(), st["cbuf"].data_ptr(), 0
    a.B, a.T, a.C = B, T, Cc
    a.gin_bstride, a.out_bstride, a.skip_bstride = T * 4 * Cc, T * Cc, T * Cc
    a.t_begin, a.t_end, a.out_act = t0, t1, c["out_act"]
    a.w_split, a.hsplit = (c["one"] if one_plane else c["three"]).data_ptr(), st["hs"].data_ptr()
    return a


def _run(L, c, entries):
    """the two time windows [0, T/2), [T/2, T) through `entries` (True = the one-plane entry) on ONE set of state buffers, NaN-filled /
    poisoned beforehand -> (state, one-plane step launches counted)"""
    st = _state(c)
    T = c["T"]
    n0 = L.ssrhip_lstm_w1_launches()
    for (t0, t1), one_plane in zip(((0, T // 2), (T // 2, T)), entries):
        a = _args(c, st, t0, t1, one_plane)
        rc = (L.ssrhip_lstm_layer_w1 if one_plane else L.ssrhip_lstm_layer)(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (rc, L.ssrhip_last_error())
    torch.cuda.synchronize()
    return st, L.ssrhip_lstm_w1_launches() - n0


def _same(x, y):
    return all(torch.equal(x[k], y[k]) for k in ("out", "cbuf", "hs"))


@pytest.mark.parametrize("skip,out_act", EPILOGUES, ids=["plain", "skip-elu"])
@pytest.mark.parametrize("B,Cc,T", SHAPES, ids=[f"{b}-{c}-{t}" for b, c, t in SHAPES])
def test_one_plane_step_is_the_three_plane_step_bit_for_bit(L, B, Cc, T, skip, out_act):
    """Two time windows each; whole buffers: `out` with its poisoned pad, `cbuf`, both `hsplit` buffers (NaN-filled beforehand, so the
    t = 0 zeroing shows). Both within 2e-5 of the fp64 cell: a failure of BOTH points at the inputs. The counter counts the one-plane
    steps and nothing else. Then the windows mixed: three-plane then one-plane and the other way round on the same hsplit / cbuf equal
    the single-entry runs — the state format is one and the same."""
    c = _case(B, Cc, T, skip, out_act)
    s3, n3 = _run(L, c, (False, False))
    s1, n1 = _run(L, c, (True, True))
    got3, got1 = (s["out"][:B * T * Cc].view(B, T, Cc).cpu().double() for s in (s3, s1))
    e3, e1 = float((got3 - c["want"]).abs().max()), float((got1 - c["want"]).abs().max())
    print(f"B={B} C={Cc} T={T} skip={skip}: max |three planes - fp64| = {e3:.3e}, max |one plane - fp64| = {e1:.3e}, "
          f"max |one - three| = {float((got1 - got3).abs().max()):.3e}")
    assert (n3, n1) == (0, T)                                              # launches: one per step of the one-plane calls
    assert torch.equal(s1["out"], s3["out"]) and bool((s1["out"][B * T * Cc:] == POISON).all())
    assert torch.equal(s1["cbuf"], s3["cbuf"]) and torch.isfinite(s1["cbuf"]).all()
    assert torch.equal(s1["hs"], s3["hs"]) and not bool((s1["hs"] == NAN16).any())
    torch.testing.assert_close(got3, c["want"], rtol=TOL, atol=TOL)
    torch.testing.assert_close(got1, c["want"], rtol=TOL, atol=TOL)
    for entries in ((False, True), (True, False)):
        sm, nm = _run(L, c, entries)
        assert _same(sm, s3), entries
        assert nm == (T - T // 2 if entries[1] else T // 2), (entries, nm)


@pytest.mark.parametrize("skip,out_act", EPILOGUES, ids=["plain", "skip-elu"])
def test_depth_8_arm_is_the_three_plane_step_bit_for_bit(L, monkeypatch, skip, out_act):
    """SSRHIP_LSTM_W1_DEPTH=8 at KS = 8 (the codec's own C = 512): eight k-steps in flight, ONE trip through the k-loop. The launcher
    reads the switch at every call, so it is set for this test alone. Same bits as the three-plane step — alone and as the second window
    behind it — and within 2e-5 of fp64."""
    B, Cc, T = 33, 512, 3
    c = _case(B, Cc, T, skip, out_act)
    s3, _ = _run(L, c, (False, False))
    monkeypatch.setenv("SSRHIP_LSTM_W1_DEPTH", "8")
    s1, n1 = _run(L, c, (True, True))
    sm, nm = _run(L, c, (False, True))
    assert (n1, nm) == (T, T - T // 2)
    assert _same(s1, s3) and _same(sm, s3)
    assert bool((s1["out"][B * T * Cc:] == POISON).all()) and not bool((s1["hs"] == NAN16).any())
    torch.testing.assert_close(s1["out"][:B * T * Cc].view(B, T, Cc).cpu().double(), c["want"], rtol=TOL, atol=TOL)


@pytest.mark.parametrize("B,Cc", [(31, 128), (64, 192), (4, 512)], ids=["B31", "C192", "small-batch"])
def test_a_shape_that_does_not_qualify_answers_1_and_touches_nothing(L, B, Cc):
    """What ssrhip_lstm_split_eligible rejects, and the small-batch shapes: answer 1, `out` and `hsplit` whole and poisoned, the counter
    where it was — and the call the caller makes next (ssrhip_lstm_layer WITHOUT planes) is within 2e-5 of fp64."""
    T = 3
    g = torch.Generator().manual_seed(B + Cc)
    whh = (torch.randn(4 * Cc, Cc, generator=g) / math.sqrt(Cc)).to(torch.bfloat16).float()
    gin = torch.randn(B, T, 4 * Cc, generator=g)
    small_b = B <= 4
    c = dict(B=B, C=Cc, T=T, skip=False, out_act=0, gin=gin.cuda(), xs=None, packed=(whh if small_b else pack_whh(whh)).cuda(),
             one=torch.zeros(4 * Cc * Cc, dtype=torch.bfloat16, device="cuda"))
    st = _state(c)
    a = _args(c, st, 0, T, True)
    a.w_packed = 0 if small_b else 1
    n0 = L.ssrhip_lstm_w1_launches()
    assert L.ssrhip_lstm_layer_w1(C.byref(a), _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((st["out"] == POISON).all()) and bool((st["hs"] == NAN16).all()) and L.ssrhip_lstm_w1_launches() == n0
    a.w_split = a.hsplit = 0
    _lib.check(L.ssrhip_lstm_layer(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    torch.testing.assert_close(st["out"][:B * T * Cc].view(B, T, Cc).cpu().double(), lstm_ref(gin, whh, None, False), rtol=TOL, atol=TOL)
    assert bool((st["out"][B * T * Cc:] == POISON).all()) and bool((st["hs"] == NAN16).all())


def test_half_set_pointers_are_a_contract_error(L):
    c = _case(64, 256, 4, False, 0)
    st = _state(c)
    for drop in ("w_split", "hsplit"):
        a = _args(c, st, 0, 4, True)
        setattr(a, drop, 0)
        assert L.ssrhip_lstm_layer_w1(C.byref(a), _lib.stream_ptr()) < 0, drop
    torch.cuda.synchronize()
    assert bool((st["out"] == POISON).all())


# ------------------------------------------------------------------------------------------ the whole codec, full config
SEED = 17


def _plane_bytes(m):
    return sum(t.numel() * t.element_size() for v in m._plane_cache.values() for t in (v if isinstance(v, tuple) else (v,)))


def _build(cfg, sd, knob):
    assert "SSRHIP_LSTM_W1" not in os.environ
    os.environ["SSRHIP_LSTM_W1"] = knob
    try:
        m = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
    finally:
        del os.environ["SSRHIP_LSTM_W1"]
    m.lstm_split_min_b = 1               # as tests/test_gpu_codec.py::test_large_batch_kernels_match_the_oracle_directly forces the split step
    return m


@pytest.fixture(scope="module")
def pair(L):
    """A: bf16 with the one-plane step, A': bf16 with SSRHIP_LSTM_W1=0 while it is built; their outputs on 33 x 0.3 s and on 33 x 1.5 s
    (75 frames > LSTM_CHUNK: the second layer's windows, t_begin = 64 among them, run on the side stream) — computed once."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=SEED)
    models = {"A": _build(cfg, sd, "1"), "A'": _build(cfg, sd, "0")}
    assert models["A"].lstm_one_plane and not models["A'"].lstm_one_plane and models["A"].one_plane and models["A'"].one_plane
    g = torch.Generator().manual_seed(SEED)
    sr = cfg.sample_rate
    wavs = {"33x0.3s": (torch.randn(33, 1, int(0.3 * sr), generator=g) * 0.3).cuda(), "33x1.5s": (torch.randn(33, 1, int(1.5 * sr), generator=g) * 0.3).cuda()}
    outs, launches, codes, labels = {}, {}, {}, {}
    for name, m in models.items():
        n0 = L.ssrhip_lstm_w1_launches()
        o = {}
        for t, w in wavs.items():
            c, _, emb = m.encode(w)
            o[f"{t}.codes"], o[f"{t}.emb"] = c.clone(), emb.clone()
            if t not in codes:                                             # both models decode the SAME codes
                codes[t] = c.clone()
                labels[t] = torch.randint(0, 2, (c.shape[0], c.shape[-1]), generator=g).cuda()
            o[f"{t}.decode"] = m.decode(codes[t]).clone()
            wm_wav, mark = m.wmdecode(codes[t], labels[t], w[..., : codes[t].shape[-1] * cfg.hop])
            o[f"{t}.wmdecode"], o[f"{t}.mark"] = wm_wav.clone(), mark.clone()
        torch.cuda.synchronize()
        outs[name], launches[name] = o, L.ssrhip_lstm_w1_launches() - n0
    return dict(cfg=cfg, models=models, outs=outs, launches=launches, codes=codes)


def test_whole_codec_one_plane_step_equals_three_plane_step(pair):
    a, b = pair["outs"]["A"], pair["outs"]["A'"]
    assert sorted(a) == sorted(b) and len(a) == 2 * 5
    assert pair["codes"]["33x1.5s"].shape[-1] == 75 > WMEncodecModel.LSTM_CHUNK
    for k in sorted(a):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))
        assert torch.isfinite(a[k].double()).all(), k


def test_whole_codec_takes_the_one_plane_step_and_only_where_asked(pair):
    n, m = pair["launches"], pair["models"]
    print("one-plane LSTM step launches per model:", n)
    assert n["A"] > 0 and n["A'"] == 0
    assert m["A"].mallocs_in_flight == 0 and m["A'"].mallocs_in_flight == 0
    for name, dtype in (("A", torch.bfloat16), ("A'", torch.int16)):
        packs = [p for net in (m[name].encoder, m[name].decoder, m[name].skip_encoder) for _, kind, obj, _ in net.nodes if kind == "lstm" for p in obj.split]
        assert packs and all(p is not None and p.dtype == dtype for p in packs), name
    # a third of the W_hh bytes, and the plane cache (the GEMMs' planes) is the same on both
    one = [p for _, kind, obj, _ in m["A"].encoder.nodes if kind == "lstm" for p in obj.split]
    three = [p for _, kind, obj, _ in m["A'"].encoder.nodes if kind == "lstm" for p in obj.split]
    assert all(3 * x.numel() == y.numel() for x, y in zip(one, three))
    assert len(m["A"]._plane_cache) == len(m["A'"]._plane_cache) and _plane_bytes(m["A"]) == _plane_bytes(m["A'"])
