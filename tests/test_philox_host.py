"""CPU: the opt-in device-side sampling noise (DESIGN.md Part I.21) as far as it can be checked without a GPU — the numpy replica of the
stream (`ssr_speech_amd/philox.py`: known answers, exact uniforms, element order, distribution, independence of neighbouring streams),
the pure rule and the setter, the CLI flag, the C entry's contract errors and `engine.PhiloxNoise` behind a fake launcher."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib, philox as P
from ssr_speech_amd import engine as E
from ssr_speech_amd import weights as W

K, CARD = 4, 2056


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_known_answers(counter, key, want):
    out = P.philox4x32_10(counter, key)
    assert out.dtype == np.uint32 and out.shape == (4,)
    assert " ".join(f"{int(v):08x}" for v in out) == want


def test_known_answers_in_one_vectorised_call():
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], dtype=np.uint64)
    key = np.array([[0, 0], [0xFFFFFFFF] * 2], dtype=np.uint64)
    out = P.philox4x32_10(ctr, key)
    assert [f"{int(v):08x}" for v in out[0]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert [f"{int(v):08x}" for v in out[1]] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def _philox_scalar(c, k):
    """An independent restatement on Python integers"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _exp_noise_scalar(seed, first_step, n_steps, k, card):
    s = seed & 0xFFFFFFFFFFFFFFFF
    out = np.empty((n_steps, k * card), dtype=np.float64)
    for i in range(n_steps):
        for e in range(k * card):
            w = _philox_scalar((e >> 2, first_step + i, 0x6E6F6973, 0), (s & 0xFFFFFFFF, s >> 32))[e & 3]
            out[i, e] = ((w >> 9) + 0.5) / 2.0 ** 23
    return out.reshape(n_steps, k, card)                     # the uniforms; the caller takes the logarithm


def test_uniforms_are_exact_in_fp32():
    """u = (n + 0.5) * 2^-23 = (2n + 1) * 2^-24: at most 24 significant bits, so the fp32 value is the float64 value — at both ends, around
    the powers of two, and on a million random n"""
    rng = np.random.default_rng(3)
    n = np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 4096, 2 ** 23), 2 ** np.arange(1, 23), 2 ** np.arange(1, 23) - 1,
                        rng.integers(0, 2 ** 23, 1_000_000)]).astype(np.uint32)
    u = P.uniforms(n << np.uint32(9))
    assert np.array_equal(u, (n.astype(np.float64) + 0.5) / 2.0 ** 23)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.array_equal((2.0 * n.astype(np.float32) + 1.0) * np.float32(2.0 ** -24), u.astype(np.float32))      # the device's expression
    assert u.min() > 0 and u.max() < 1
    q = -np.log(P.uniforms(np.array([0, 0xFFFFFFFF], dtype=np.uint32)))
    assert abs(q[0] - 16.6355) < 1e-3 and abs(q[1] - 5.96e-8) < 1e-9          # the range the issue names: finite, strictly positive


@pytest.mark.parametrize("seed, first, n, k, card", [(0, 0, 2, 4, 72), (2 ** 32 + 5, 7, 3, 3, 73), (2 ** 64 - 1, 255, 1, 1, 5)])
def test_exp_noise_equals_the_scalar_loop(seed, first, n, k, card):
    got = P.exp_noise(seed, first, n, k, card)
    assert got.dtype == np.float64 and got.shape == (n, k, card)
    u = _exp_noise_scalar(seed, first, n, k, card)
    assert np.array_equal(P.uniforms(P.words(seed, first, n, k, card)), u)                   # the uniforms: exactly
    want = np.array([-math.log(v) for v in u.reshape(-1)]).reshape(u.shape)
    # two float64 logarithms (numpy's, the C library's), each within an ulp of the true value: 2^-51 relative covers both
    assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -51)
    assert np.array_equal(P.exp_noise32(seed, first, n, k, card), got.astype(np.float32))


def test_element_e_is_word_e_mod_4_of_block_e_div_4_also_when_ragged():
    k, card, seed, step = 3, 73, 11, 5                       # 219 elements: 54 whole blocks and 3 words of the 55th
    w = P.words(seed, step, 1, k, card).reshape(-1)
    assert w.shape == (219,)
    key = P.seed_key(seed)
    for e in (0, 1, 2, 3, 4, 72, 73, 74, 145, 146, 215, 216, 217, 218):
        assert int(w[e]) == int(P.philox4x32_10((e >> 2, step, P.TAG, 0), key)[e & 3]), e
    # the same stream whatever the shape it is cut into: a longer row continues it
    assert np.array_equal(P.words(seed, step, 1, 1, 224).reshape(-1)[:219], w)
    # steps are rows of the counter, not a running offset
    assert np.array_equal(P.words(seed, 3, 4, k, card)[2], P.words(seed, step, 1, k, card)[0])
    assert P.seed_key(2 ** 32 + 5) == (5, 1) and P.seed_key(-1) == (0xFFFFFFFF, 0xFFFFFFFF)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 + 5])
def test_distribution_of_sixteen_steps(seed):
    """Conditions on fixed inputs (measured once: KS 0.0024 / 0.0022 / 0.0014 against the bound 0.0045, |mean - 1| 0.0041 / 0.0011 / 0.0018
    against 0.0083)"""
    q = P.exp_noise(seed, 0, 16, K, CARD).reshape(-1)
    n = q.size
    assert n == 131584
    x = np.sort(q)
    cdf = 1.0 - np.exp(-x)
    i = np.arange(1, n + 1)
    ks = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    assert ks < 1.63 / math.sqrt(n), ks                      # the 1 % level of the Kolmogorov-Smirnov distance
    assert abs(float(q.mean()) - 1.0) < 3.0 / math.sqrt(n), q.mean()
    assert q.min() > 0 and np.isfinite(q).all()


def test_neighbouring_streams_share_no_block():
    s, t = 12345, 9
    blocks = {}
    for name, (seed, step) in dict(a=(s, t), b=(s + 1, t), c=(s, t + 1)).items():
        w = P.words(seed, step, 1, K, CARD).reshape(-1, 4)
        blocks[name] = {tuple(int(v) for v in row) for row in w}
        assert len(blocks[name]) == w.shape[0]               # nor does a stream repeat one
    assert not (blocks["a"] & blocks["b"]) and not (blocks["a"] & blocks["c"]) and not (blocks["b"] & blocks["c"])


# ---------------------------------------------------------------- the rule, the setter, the flag
def test_resolve_sampling_rng():
    assert E.SAMPLING_RNGS == ("torch_cpu", "philox")
    for default in E.SAMPLING_RNGS:
        assert E.resolve_sampling_rng(None, default) == default
        for name in E.SAMPLING_RNGS:
            assert E.resolve_sampling_rng(name, default) == name
    assert E.resolve_sampling_rng(None) == "torch_cpu"
    for bad in ("", "Philox", "cuda", "torch", 1):
        with pytest.raises(ValueError):
            E.resolve_sampling_rng(bad, "torch_cpu")
        with pytest.raises(ValueError):
            E.resolve_sampling_rng(None, bad)


def test_setter_takes_the_two_names_and_drops_nothing():
    from ssr_speech_amd.models.ssr import SSR_Speech
    m = SSR_Speech(W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64))
    assert m.sampling_rng == "torch_cpu"
    sentinel = object()
    m._engines = {"kept": sentinel}                          # the source is a property of a run: the setter leaves the engines alone
    m._arena = sentinel
    for name in ("philox", "torch_cpu", "philox"):
        m.set_sampling_rng(name)
        assert m.sampling_rng == name
    for bad in (None, "", "PHILOX", "device", 0):
        with pytest.raises(ValueError):
            m.set_sampling_rng(bad)
    assert m.sampling_rng == "philox"
    assert m._engines == {"kept": sentinel} and m._arena is sentinel
    m._engines, m._arena = {}, None


def test_cli_flag():
    from ssr_speech_amd import inference_v2 as CLI
    flags = dict(CLI.EXTRA_FLAGS)
    assert flags["--sampling_rng"]["choices"] == ["torch_cpu", "philox"] and flags["--sampling_rng"]["default"] == "torch_cpu"
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampling_rng", **flags["--sampling_rng"])
    assert ap.parse_args([]).sampling_rng == "torch_cpu" and ap.parse_args(["--sampling_rng", "philox"]).sampling_rng == "philox"
    with pytest.raises(SystemExit):
        ap.parse_args(["--sampling_rng", "mt19937"])
    assert CLI.parse_args([]).sampling_rng == "torch_cpu"


# ---------------------------------------------------------------- the C entry: contract errors before any HIP call
def _args(n_seg=1, **seg):
    a = _lib.NoiseArgs()
    a.noise, a.n_utt, a.max_steps, a.K, a.card, a.n_seg = 4096, 5, 40, 4, 72, n_seg       # a non-null address that is never dereferenced
    s = dict(slot=0, first_step=0, n_steps=0)
    s.update(seg)
    for i in range(min(max(n_seg, 0), _lib.NOISE_MAX_SEGMENTS)):
        a.seg[i].slot, a.seg[i].first_step, a.seg[i].n_steps = s["slot"], s["first_step"], s["n_steps"]
    return a


def test_abi_additions_only():
    L = _lib.lib()
    assert L.ssrhip_version() == 107 == _lib.ABI_VERSION and L.ssrhip_sizeof(16) == -1
    assert L.ssrhip_noise_sizeof() == C.sizeof(_lib.NoiseArgs) == 16 + 5 * 4 + 4 + 32 * 20
    assert C.sizeof(_lib.NoiseSegment) == 20 and _lib.NOISE_MAX_SEGMENTS == 32


def test_contract_errors_need_no_gpu():
    L = _lib.lib()
    assert L.ssrhip_noise_philox(None, None) < 0 and b"null" in L.ssrhip_last_error()
    a = _args()
    a.noise = None
    assert L.ssrhip_noise_philox(C.byref(a), None) < 0 and b"null" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(n_seg=33)), None) < 0 and b"33 segments" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(n_seg=-1)), None) < 0
    assert L.ssrhip_noise_philox(C.byref(_args(first_step=-1, n_steps=2)), None) < 0 and b"negative" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(first_step=3, n_steps=-2)), None) < 0 and b"negative" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(first_step=30, n_steps=11)), None) < 0 and b"step 41 of 40" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(first_step=2 ** 31 - 1, n_steps=2 ** 31 - 1)), None) < 0
    assert L.ssrhip_noise_philox(C.byref(_args(slot=5, n_steps=1)), None) < 0 and b"slot 5 of 5" in L.ssrhip_last_error()
    assert L.ssrhip_noise_philox(C.byref(_args(slot=-1, n_steps=1)), None) < 0
    # nothing to draw is no error and no launch: no segment, or only empty ones (first_step == max_steps is the empty tail)
    assert L.ssrhip_noise_philox(C.byref(_args(n_seg=0)), None) == 0
    assert L.ssrhip_noise_philox(C.byref(_args(n_seg=3, first_step=40, n_steps=0)), None) == 0


# ---------------------------------------------------------------- the engine object behind a fake launcher
def test_philox_noise_sends_noise_segments_one_to_one():
    calls = []
    seeds = [7, 2 ** 32 + 5, 9]
    src = E.PhiloxNoise(seeds, launch=calls.append).bind(None, 16)
    ref = E.TorchCpuNoiseFeed([torch.Generator().manual_seed(i) for i in range(3)], 1, 8)     # the bookkeeping it has to mirror
    buf = torch.empty(3, 16, 1, 8)
    src.begin(src)
    for buf_i, slots, limit in [(0, [0, 1, 2], 40), (1, [2, 0], 40), (0, [0, 1, 2], 40), (1, [0, 1, 2], 40), (0, [1], 40)]:
        want = E.noise_segments(src.drawn, slots, 16, limit)
        n_before = len(calls)
        src.send(buf_i, slots, limit)
        E.NoiseUploader.fill(ref, buf, slots, 16, limit)
        if want:
            assert calls[-1] == [(u, off, n, seeds[u]) for u, off, n in want]
        else:
            assert len(calls) == n_before                    # every slot at the limit: nothing is launched
        assert src.drawn == ref.drawn
    assert src.drawn == [40, 40, 40]
    assert calls[2] == [(0, 32, 8, 7), (1, 16, 16, 2 ** 32 + 5), (2, 32, 8, 9)]        # cut at the limit, per slot
    src.wait(None)                                           # nothing to wait for


def test_philox_noise_reset_and_finish_leave_drawn_as_the_torch_feed_does():
    calls = []
    src = E.PhiloxNoise([1, 2], launch=calls.append).bind(None, 16)
    ref = E.TorchCpuNoiseFeed([torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)], 1, 8)
    buf = torch.empty(2, 16, 1, 8)

    def both(fn):
        fn(src)
        fn(ref)
        assert src.drawn == ref.drawn

    both(lambda f: f.send(0, [0, 1], 256) if f is src else E.NoiseUploader.fill(f, buf, [0, 1], 16, 256))
    both(lambda f: f.send(1, [0, 1], 256) if f is src else E.NoiseUploader.fill(f, buf, [0, 1], 16, 256))
    both(lambda f: f.finish(0, 21))                          # stopped inside the second chunk: the steps drawn ahead are taken back
    both(lambda f: f.finish(1, 32))                          # stopped at the chunk's end: nothing to take back
    both(lambda f: f.finish(1, 40))                          # a count past what was drawn changes nothing
    assert src.drawn == [21, 32]
    both(lambda f: f.reset_slot(0, torch.Generator().manual_seed(5), 77))
    assert src.drawn == [0, 32] and src.seeds == [77, 2]
    src.send(2, [0], 256)
    assert calls[-1] == [(0, 0, 16, 77)]                     # the refilled slot starts at step 0 under the new job's seed


def test_make_noise_feed():
    assert isinstance(E.make_noise_feed("torch_cpu", 3, 4, 72), E.TorchCpuNoiseFeed)
    src = E.make_noise_feed("philox", 3, 4, 72)
    assert isinstance(src, E.PhiloxNoise) and src.drawn == [0, 0, 0] and src.on_device
    with pytest.raises(ValueError):
        E.make_noise_feed("mt19937", 3, 4, 72)
