"""GPU: the batched watermarked stream (DESIGN.md Part I.29). `WMEncodecModel.wmdecode_stream_batch` with one item against
`WMDecodeStream` bit for bit; with 3 and 5 items — prompts of different lengths, one of them shorter than the chain's left margin,
ends at and next to a poll boundary — against `wmdecode(..., with_mark=False)` at batch 1 (2e-5: only the LSTM step kernel differs
with B) and the oracle (2e-4), the bounds of tests/test_gpu_ragged.py; the zero rows and the zero LSTM state in front of a short
prompt; allocations and library calls; the public generators against `inference_samples(use_watermark=True)`; and the bits of
`BatchDecodeStream` / `WMDecodeStream` against a recording made on the commit before this stream existed."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import inference_scale as S
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel, _device_mallocs, skip_stream_margins, wm_stream_holdback
from ssr_speech_amd.data.tokenizer import write_wav
from oracle import codec as OC
import helpers_wmstream_batch as HB
from test_gpu_stream_batch import PHN2NUM, FakePhonemizer, _pipeline

pytestmark = pytest.mark.gpu

# name -> (ratios, n_filters, pad_mode, prompts, generated frames). LSTM C = 16 n_filters: at C = 128 every B runs the matrix-core step
# kernel, at C = 256 B = 3 runs the small-batch one. Ends: one AT a poll boundary of 16 frames and one a frame behind it among the first
# three items. (4, 3, 2, 2): chain margins (2, 2), so the 1-frame prompt is shorter than the left margin — constant padding only: with
# reflect padding a prompt must be longer than the padding it is mirrored into. Its hop is 48: the last layer's kernel is known from
# 86 frames on, so the items are that long.
CASES = {
    "r8542_const": ((8, 5, 4, 2), 8, "constant", (12, 19, 40, 9, 27), (33, 32, 21, 45, 37)),
    "r8542_reflect": ((8, 5, 4, 2), 8, "reflect", (12, 19, 40, 9, 27), (33, 32, 21, 45, 37)),
    "r8542_c256": ((8, 5, 4, 2), 16, "constant", (3, 19, 40, 9, 27), (33, 32, 21, 45, 37)),
    "r4322_const": ((4, 3, 2, 2), 8, "constant", (1, 19, 40, 12, 27), (97, 96, 100, 93, 81)),
    "r4322_reflect": ((4, 3, 2, 2), 8, "reflect", (10, 19, 40, 12, 27), (97, 96, 100, 93, 81)),
}


@functools.lru_cache(maxsize=None)
def _codec(name):
    ratios, nf, pad_mode = CASES[name][:3]
    cfg = W.CodecConfig(dimension=64, n_filters=nf, ratios=ratios, bins=64, pad_mode=pad_mode)
    sd = W.codec_state_dict(cfg, seed=21)
    return cfg, sd, WMEncodecModel(cfg, sd, "cuda")


@functools.lru_cache(maxsize=None)
def _items(name):
    """per item: codes [1, K, P + G], labels [1, P + G] (0 under the prompt, 1 behind it), the kept-audio track [1, 1, (P + G) hop] (the
    original audio under the prompt, silence behind it) on the CPU, and `wmdecode` of them at batch 1 — computed once, never modified"""
    cfg, _, m = _codec(name)
    prompts, new = CASES[name][3:]
    g = torch.Generator().manual_seed(131)
    items = []
    for p, n in zip(prompts, new):
        codes = torch.randint(0, cfg.bins, (1, cfg.n_q, p + n), generator=g)
        labels = torch.cat([torch.zeros(1, p, dtype=torch.long), torch.ones(1, n, dtype=torch.long)], 1)
        track = torch.cat([torch.randn(1, 1, p * cfg.hop, generator=g) * 0.3, torch.zeros(1, 1, n * cfg.hop)], -1)
        items.append((codes, labels, track, m.wmdecode(codes.cuda(), labels.cuda(), track.cuda(), with_mark=False)[0].clone()))
    return items


def _stream(name, B, poll, probe=None):
    """the items 0 .. B-1 through one BatchWMDecodeStream in polls of `poll` frames -> (per item waveform, stream, chunk sizes per call);
    `probe(stream, when)` is called after the prompt pass and after every call"""
    cfg, _, m = _codec(name)
    prompts, new = CASES[name][3][:B], CASES[name][4][:B]
    items = _items(name)
    st = m.wmdecode_stream_batch(prompts, max(new) + 2)
    n0 = _device_mallocs(m.device)
    st.push_prompts([items[u][0][0, :, :prompts[u]] for u in range(B)], [items[u][2][0, 0, : prompts[u] * cfg.hop].cuda() for u in range(B)])
    if probe:
        probe(st, "prompts")
    done, got, calls = [0] * B, [[] for _ in range(B)], []
    while not all(st.ended):
        take = [min(poll, new[u] - done[u]) for u in range(B)]
        ended = [not st.ended[u] and new[u] - done[u] <= poll for u in range(B)]
        out = st.advance(take, ended, codes=[items[u][0][0, :, prompts[u] + done[u]: prompts[u] + done[u] + take[u]] for u in range(B)])
        calls.append([int(o.shape[-1]) for o in out])
        for u in range(B):
            assert out[u].dim() == 3 and out[u].shape[:2] == (1, 1) and out[u].shape[-1] % st.hop == 0
            got[u].append(out[u])
            done[u] += take[u]
        if probe:
            probe(st, "advance")
    assert _device_mallocs(m.device) == n0, "the stream went to the driver for memory after it was created"      # creation .. finished
    assert st.finished
    return [torch.cat(g_, -1).clone() for g_ in got], st, calls


# ----------------------------------------------------------------------------------------------- one item: WMDecodeStream's bits
@pytest.mark.parametrize("name", ["r8542_const", "r8542_reflect", "r8542_c256", "r4322_const", "r4322_reflect"])
def test_a_batch_of_one_item_is_wmdecode_stream_bit_for_bit(name):
    """One item (prompt 12 frames, 20 generated frames in polls of 7, ended with the last poll) returns the bits of a `WMDecodeStream`
    given the prompt as an `emit=False` prefix and the same frames in pushes of 7: the same kernels at B = 1, the same window rules, and
    the rows in front of the item's first frame leave both LSTMs' state exactly zero."""
    cfg, _, m = _codec(name)
    P, G, hop = 12, 20, cfg.hop
    g = torch.Generator().manual_seed(55)
    codes = torch.randint(0, cfg.bins, (1, cfg.n_q, P + G), generator=g).cuda()
    audio = (torch.randn(1, 1, P * hop, generator=g) * 0.3).cuda()
    lab = torch.cat([torch.zeros(P, dtype=torch.int32), torch.ones(G, dtype=torch.int32)]).cuda()
    one = m.wmdecode_stream(P + G + 2)
    assert one.push(codes[..., :P], lab[:P], audio, emit=False).shape == (1, 1, 0)
    chunks = [one.push(codes[..., t: t + 7], lab[t: t + 7], None) for t in range(P, P + G, 7)] + [one.finish()]
    want = torch.cat(chunks, -1).clone()
    st = m.wmdecode_stream_batch((P,), G + 2)
    st.push_prompts([codes[0, :, :P]], [audio])
    got = []
    for t in range(P, P + G, 7):
        n = min(7, P + G - t)
        got.append(st.advance([n], [t + n == P + G], codes=[codes[0, :, t: t + n]])[0])
    got = torch.cat(got, -1)
    assert st.B == 1 and st.finished and st.windows_batched == 0 and st.chain_windows_batched == 0
    assert got.shape == want.shape == (1, 1, G * hop)
    assert torch.equal(got, want), f"max |batch of one - WMDecodeStream| = {float((got - want).abs().max()):.3g}"


# ----------------------------------------------------------------------------------------------- 3 and 5 items
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_wmdecode_stream_equals_batch1_wmdecode_and_the_oracle(name, B):
    cfg, sd, m = _codec(name)
    prompts, new = CASES[name][3:]
    items, hop = _items(name), cfg.hop
    got, st, calls = _stream(name, B, 16)
    assert st.B == B and st.windows_batched > 0 and st.chain_windows_batched > 0
    if min(prompts[:B]) < skip_stream_margins(cfg)[0]:
        assert st.chain_windows > st.chain_windows_batched                     # the short prompt's first chain window ran alone
    for u in range(B):
        want = items[u][3][..., prompts[u] * hop:]
        assert got[u].shape == want.shape == (1, 1, new[u] * hop)
        err = float((got[u] - want).abs().max())
        print(f"{name} B={B} item {u}: max |stream - batch-1 wmdecode| = {err:.3g}")
        assert err <= 2e-5, (u, err)
    with torch.no_grad():
        for u in range(B):
            ref = OC.wmdecode(sd, items[u][0], items[u][1], items[u][2], cfg)[0][..., prompts[u] * hop:]
            err = float((got[u].cpu() - ref).abs().max())
            print(f"{name} B={B} item {u}: max |stream - oracle| = {err:.3g}")
            assert err <= 2e-4, (u, err)
    # samples leave while the batch still runs, as far as the hold-back allows: the longest item has output in more than one call,
    # and before its last one
    longest = max(range(B), key=lambda u: new[u])
    assert sum(c[longest] > 0 for c in calls[:-1]) >= 2, calls
    first = next(k for k, c in enumerate(calls) if c[longest] > 0)
    assert calls[first][longest] <= (16 * (first + 1) - wm_stream_holdback(cfg)) * hop
    # the same stream in polls of 7 and all at once: the same bits
    for poll in (7, 10 ** 6):
        other, _, _ = _stream(name, B, poll)
        for u in range(B):
            assert torch.equal(other[u], got[u]), (poll, u, float((other[u] - got[u]).abs().max()))


@pytest.mark.parametrize("B", [3, 5])
def test_rows_and_lstm_state_in_front_of_a_short_prompt_are_zero(B):
    """After the prompt pass: every row in front of an item's first frame is 0.0 in the input, the pre-activations and the output of both
    LSTMs — although the skip encoder's convolutions have biases, so the chain over the zero track there is not zero — and the item
    whose 1-frame prompt the pass has not reached yet (it ends in front of it, by the chain's right margin) still has h = c = 0 in both."""
    seen = []

    def probe(st, when):
        if when != "prompts" or seen:
            return
        seen.append(1)
        assert st.off[0] == st.E - 1 and st.nL <= st.off[0] and st.n1 <= st.off[0]       # item 0: nothing of it has been reached
        assert st.nL > max(st.off[1:]) and st.n1 > min(st.off[1:])                       # ... while the others are under way
        zero = lambda t: torch.equal(t, torch.zeros_like(t))                             # noqa: E731
        for u in range(st.B):
            a, b = min(st.off[u], st.nL), min(st.off[u], st.n1)
            for t in [st.p, st.u.data] + st.sk_gins + st.sk_mids:
                assert zero(t[u, :a]), u
            for t in [st.y0, st.s1.data[:, 1:]] + st.gins + st.mids:
                assert zero(t[u, :b]), u
        for cb in st.sk_cbufs + st.cbufs:                                                # (h: the rows above — a layer's output row is its h)
            assert zero(cb[0]) and not zero(cb[1])
        # the chain's rows in front of an item are NOT zero before they are zeroed: the claim above is not empty
        taps, rows = st._chain_pass(0, st.front + 4, None)
        assert float(rows.interior_view()[:, : st.front].abs().max()) > 0

    _stream("r4322_const", B, 16, probe)
    assert seen


def test_nothing_is_allocated_and_every_stage_is_one_launch_whatever_b_is():
    """`num_device_alloc` does not move between creation and `finished` (asserted in `_stream`); the library calls of an `advance` in
    which every item is live and the windows agree are the same at B = 2 and B = 5, and two of them are row-op launches — the cores of
    the chain window and of the stage-2 window."""
    per_b = {}
    for B in (2, 5):
        cfg, _, m = _codec("r8542_const")
        counts = []

        def probe(st, when):
            counts.append((m.n_launches, st.ops.launches, when, all(not e for e in st.ended), st.chain_windows, st.windows))

        _stream("r8542_const", B, 16, probe)
        # the first advance: frames 0 .. 16 of every item, nobody ends, one chain window and one stage-2 window
        (l0, o0, _, _, c0, w0), (l1, o1, _, live, c1, w1) = counts[0], counts[1]
        assert live and c1 - c0 == 1 and w1 - w0 == 1
        per_b[B] = (l1 - l0, o1 - o0)
    print(f"library calls per all-live advance: {per_b}")
    assert per_b[2] == per_b[5] and per_b[2][1] == 2


def test_batch_wmdecode_stream_refusals():
    cfg, _, m = _codec("r8542_const")
    st = m.wmdecode_stream_batch((5, 9), 8)
    good = [torch.zeros(cfg.n_q, 5, dtype=torch.long), torch.zeros(cfg.n_q, 9, dtype=torch.long)]
    audio = [torch.zeros(5 * cfg.hop), torch.zeros(9 * cfg.hop - 3)]               # (a shorter one is zero-extended)
    with pytest.raises(RuntimeError):
        st.advance([1, 1], [False, False], codes=[g[:, :1] for g in good])
    with pytest.raises(ValueError, match="samples under a prompt"):
        st.push_prompts(good, [torch.zeros(5 * cfg.hop + 1), audio[1]])
    with pytest.raises(IndexError):
        st.push_prompts([good[0], torch.full((cfg.n_q, 9), cfg.bins, dtype=torch.long)], audio)
    st = m.wmdecode_stream_batch((5, 9), 8)
    st.push_prompts(good, audio)
    with pytest.raises(ValueError, match="lock-step"):
        st.advance([2, 3], [False, False], codes=[good[0][:, :2], good[1][:, :3]])
    with pytest.raises(ValueError, match="max_new_frames"):
        st.advance([9, 9], [False, False], codes=[good[1], good[1]])
    with pytest.raises(IndexError):
        st.advance([2, 2], [False, False], codes=[good[0][:, :2]] * 2, flag=torch.ones(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="reflect"):
        _codec("r8542_reflect")[2].wmdecode_stream_batch((7, 19), 8)               # a prompt no longer than what it is mirrored into


# ----------------------------------------------------------------------------------------------- end to end on the tiny stack
def test_samples_of_one_utterance_watermarked_stream(tmp_path):
    """N = 3 samples, sampled, with CFG: the tokens of `inference_batch(refill=False)`, the waveforms of
    `inference_samples(use_watermark=True)`, a chunk of every sample before the iterator is exhausted; and without the watermark the
    chunks of `inference_samples_stream`."""
    args, m, tok = _pipeline()
    margs = argparse.Namespace(**vars(args))
    fn = str(tmp_path / "prompt.wav")
    write_wav(fn, torch.randn(1, 20 * 320 - 7, generator=torch.Generator().manual_seed(1)) * 0.2, 16000)
    dc = {"top_k": 40, "top_p": 0.8, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    call = lambda wm: (m, margs, PHN2NUM, FakePhonemizer(), tok, fn, "hello world", "hello world again", torch.LongTensor([[20, 20]]), 1.5, 2,      # noqa: E731
                       True, False, wm, True, "cuda", dc)
    seeds = [11, 12, 13]
    # the tokens
    y, _ = S._prompt_codes(tok, fn, 4)
    one = {"x": S._phoneme_ids(FakePhonemizer(), PHN2NUM, "hello world again"), "y": y, "mask_interval": torch.tensor([[[20, 20]]], dtype=torch.long)}
    kw = dict(top_k=40, top_p=0.8, temperature=1, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, aug_text=True, seed=seeds[0])
    want = m.inference_batch([one] * 3, refill=False, **kw)
    it = m.inference_batch_wmstream([one] * 3, **kw)
    assert it.results is None and len(list(it)) >= 3
    assert len(it.results) == len(want) == 3
    for got, ref in zip(it.results, want):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3]
    # the samples
    waves = [w.clone() for w in S.inference_samples(*call(True), seeds=seeds)]
    parts, at = [[] for _ in seeds], [[] for _ in seeds]
    for i, chunk in S.inference_samples_wmstream(*call(True), seeds=seeds):
        assert chunk.dim() == 3 and chunk.shape[:2] == (1, 1) and chunk.shape[-1] > 0
        parts[i].append(chunk)
        at[i].append(next(iter(m._engines.values()))._steps_enqueued)
    last = max(max(a) for a in at)
    for i in range(3):
        got = torch.cat(parts[i], -1)
        assert got.shape == waves[i].shape, (i, got.shape, waves[i].shape)
        err = float((got - waves[i]).abs().max())
        print(f"sample {i}: {got.shape[-1] // 320} frames in {len(parts[i])} chunks, max |stream - inference_samples(use_watermark=True)| = {err:.3g}")
        assert err <= 2e-5, (i, err)
        assert at[i][0] < last, f"sample {i}: its first chunk came with the last poll"
    plain = float((torch.cat(parts[0], -1) - S.inference_samples(*call(False), seeds=seeds)[0]).abs().max())
    assert plain > 1e-3, "the watermarked waveform is the plain one: the test shows nothing"
    # a falsy use_watermark: the un-watermarked twin's chunks
    twin = [(i, c.clone()) for i, c in S.inference_samples_stream(*call(False), seeds=seeds)]
    mine = [(i, c.clone()) for i, c in S.inference_samples_wmstream(*call(False), seeds=seeds)]
    assert len(mine) == len(twin) and all(a[0] == b[0] and torch.equal(a[1], b[1]) for a, b in zip(mine, twin))


def test_inference_batch_wmstream_of_three_utterances(tmp_path):
    """three utterances with prompts of different lengths, greedy, with CFG: each against `inference_one_sample(use_watermark=True)`"""
    from test_gpu_stream_batch import FRAMES, TEXTS
    args, m, tok = _pipeline()
    margs = argparse.Namespace(**vars(args))
    utts = []
    for i in range(3):
        fn = str(tmp_path / f"prompt{i}.wav")
        write_wav(fn, torch.randn(1, FRAMES[i] * 320 - 7, generator=torch.Generator().manual_seed(40 + i)) * 0.2, 16000)
        utts.append({"audio_fn": fn, "target_text": TEXTS[i]})
    dc = {"top_k": 1, "top_p": 1.0, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    parts = [[] for _ in utts]
    for i, chunk in S.inference_batch_wmstream(m, margs, PHN2NUM, FakePhonemizer(), tok, utts, 1.5, 2, True, True, "cuda", dc, seed=5):
        parts[i].append(chunk)
    for i in range(3):
        mi = torch.LongTensor([[FRAMES[i], FRAMES[i]]])
        torch.manual_seed(5 + i)
        one = S.inference_one_sample(m, margs, PHN2NUM, FakePhonemizer(), tok, utts[i]["audio_fn"], "hello", TEXTS[i], mi, 1.5, 2, True, False,
                                     True, True, "cuda", dc)
        got = torch.cat(parts[i], -1)
        assert got.shape == one.shape, (i, got.shape, one.shape)
        err = float((got - one).abs().max())
        print(f"utterance {i}: max |stream - inference_one_sample(use_watermark=True)| = {err:.3g}")
        assert err <= 2e-5 and len(parts[i]) >= 2, (i, err)


# ----------------------------------------------------------------------------------------------- the other streams keep their bits
def test_batch_decode_stream_and_wmdecode_stream_keep_their_bits():
    """`BatchDecodeStream` and `WMDecodeStream` on one fixed case each (tests/helpers_wmstream_batch.py), against what the same code
    returned on the commit before `BatchWMDecodeStream` and `ssrhip_stream_rows` existed."""
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", HB.GOLDEN))
    now = HB.golden_streams()
    assert sorted(now) == sorted(rec.files) == ["batch0", "batch1", "batch2", "wm"]
    for k in rec.files:
        assert now[k].shape == rec[k].shape and np.array_equal(now[k], rec[k]), (k, float(np.abs(now[k] - rec[k]).max()))
