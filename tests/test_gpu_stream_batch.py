"""GPU: the batched stream (DESIGN.md Part I.16). `ssrhip_stream_gather` against its numpy model, the zero-state claim of
`BatchDecodeStream` at the kernel level, the codec stream at B = 2 / 4 / 5 against `decode` at batch 1 and the oracle,
`SSR_Speech.inference_batch_stream` against `inference_batch(refill=False)`, the public generator against `inference_one_sample`,
and one run at the 830M shape."""
import argparse
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import inference_scale as S
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel, _device_mallocs, stream_margins
from ssr_speech_amd.data.tokenizer import AudioTokenizer, write_wav
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import codec as OC
import helpers_codec as H
from test_stream_batch_host import gather_model

pytestmark = pytest.mark.gpu
K = 4
POISON = -12345


# ----------------------------------------------------------------------------------------------- ssrhip_stream_gather
def _gather(gen: np.ndarray, table: np.ndarray, B: int, cap: int, bins: int, dev_table=None, **null):
    """-> (rc, codes_out [B][K][cap] on the CPU, flag): one call on a poisoned output block"""
    L = _lib.lib()
    n, max_steps, k = gen.shape
    dgen = torch.from_numpy(gen.astype(np.int32)).cuda()
    host = np.ascontiguousarray(table, dtype=np.int32)
    dtab = torch.from_numpy(np.ascontiguousarray(table if dev_table is None else dev_table, dtype=np.int32)).cuda()
    out = torch.full((B, k, cap), POISON, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = dict(generated=dgen.data_ptr(), ranges_host=host.ctypes.data, ranges_dev=dtab.data_ptr(), codes_out=out.data_ptr(), flag=flag.data_ptr())
    ptr.update(null)
    rc = L.ssrhip_stream_gather(ptr["generated"], n, max_steps, null.get("K", k), ptr["ranges_host"], ptr["ranges_dev"], ptr["codes_out"], B, cap,
                                bins, ptr["flag"], _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(flag.item())


@pytest.mark.parametrize("n_utt", [1, 3, 16])
def test_gather_equals_its_numpy_model_over_the_whole_poisoned_block(n_utt):
    g = np.random.default_rng(n_utt)
    max_steps, cap, bins = 200, 150, 64
    gen = g.integers(0, bins, size=(n_utt, max_steps, K))
    tables = []
    for trial in range(4):
        t = np.zeros((4, n_utt), dtype=np.int64)
        for u in range(n_utt):
            step0 = int(g.integers(0, 40))
            most = max_steps - (K - 1) - step0                                 # frames whose last codebook is still a valid step
            f1 = most if (u + trial) % 3 == 0 else int(g.integers(0, most + 1))   # ... some ranges end ON the last valid step
            f0 = f1 if (u + trial) % 4 == 1 else int(g.integers(max(f1 - 140, 0), f1 + 1))       # ... and some are empty
            col0 = int(g.integers(-f0, cap - f1 + 1))
            t[:, u] = (step0, f0, f1, col0)
        tables.append(t)
    tables.append(np.stack([np.zeros(n_utt), np.full(n_utt, 5), np.full(n_utt, 5), np.zeros(n_utt)]).astype(np.int64))      # all empty: no launch
    for t in tables:
        want = np.full((n_utt + 1, K, cap), POISON, dtype=np.int64)
        assert not gather_model(gen, t, want, bins)
        rc, got, flag = _gather(gen, t, n_utt + 1, cap, bins)                   # one row more than utterances: it must stay poisoned
        assert rc == 0 and flag == 0
        assert np.array_equal(got, want)
    assert any((t[2] - t[1]).max() > 64 for t in tables) and any((t[2] == t[1]).any() for t in tables)


def test_gather_clamps_and_flags_ids_outside_the_codebook():
    gen = np.random.default_rng(5).integers(0, 64, size=(3, 40, K))
    gen[1, 7, 2] = 64                                                          # frame 5, codebook 2: id == bins
    gen[2, 9, 0] = -1                                                          # frame 9, codebook 0: negative
    t = np.array([[0, 0, 0], [0, 0, 0], [20, 20, 20], [0, 0, 0]])
    want = np.full((3, K, 20), POISON, dtype=np.int64)
    assert gather_model(gen, t, want, 64)
    rc, got, flag = _gather(gen, t, 3, 20, 64)
    assert rc == 0 and flag == 1 and np.array_equal(got, want)
    assert got[1, 2, 5] == 63 and got[2, 0, 9] == 0
    t[1] = 10                                                                  # the bad ids are not in [10, 20): no flag
    rc, got, flag = _gather(gen, t, 3, 20, 64)
    assert rc == 0 and flag == 0


def test_gather_contract_errors_come_before_any_launch():
    L = _lib.lib()
    gen = np.zeros((2, 30, K), dtype=np.int64)
    ok = np.array([[0, 0], [0, 2], [8, 9], [0, 0]])

    def refused(table, what, cap=16, **kw):
        rc, got, flag = _gather(gen, table, 2, cap, 64, dev_table=ok, **kw)   # the device copy is fine: only the host check can refuse
        assert rc != 0 and what in L.ssrhip_last_error().decode(), (rc, L.ssrhip_last_error())
        assert np.all(got == POISON) and flag == 0, "something was launched"

    for name in ("generated", "ranges_host", "ranges_dev", "codes_out", "flag"):
        refused(ok, "null", **{name: 0})
    refused(ok, "K=5", K=5)
    refused(np.array([[0, 0], [0, 5], [8, 4], [0, 0]]), "frame range")            # f0 > f1
    refused(np.array([[0, 0], [0, -1], [8, 4], [0, 0]]), "frame range")
    refused(ok, "columns", cap=8)                                                 # a column past cap
    refused(np.array([[0, 0], [0, 2], [8, 9], [0, -3]]), "columns")               # ... and one in front of the block
    refused(np.array([[0, 20], [0, 2], [8, 9], [0, 0]]), "reads step")            # 20 + 8 + 3 >= 30 steps
    assert _gather(gen, ok, 2, 16, 64)[0] == 0
    # the kernel checks the device copy again: with a stale table it skips what falls outside `generated` and the block
    stale = np.array([[0, 28], [0, 0], [8, 40], [0, 10]])
    rc, got, flag = _gather(gen, ok, 2, 16, 64, dev_table=stale)
    assert rc == 0 and flag == 0
    assert np.all(got[0, :, :8] == 0) and np.all(got[0, :, 8:] == POISON)
    assert got[1, 0, 10] == 0 and got[1, 1, 10] == 0 and got[1, 0, 11] == 0          # steps 28 and 29 exist
    assert got[1, 2, 10] == POISON and got[1, 3, 10] == POISON and got[1, 1, 11] == POISON and np.all(got[1, :, 12:] == POISON)
    assert np.all(got[1, :, :10] == POISON)


# ----------------------------------------------------------------------------------------------- the zero-state claim
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("Cc", [128, 256])          # B = 2: the matrix-core kernel at C = 128, the small-batch kernel at C = 256; B = 5: matrix-core
def test_rows_with_zero_input_leave_the_lstm_state_exactly_zero(B, Cc):
    """What `BatchDecodeStream` rests on: over rows whose `gin` and skip input are zero, from h = c = 0, the layer writes exactly 0.0 and
    leaves exactly 0.0 in hbuf / cbuf; a later row equals, bit for bit, the same item run from row 0 without the zero rows in front."""
    L = _lib.lib()
    T, lead = 21, (9, 0, 4, 13, 9)[:B]                                          # item u has lead[u] zero rows in front
    g = torch.Generator().manual_seed(7000 + Cc + B)
    gin, skip, whh = torch.randn(B, T, 4 * Cc, generator=g), torch.randn(B, T, Cc, generator=g), H.lstm_weights(Cc, seed=Cc)
    for u, p in enumerate(lead):
        gin[u, :p], skip[u, :p] = 0.0, 0.0
    small = B <= 4 and Cc == 256
    w = (whh if small else H.pack_whh(whh)).cuda().contiguous()

    def run(gin_, skip_, windows, elu):
        Tn = gin_.shape[1]
        dgin, dskip = gin_.cuda().contiguous(), skip_.cuda().contiguous()
        out = torch.full((B, Tn, Cc), float("nan"), device="cuda")
        hbuf, cbuf = torch.full((2, 16, Cc), float("nan"), device="cuda"), torch.full((B, Cc), float("nan"), device="cuda")
        for t0, t1 in windows:
            a = _lib.LstmArgs()
            a.gin, a.w_hh, a.out, a.skip = dgin.data_ptr(), w.data_ptr(), out.data_ptr(), dskip.data_ptr()
            a.hbuf, a.cbuf, a.gates = hbuf.data_ptr(), cbuf.data_ptr(), 0
            a.B, a.T, a.C = B, Tn, Cc
            a.gin_bstride, a.out_bstride, a.skip_bstride = Tn * 4 * Cc, Tn * Cc, Tn * Cc
            a.t_begin, a.t_end, a.w_packed, a.out_act = t0, t1, int(not small), (_lib.ACT_ELU if elu else 0)
            _lib.check(L.ssrhip_lstm_layer(C.byref(a), _lib.stream_ptr()), "ssrhip_lstm_layer")
        torch.cuda.synchronize()
        return out.cpu(), hbuf.cpu(), cbuf.cpu()

    for elu in (False, True):
        # every item zero over the rows [0, 4) (lead >= 4 for the items looked at): the state the step kernel leaves behind
        zin, zskip = gin.clone(), skip.clone()
        zin[:, :4], zskip[:, :4] = 0.0, 0.0
        out, hbuf, cbuf = run(zin, zskip, [(0, 4)], elu)
        assert torch.equal(out[:, :4], torch.zeros(B, 4, Cc))
        written = ~torch.isnan(hbuf)
        assert int(written.sum()) >= B * Cc and torch.equal(hbuf[written], torch.zeros(int(written.sum())))
        assert torch.equal(cbuf, torch.zeros(B, Cc))
        # the whole run, in the pieces a stream advances by, against the items without their zero rows
        full, _, _ = run(gin, skip, [(0, 3), (3, 10), (10, T)], elu)
        for u, p in enumerate(lead):
            assert torch.equal(full[u, :p], torch.zeros(p, Cc)), u
        for p in sorted(set(lead)):
            cut, _, _ = run(gin[:, p:], skip[:, p:], [(0, T - p)], elu)
            for u in [u for u in range(B) if lead[u] == p]:
                assert torch.equal(full[u, p:], cut[u]), (u, p, float((full[u, p:] - cut[u]).abs().max()))
        want = H.lstm_ref(gin, whh, skip, elu)
        torch.testing.assert_close(full.double(), want, rtol=2e-5, atol=2e-5)


# ----------------------------------------------------------------------------------------------- BatchDecodeStream
TINY = W.CodecConfig(dimension=64, n_filters=8, ratios=(8, 5, 4, 2), bins=64)
PROMPTS = (5, 19, 40, 8, 27)
NEW = (2, 37, 21, 45, 30)              # generated frames: item 0 ends inside the first poll behind its prompt, the others in different polls


@functools.lru_cache(maxsize=None)
def _codec(pad_mode, full=False):
    cfg = dataclasses.replace(W.codec_config_full() if full else TINY, pad_mode=pad_mode)
    sd = W.codec_state_dict(cfg, seed=21)
    return cfg, sd, WMEncodecModel(cfg, sd, "cuda")


@functools.lru_cache(maxsize=None)
def _items(pad_mode, full=False):
    """per item: (codes [1, K, P + G] on the CPU, `decode` of them at batch 1) — computed once, never modified"""
    cfg, _, m = _codec(pad_mode, full)
    g = torch.Generator().manual_seed(31)
    codes = [torch.randint(0, cfg.bins, (1, cfg.n_q, p + n), generator=g) for p, n in zip(PROMPTS, NEW)]
    return codes, [m.decode(c.cuda()).clone() for c in codes]


def _stream(m, codes, B, poll, prompts=PROMPTS, new=NEW):
    """the items 0 .. B-1 through one BatchDecodeStream in polls of `poll` frames -> (per item waveform, stream, chunks per call)"""
    st = m.decode_stream_batch(prompts[:B], max(new[:B]) + 2)
    n0 = _device_mallocs(m.device)
    st.push_prompts([codes[u][0, :, :prompts[u]] for u in range(B)])
    done, got, calls = [0] * B, [[] for _ in range(B)], []
    while not all(st.ended):
        # lock-step: every item that goes on gets `poll` frames; an item with no more than that left ends here
        take = [min(poll, new[u] - done[u]) for u in range(B)]
        ended = [not st.ended[u] and new[u] - done[u] <= poll for u in range(B)]
        out = st.advance(take, ended, codes=[codes[u][0, :, prompts[u] + done[u]: prompts[u] + done[u] + take[u]] for u in range(B)])
        calls.append([int(o.shape[-1]) for o in out])
        for u in range(B):
            assert out[u].dim() == 3 and out[u].shape[:2] == (1, 1) and out[u].shape[-1] % st.hop == 0
            got[u].append(out[u])
            done[u] += take[u]
    assert _device_mallocs(m.device) == n0, "the stream went to the driver for memory after it was created"
    assert st.finished
    return [torch.cat(g_, -1).clone() for g_ in got], st, calls


@pytest.mark.parametrize("B", [2, 4, 5])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_batch_decode_stream_equals_batch1_decode_and_the_oracle(pad_mode, B):
    cfg, sd, m = _codec(pad_mode)
    codes, ones = _items(pad_mode)
    hop = cfg.hop
    got, st, calls = _stream(m, codes, B, 16)
    assert st.B == B and (st.windows_batched > 0 or B == 2)      # (B = 2: item 0 ends in the first poll, item 1 is alone from there on)
    for u in range(B):
        want = ones[u][..., PROMPTS[u] * hop:]
        assert got[u].shape == want.shape == (1, 1, NEW[u] * hop)
        err = float((got[u] - want).abs().max())
        print(f"{pad_mode} B={B} item {u}: max |stream - batch-1 decode| = {err:.3g}")
        assert err <= 2e-5, (u, err)
    with torch.no_grad():
        for u in range(B):
            ref = OC.decode(sd, codes[u], cfg)[..., PROMPTS[u] * hop:]
            np.testing.assert_allclose(got[u].cpu().numpy(), ref.numpy(), rtol=0, atol=2e-4)
    # a dense zero-padded decode of the batch is NOT the same thing on the shortest item: the test would show nothing if it were
    dense = torch.zeros(B, cfg.n_q, max(p + n for p, n in zip(PROMPTS[:B], NEW[:B])), dtype=torch.long)
    for u in range(B):
        dense[u, :, : codes[u].shape[-1]] = codes[u][0]
    naive = m.decode(dense.cuda())
    miss = float((naive[0:1, :, PROMPTS[0] * hop: (PROMPTS[0] + NEW[0]) * hop] - ones[0][..., PROMPTS[0] * hop:]).abs().max())
    print(f"dense zero-padded decode, shortest item: {miss:.3g}")
    assert miss > 2e-5
    # samples leave while the batch still runs: the longest item has output in more than one call, and before its last one
    longest = max(range(B), key=lambda u: NEW[u])
    assert sum(c[longest] > 0 for c in calls[:-1]) >= 2
    # the same stream in polls of 7 and all at once: the same bits
    for poll in (7, 10 ** 6):
        other, _, _ = _stream(m, codes, B, poll)
        for u in range(B):
            assert torch.equal(other[u], got[u]), (poll, u, float((other[u] - got[u]).abs().max()))


def test_batch_decode_stream_full_codec():
    """the 830M pipeline's codec (LSTM C = 512): B = 4 is the small-batch LSTM kernel, as batch 1 is"""
    cfg, sd, m = _codec("constant", True)
    codes, ones = _items("constant", True)
    got, st, _ = _stream(m, codes, 4, 16)
    for u in range(4):
        err = float((got[u] - ones[u][..., PROMPTS[u] * cfg.hop:]).abs().max())
        print(f"full codec item {u}: max |stream - batch-1 decode| = {err:.3g}")
        assert err <= 2e-5, (u, err)


def test_a_prompt_shorter_than_the_left_margin_takes_its_first_window_alone():
    """The ratios (4, 3, 2, 2) have margins (2, 2) — at the product's (8, 5, 4, 2) they are (1, 1) and no prompt is shorter. Item 0's prompt
    is ONE frame: its first window would reach in front of its first frame, so it is cut there (a true edge) and runs alone."""
    cfg = W.CodecConfig(dimension=64, n_filters=8, ratios=(4, 3, 2, 2), bins=64)
    assert stream_margins(cfg) == (2, 2)
    m = WMEncodecModel(cfg, W.codec_state_dict(cfg, seed=7), "cuda")
    prompts, new = (1, 19, 40), (100, 100, 93)                                  # long enough for the last layer's kernel to be known early
    g = torch.Generator().manual_seed(77)
    codes = [torch.randint(0, cfg.bins, (1, cfg.n_q, p + n), generator=g) for p, n in zip(prompts, new)]
    got, st, calls = _stream(m, codes, 3, 16, prompts, new)
    assert st.windows_batched > 0 and st.windows > st.windows_batched
    assert any(c[0] > 0 for c in calls[:-1]) and any(c[2] > 0 for c in calls[:3])      # item 2 (86 frames at the third poll) starts first
    for u in range(3):
        want = m.decode(codes[u].cuda())[..., prompts[u] * cfg.hop:]
        err = float((got[u] - want).abs().max())
        print(f"margins (2, 2), item {u}: max |stream - batch-1 decode| = {err:.3g}")
        assert got[u].shape == want.shape and err <= 2e-5, (u, err)


@pytest.mark.parametrize("name", ["tiny_const", "tiny_reflect", "r8542_c128"])
def test_a_batch_of_one_item_is_decode_stream_bit_for_bit(name):
    """The two streams are one core: a `BatchDecodeStream` with ONE item (prompt 5 frames, 20 generated frames in polls of 7, ended with
    the last poll) returns the bits of a `DecodeStream` given the prompt as an `emit=False` prefix and the same frames in pushes of 7.
    Same kernels at B = 1, the same window rule, and the rows in front of the item's first frame leave the LSTM state exactly zero."""
    import test_gpu_stream as GS
    cfg, _, m = GS._codec(name)
    P, G = 5, 20
    codes = torch.randint(0, cfg.bins, (1, cfg.n_q, P + G), generator=torch.Generator().manual_seed(55))
    one = m.decode_stream(P + G + 2)
    assert one.push(codes[..., :P].cuda(), emit=False).shape == (1, 1, 0)
    chunks = [one.push(codes[..., t: t + 7].cuda()) for t in range(P, P + G, 7)] + [one.finish()]
    want = torch.cat(chunks, -1).clone()
    got, st, calls = _stream(m, [codes], 1, 7, (P,), (G,))
    assert st.B == 1 and len(calls) == 3 and st.windows_batched == 0
    assert got[0].shape == want.shape == (1, 1, G * cfg.hop)
    assert torch.equal(got[0], want), f"max |batch of one - DecodeStream| = {float((got[0] - want).abs().max()):.3g}"


def test_batch_decode_stream_refuses_what_decode_refuses():
    cfg, _, m = _codec("constant")
    st = m.decode_stream_batch((5, 9), 8)
    good = [torch.zeros(cfg.n_q, 5, dtype=torch.long), torch.zeros(cfg.n_q, 9, dtype=torch.long)]
    with pytest.raises(RuntimeError):
        st.advance([1, 1], [False, False], codes=[g[:, :1] for g in good])      # before the prompts
    with pytest.raises(IndexError):
        st.push_prompts([good[0], torch.full((cfg.n_q, 9), cfg.bins, dtype=torch.long)])
    st = m.decode_stream_batch((5, 9), 8)
    st.push_prompts(good)
    with pytest.raises(ValueError, match="lock-step"):
        st.advance([2, 3], [False, False], codes=[good[0][:, :2], good[1][:, :3]])
    with pytest.raises(ValueError, match="max_new_frames"):
        st.advance([9, 9], [False, False], codes=[good[1], good[1]])
    flag = torch.ones(1, dtype=torch.int32, device="cuda")                       # what the gather sets for an id outside the codebook
    with pytest.raises(IndexError):
        st.advance([2, 2], [False, False], codes=[good[0][:, :2]] * 2, flag=flag)
    with pytest.raises(ValueError):
        _codec("reflect")[2].decode_stream_batch((3, 9), 8)                      # a prompt no longer than the reflect padding
    tok = AudioTokenizer(device="cuda", config=cfg, state_dict=W.codec_state_dict(cfg, seed=21))
    with pytest.raises(ValueError, match="watermark"):
        tok.decode_stream_batch((5, 9), 8, use_watermark=True)
    assert stream_margins(cfg) == (1, 1)


# ----------------------------------------------------------------------------------------------- end to end on the tiny stack
class FakePhonemizer:
    def __call__(self, texts):
        return [[c for c in t if c != " "] for t in texts]


@functools.lru_cache(maxsize=None)
def _pipeline():
    """the models of tests/test_gpu_stream.py"""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    lsd = W.lm_state_dict(args, seed=8)
    for k in range(4):   # a random-weight LM would emit special ids (>= vocab) that RVQ decode rejects, as in the reference: bias them away
        lsd[f"predict_layer.{k}.2.bias"][64:] = -30.0
    m = SSR_Speech(args)
    m.load_state_dict(lsd)
    return args, m.to("cuda").eval(), AudioTokenizer(device="cuda", config=TINY, state_dict=W.codec_state_dict(TINY, seed=7))


TEXTS = ("hello world again", "a much longer line of text to read out loud", "short one")
FRAMES = (20, 9, 12)
PHN2NUM = {c: i for i, c in enumerate("abcdefghijklmnopqrstuvwxyz")}


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("n_utt,aug_text", [(3, True), (2, False)])
def test_inference_batch_stream_end_to_end(tmp_path, n_utt, aug_text, sampled):
    args, m, tok = _pipeline()
    margs = argparse.Namespace(**vars(args))
    utts = []
    for i in range(n_utt):
        fn = str(tmp_path / f"prompt{i}.wav")
        write_wav(fn, torch.randn(1, FRAMES[i] * 320 - 7, generator=torch.Generator().manual_seed(40 + i)) * 0.2, 16000)
        utts.append({"audio_fn": fn, "target_text": TEXTS[i]})
    dc = {"top_k": 40 if sampled else 1, "top_p": 0.8 if sampled else 1.0, "temperature": 1, "stop_repetition": 2, "kvcache": 1,
          "codec_audio_sr": 16000, "codec_sr": 50}
    seed = 5
    # the tokens: `.results` against the one-pass call, on every integer of every tuple
    jobs = []
    for u in utts:
        y, _ = S._prompt_codes(tok, u["audio_fn"], K)
        jobs.append({"x": S._phoneme_ids(FakePhonemizer(), PHN2NUM, u["target_text"]), "y": y,
                     "mask_interval": torch.tensor([[[y.shape[1], y.shape[1]]]], dtype=torch.long)})
    kw = dict(top_k=dc["top_k"], top_p=dc["top_p"], temperature=1, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, aug_text=aug_text, seed=seed)
    want = m.inference_batch(jobs, refill=False, **kw)
    it = m.inference_batch_stream(jobs, **kw)
    assert it.results is None and it.polls == 0
    incs = list(it)
    assert incs[0].kept and incs[0].counts == [int(j["y"].shape[1]) for j in jobs] and not any(i.kept for i in incs[1:])
    assert len(it.results) == len(want) == n_utt and it.polls >= 3
    for got, ref in zip(it.results, want):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3]
    for u in range(n_utt):
        assert sum(i.counts[u] for i in incs[1:]) == want[u][0].shape[-1] - jobs[u]["y"].shape[1]
        assert sum(i.ended[u] for i in incs[1:]) == 1
    # the samples: the public generator against one inference_one_sample per utterance under seed + i
    chunks, at = [[] for _ in range(n_utt)], [[] for _ in range(n_utt)]
    for i, chunk in S.inference_batch_stream(m, margs, PHN2NUM, FakePhonemizer(), tok, utts, 1.5, 2, aug_text, False, "cuda", dc, seed=seed):
        eng = next(iter(m._engines.values()))
        assert chunk.dim() == 3 and chunk.shape[:2] == (1, 1) and chunk.shape[-1] > 0
        chunks[i].append(chunk)
        at[i].append(eng._steps_enqueued)
    last = max(max(a) for a in at)
    for i in range(n_utt):
        steps = int(want[i][0].shape[-1] - jobs[i]["y"].shape[1]) + K
        assert steps > 32, f"utterance {i} is too short ({steps} steps) to show audio leaving before it ends"
        assert at[i][0] < last, f"utterance {i}: the first chunk came with the last poll"
        assert at[i][0] < (steps + 15) // 16 * 16, f"utterance {i}: nothing left before its own last poll"
        mi = torch.LongTensor([[FRAMES[i], FRAMES[i]]])
        torch.manual_seed(seed + i)
        one = S.inference_one_sample(m, margs, PHN2NUM, FakePhonemizer(), tok, utts[i]["audio_fn"], "hello", TEXTS[i], mi, 1.5, 2, aug_text, False,
                                     False, True, "cuda", dc)
        got = torch.cat(chunks[i], -1)
        assert got.shape == one.shape, (i, got.shape, one.shape)
        err = float((got - one).abs().max())
        print(f"n_utt={n_utt} cfg={aug_text} sampled={sampled} utterance {i}: max |stream - inference_one_sample| = {err:.3g}")
        assert err <= 2e-5, (i, err)


def test_samples_of_one_utterance_stream(tmp_path):
    """`inference_samples_stream`: the N samples of one utterance, each against `inference_one_sample` under its own seed"""
    args, m, tok = _pipeline()
    margs = argparse.Namespace(**vars(args))
    fn = str(tmp_path / "prompt.wav")
    write_wav(fn, torch.randn(1, 20 * 320 - 7, generator=torch.Generator().manual_seed(1)) * 0.2, 16000)
    dc = {"top_k": 40, "top_p": 0.8, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    call = (m, margs, PHN2NUM, FakePhonemizer(), tok, fn, "hello world", "hello world again", torch.LongTensor([[20, 20]]), 1.5, 2, True, False,
            False, True, "cuda", dc)
    seeds = [11, 12, 13]
    parts = [[] for _ in seeds]
    for i, chunk in S.inference_samples_stream(*call, seeds=seeds):
        parts[i].append(chunk)
    for i, s in enumerate(seeds):
        torch.manual_seed(s)
        one = S.inference_one_sample(*call)
        got = torch.cat(parts[i], -1)
        assert got.shape == one.shape and float((got - one).abs().max()) <= 2e-5
        assert len(parts[i]) >= 2


def test_cli_stream_dir_writes_each_samples_chunks(tmp_path):
    """`--tts --sample_batch_size 3 --stream_dir DIR`: one raw float32 file per sample, appended chunk by chunk, holding the waveform
    the run also writes as .wav — which is, to the PCM step, what the run without the flag writes."""
    from ssr_speech_amd import inference_v2 as CLI
    from ssr_speech_amd.data.tokenizer import read_wav
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    lsd = W.lm_state_dict(args, seed=8)
    for k in range(4):
        lsd[f"predict_layer.{k}.2.bias"][64:] = -30.0
    lm_ckpt, codec_ckpt = str(tmp_path / "lm.pth"), str(tmp_path / "codec.th")
    torch.save({"config": argparse.Namespace(**vars(args)), "model": lsd, "phn2num": PHN2NUM}, lm_ckpt)
    torch.save({"codec_config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(TINY).items()},
                "model": W.codec_state_dict(TINY, seed=7)}, codec_ckpt)
    wav_fn = str(tmp_path / "orig.wav")
    write_wav(wav_fn, torch.randn(1, 24 * 320, generator=torch.Generator().manual_seed(3)) * 0.2, 16000)
    ids = lambda t: ",".join(str(PHN2NUM[c]) for c in t if c != " ")
    base = ["--model_path", lm_ckpt, "--codec_path", codec_ckpt, "--orig_audio", wav_fn, "--orig_transcript", "hello world",
            "--target_transcript", "again", "--temp_folder", str(tmp_path / "tmp"), "--savename", "utt", "--seed", "11", "--top_k", "12",
            "--top_p", "0.9", "--cfg_stride", "2", "--aug_text", "--tts", "--prompt_end", "0.4", "--phoneme_ids", ids("hello world again"),
            "--prompt_phoneme_ids", ids("hello world"), "--sample_batch_size", "3"]
    CLI.main(base + ["--output_dir", str(tmp_path / "plain")])
    CLI.main(base + ["--output_dir", str(tmp_path / "streamed"), "--stream_dir", str(tmp_path / "chunks")])
    for num in range(3):
        raw = np.fromfile(str(tmp_path / "chunks" / f"utt_new_seed{11 + num}.f32"), dtype="<f4")
        a, _ = read_wav(str(tmp_path / "streamed" / f"utt_new_seed{11 + num}.wav"))
        b, _ = read_wav(str(tmp_path / "plain" / f"utt_new_seed{11 + num}.wav"))
        assert raw.size > 0 and raw.size % 320 == 0 and a.shape == b.shape == (1, raw.size)
        pcm = (np.round(np.clip(raw, -1, 1) * 32767.0) / 32768.0).astype(np.float32)      # write_wav's 16 bits, as read_wav returns them
        assert np.array_equal(a[0].numpy(), pcm)
        assert float((a - b).abs().max()) <= 1.0 / 32768.0 + 1e-7                          # 2e-5 apart at most: one PCM step
    with pytest.raises(ValueError, match="inference_samples"):                              # a speech edit is not streamed
        CLI.main(["--model_path", lm_ckpt, "--codec_path", codec_ckpt, "--orig_audio", wav_fn, "--orig_transcript", "hello world",
                  "--target_transcript", "again", "--temp_folder", str(tmp_path / "tmp"), "--savename", "utt", "--seed", "11", "--top_k", "12",
                  "--top_p", "0.9", "--cfg_stride", "2", "--aug_text", "--mask_start", "0.20", "--mask_end", "0.30", "--phoneme_ids", ids("again"),
                  "--prompt_phoneme_ids", ids("hello world"), "--sample_batch_size", "2", "--output_dir", str(tmp_path / "edit"),
                  "--stream_dir", str(tmp_path / "chunks2")])


# ----------------------------------------------------------------------------------------------- one run at the 830M shape
def test_830m_8_utterances_with_cfg():
    """8 utterances x CFG (16 rows) at the 830M shape with the full codec, about 48 steps each: tokens equal `inference_batch`'s, the
    streamed samples are within 2e-5 of `decode` of each result at batch 1, and nothing is allocated while the steps run."""
    args = W.lm_args_830m()
    sd = W.lm_state_dict(args, seed=0, device="cuda")
    for k in range(args.n_codebooks):          # only codec ids leave the LM (bench.py build_api_model)
        b = sd[f"predict_layer.{k}.2.bias"].clone()
        b[int(args.audio_vocab_size):] = -30.0
        sd[f"predict_layer.{k}.2.bias"] = b
    m = SSR_Speech(args)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    del sd
    m = m.to("cuda").eval()
    ccfg = W.codec_config_full()
    tok = AudioTokenizer(device="cuda", config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=0))
    g = torch.Generator().manual_seed(83)
    jobs = []
    for u in range(8):
        P = 60 + 2 * u                                                     # step cap = 10 L + 2 - (P + 5) + K + 1 = 62 - 2u .. 48
        jobs.append({"x": torch.randint(0, 100, (1, 12), generator=g), "y": torch.randint(0, min(ccfg.bins, args.audio_vocab_size), (1, P, K), generator=g),
                     "mask_interval": torch.tensor([[[P, P]]], dtype=torch.long)})
    kw = dict(top_k=1, top_p=1.0, temperature=1, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True, seed=3)
    want = m.inference_batch(jobs, refill=False, **kw)
    held = {}

    def before_start(info):
        held["codec"] = tok.decode_stream_batch(info["prompt_lens"], info["max_new_frames"])
        return held["codec"].codes

    it = m.inference_batch_stream(jobs, bins=ccfg.bins, before_start=before_start, **kw)
    parts, n0 = [[] for _ in jobs], None
    for inc in it:
        if inc.kept:
            held["codec"].push_prompts(inc.codes)
            continue
        if n0 is None:
            n0 = _device_mallocs(m.device)                                 # the first poll: the prefill and 16 steps are behind us
        for u, chunk in enumerate(held["codec"].advance(inc.counts, inc.ended, flag=it.flag)):
            parts[u].append(chunk)
    assert _device_mallocs(m.device) == n0, "memory was mapped while the steps ran"
    assert it.polls >= 3
    for u, (got, ref) in enumerate(zip(it.results, want)):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3]
        P = int(jobs[u]["y"].shape[1])
        one = tok.codec.decode(ref[0])[..., P * ccfg.hop:]
        wav = torch.cat(parts[u], -1)
        assert wav.shape == one.shape and wav.shape[-1] > 0
        err = float((wav - one).abs().max())
        print(f"830M utterance {u}: {ref[0].shape[-1] - P} frames, max |stream - batch-1 decode| = {err:.3g}")
        assert err <= 2e-5, (u, err)
        assert sum(c.shape[-1] > 0 for c in parts[u]) >= 2
    for e in m._engines.values():
        e.close()
