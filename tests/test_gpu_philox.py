"""GPU: the opt-in device-side sampling noise (DESIGN.md Part I.21). The kernel (csrc/noise.hip) against the numpy replica
(`ssr_speech_amd/philox.py`): the raw words exactly, the values within 2^-22 relative of the float64 reference, nothing outside the segments
touched. The engine under `set_sampling_rng("philox")`: the noise the loop writes is the noise a direct call writes, the batch contract
(row i == the batch-1 run after `torch.manual_seed(seed + i)`) for every grouping, the streams equal their one-pass twins, the CPU generator
is left alone, nothing is staged, and "torch_cpu" is untouched. The oracle, fed the device-written noise, picks the same tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib, philox as P
from ssr_speech_amd import engine as E
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import lm as O

pytestmark = pytest.mark.gpu

SEGS = [(3, 5, 7, 2 ** 32 + 5), (0, 1, 16, 7), (4, 33, 7, 2 ** 63 + 11)]      # slots out of order, unequal lengths, the last ends AT max_steps
N_UTT, MAX_STEPS = 5, 40
KW = dict(top_k=40, top_p=0.8, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)


# ---------------------------------------------------------------- the kernel against the replica
@pytest.mark.parametrize("k, card", [(4, 2056), (4, 72), (3, 73)])
def test_kernel_equals_the_replica(k, card):
    noise = torch.full((N_UTT, MAX_STEPS, k, card), float("nan"), device="cuda")
    words = torch.full((N_UTT, MAX_STEPS, k, card), -1, dtype=torch.int32, device="cuda")
    E.philox_fill(noise, SEGS, words=words)
    torch.cuda.synchronize()
    got, got_w = noise.cpu().numpy(), words.cpu().numpy().view(np.uint32)
    inside = np.zeros(got.shape, dtype=bool)
    worst = 0.0
    for u, off, n, seed in SEGS:
        inside[u, off:off + n] = True
        want_w = P.words(seed, off, n, k, card)
        assert np.array_equal(got_w[u, off:off + n], want_w), (u, "raw words")                # the uniforms: exactly
        q64 = -np.log(P.uniforms(want_w))
        q = got[u, off:off + n].astype(np.float64)
        rel = np.abs(q - q64) / q64
        worst = max(worst, float(rel.max()))
        assert np.all(q > 0) and np.all(np.isfinite(q))
    print(f"K={k} card={card}: worst |q - q64| / q64 = {worst:.3e} = {worst * 2 ** 23:.3f} ulp (bound 2^-22 = {2.0 ** -22:.3e})")
    # 2 ulp: the library's logf is specified to 1 ulp, plus the final rounding
    assert worst <= 2.0 ** -22, worst
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()                   # nothing outside the segments was written
    assert np.all(got_w[~inside] == 0xFFFFFFFF)
    again = torch.full_like(noise, float("nan"))
    E.philox_fill(again, SEGS)
    torch.cuda.synchronize()
    assert torch.equal(again[torch.from_numpy(inside)], noise[torch.from_numpy(inside)])      # a second identical call: the same bits
    assert torch.isnan(again[torch.from_numpy(~inside)]).all()


def test_value_depends_on_seed_step_and_element_only():
    """the same (seed, steps) into another slot, through another split into segments and launches, and beside other segments"""
    k, card, seed = 4, 72, 2 ** 40 + 3
    a = torch.full((2, 32, k, card), float("nan"), device="cuda")
    b = torch.full((34, 32, k, card), float("nan"), device="cuda")
    E.philox_fill(a, [(1, 0, 24, seed)])
    segs = [(33, 0, 5, seed), (33, 5, 19, seed)] + [(u, 3, 2, u) for u in range(33)]          # 35 segments: two launches
    E.philox_fill(b, segs)
    torch.cuda.synchronize()
    assert torch.equal(a[1, :24], b[33, :24]) and torch.isnan(b[33, 24:]).all() and torch.isnan(a[0]).all()
    assert np.abs(b[7, 3:5].cpu().numpy().astype(np.float64) / P.exp_noise(7, 3, 2, k, card) - 1).max() <= 2.0 ** -22


def test_contract_errors_launch_nothing():
    L = _lib.lib()
    noise = torch.full((N_UTT, MAX_STEPS, 4, 72), float("nan"), device="cuda")

    def call(n_seg=1, slot=0, first=0, n=1, null=False):
        a = _lib.NoiseArgs()
        a.noise = 0 if null else noise.data_ptr()
        a.n_utt, a.max_steps, a.K, a.card, a.n_seg = N_UTT, MAX_STEPS, 4, 72, n_seg
        for i in range(min(max(n_seg, 0), _lib.NOISE_MAX_SEGMENTS)):
            a.seg[i].slot, a.seg[i].first_step, a.seg[i].n_steps = slot, first, n
        return L.ssrhip_noise_philox(C.byref(a), _lib.stream_ptr())

    assert call(null=True) < 0
    assert call(n_seg=33) < 0
    assert call(first=-1) < 0 and call(n=-1) < 0
    assert call(first=30, n=11) < 0
    assert call(slot=N_UTT) < 0 and call(slot=-1) < 0
    torch.cuda.synchronize()
    assert torch.isnan(noise).all()
    assert call(first=30, n=10) == 0                         # the same call inside the contract does write
    torch.cuda.synchronize()
    assert not torch.isnan(noise[0, 30:]).any() and torch.isnan(noise[0, :30]).all() and torch.isnan(noise[1:]).all()


# ---------------------------------------------------------------- the engine
def _model(seed=21):
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = SSR_Speech(args)
    m.load_state_dict(W.lm_state_dict(args, seed=seed))
    return args, m.to("cuda").eval()


def _utterances(n, tts_only=False):
    g = torch.Generator().manual_seed(3)
    utts = []
    for (L, T) in [(9, 14), (13, 22), (6, 10), (11, 17), (7, 12)][:n]:
        utts.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    if not tts_only and n > 1:
        utts[1]["mask_interval"] = torch.LongTensor([[[5, 9]]])                                # one of them is an edit, the others TTS
    return utts


def _one(m, u, **extra):
    L = u["x"].shape[1]
    kw = dict(KW, **extra)
    return m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                       u["mask_interval"].cuda(), kvcache=1, **kw)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


@pytest.fixture(scope="module")
def philox_model():
    args, m = _model()
    m.set_sampling_rng("philox")
    return args, m


@pytest.fixture(scope="module")
def batch1_runs(philox_model):
    """utterance i alone under torch.manual_seed(300 + i): computed once, read by the tests below (10, 92, 45, 83 and 49 steps: up to six
    16-step chunks, every refill of the 2-slot queue lands in a slot that has drawn further than the newcomer will)"""
    _, m = philox_model
    outs = []
    for i, u in enumerate(_utterances(5)):
        torch.manual_seed(300 + i)
        outs.append(_one(m, u))
    return outs


@pytest.mark.parametrize("use_graph", [False, True])
def test_loop_noise_is_the_direct_calls_noise_at_every_step(philox_model, use_graph):
    """The engine's own loop under PhiloxNoise, polled after every step so that the post-edit logits of each step can be kept, against a
    second run that is handed `noise=` the tensor ONE direct ssrhip_noise_philox call wrote for the same seed: equal logits at every
    step, equal tokens. Then the public `inference` (16-step chunks) gives these tokens too."""
    args, m = philox_model
    u = _utterances(1)[0]
    seed = 2 ** 33 + 17
    torch.manual_seed(seed)
    unc = torch.randint(0, args.text_vocab_size + 1, (1, u["x"].shape[1]))
    arena = E.LMWeightsArena(args, W.lm_state_dict(args, seed=21, device="cuda"), torch.device("cuda"))
    eng = E.DecodeEngine(arena, 1, True, 1024, 256, debug_logits=True)
    cated, _, num_task, _ = LY.build_layout(u["y"][0].numpy().T, u["mask_interval"][0].numpy(), args)
    rows = [u["x"][0].numpy(), unc[0].numpy()]
    kn = E.DecodeKnobs(top_k=KW["top_k"], top_p=KW["top_p"], temperature=1.0, stop_repetition=2, silence_tokens=(3, 7, 11), cfg_coef=1.5,
                       cfg_stride=2, use_cfg=True, text_len=u["x"].shape[1], n_spans=num_task, seed=seed)

    def run(feed, **start_kw):
        eng.start(rows, [cated], [kn], **start_kw)
        logits = []
        for states in eng.iter_chunks(chunk=1, use_graph=use_graph, max_total=120, feed=feed):
            logits.append(eng.dbg_logits[0].clone())
        st = states[0]
        assert st.done == 1
        return logits[: int(st.n_steps)], eng.tokens(0, int(st.n_steps))

    src = E.PhiloxNoise([seed])
    log_a, tok_a = run(src, host_noise=True)
    assert src.drawn == [len(tok_a)] and eng._uploader is None
    direct = torch.full((1, eng.max_steps, args.n_codebooks, arena.card), float("nan"), device="cuda")
    E.philox_fill(direct, [(0, 0, eng.max_steps, seed)])
    log_b, tok_b = run(None, noise=direct)
    assert len(tok_a) > 8 and np.array_equal(tok_a, tok_b)
    assert len(log_a) == len(log_b) and all(torch.equal(a, b) for a, b in zip(log_a, log_b))
    # the public path: 16-step chunks, the seed from the global generator, the unconditional text drawn from it
    torch.manual_seed(seed)
    res = _one(m, u)
    assert m.last_run["steps"] == len(tok_a)
    meng = next(iter(m._engines.values()))
    assert np.array_equal(meng.tokens(0, len(tok_a)), tok_a)
    res_n = _one(m, u, noise=direct[0], uncond_x=unc)        # an explicit noise= wins over the setting
    assert _same(res, res_n)
    eng.close()


@pytest.mark.parametrize("how", [dict(group=2), dict(group=2, refill=False), dict(group=5)])
def test_batch_rows_equal_the_batch1_runs(philox_model, batch1_runs, how):
    _, m = philox_model
    batch = m.inference_batch(_utterances(5), seed=300, **KW, **how)
    eng = next(iter(m._engines.values()))
    if how == dict(group=2):
        assert eng.n_refills >= 3                            # 5 utterances through 2 slots
    assert len(batch) == 5
    for i, (got, one) in enumerate(zip(batch, batch1_runs)):
        assert _same(got, one), i
    assert len({tuple(r[0].cpu().numpy().reshape(-1).tolist()) for r in batch}) == 5          # five seeds, five results


def test_streams_equal_their_one_pass_twins(philox_model, batch1_runs):
    _, m = philox_model
    u = _utterances(5)[3]                                    # 83 steps
    torch.manual_seed(303)
    L = u["x"].shape[1]
    it = m.inference_stream(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                            u["mask_interval"].cuda(), kvcache=1, **KW)
    incs = list(it)
    assert len(incs) > 3 and _same(it.result, batch1_runs[3])
    utts = _utterances(3, tts_only=True)
    want = m.inference_batch(utts, seed=300, refill=False, **KW)
    bit = m.inference_batch_stream(utts, seed=300, **KW)
    list(bit)
    assert bit.polls >= 3 and len(bit.results) == 3 and all(_same(a, b) for a, b in zip(bit.results, want))


def test_cpu_generator_untouched_and_nothing_staged():
    """a model that has only ever run under "philox": without aug_text no draw is made on the CPU generator; no uploader (pinned staging,
    copy stream) exists on any engine; greedy runs ignore the setting"""
    _, m = _model()
    m.set_sampling_rng("philox")
    u = _utterances(1)[0]
    kw = dict(aug_text=False)
    torch.manual_seed(77)
    before = torch.get_rng_state()
    a = _one(m, u, **kw)
    assert torch.equal(torch.get_rng_state(), before)
    batch = m.inference_batch(_utterances(3), seed=77, **dict(KW, **kw))
    assert torch.equal(torch.get_rng_state(), before)
    assert _same(batch[0], a)                                # seed 77 + 0, the same utterance
    assert m._engines and all(e._uploader is None and isinstance(e._feed, E.PhiloxNoise) for e in m._engines.values())
    greedy = dict(top_k=1, top_p=1.0, aug_text=False)
    g_philox = _one(m, u, **greedy)
    assert all(e._uploader is None and e._feed is None for e in m._engines.values())
    m.set_sampling_rng("torch_cpu")
    assert _same(_one(m, u, **greedy), g_philox)


def test_torch_cpu_set_back_equals_a_model_that_never_saw_the_setter():
    _, fresh = _model()
    _, m = _model()
    u = _utterances(2)[1]
    m.set_sampling_rng("philox")
    torch.manual_seed(9)
    p = _one(m, u)
    m.set_sampling_rng("torch_cpu")
    outs = []
    for model in (m, fresh):
        torch.manual_seed(9)
        outs.append((_one(model, u), torch.get_rng_state()))
    assert _same(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert p is not None                                     # (other noise: nothing is claimed about p against the torch_cpu tokens)
    want = fresh.inference_batch(_utterances(3), seed=9, **KW)
    got = m.inference_batch(_utterances(3), seed=9, **KW)
    assert all(_same(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------- the oracle on the device-written noise
def test_oracle_fed_the_device_noise_picks_the_same_tokens(philox_model):
    args, m = philox_model
    u = _utterances(2)[1]                                    # the edit
    seed = 2 ** 32 + 1234
    torch.manual_seed(seed)
    got = _one(m, u)
    steps = int(m.last_run["steps"])
    card = args.audio_vocab_size + args.n_special + args.max_n_spans
    noise = torch.full((1, steps, args.n_codebooks, card), float("nan"), device="cuda")
    E.philox_fill(noise, [(0, 0, steps, seed)])
    host = noise[0].cpu()
    torch.manual_seed(seed)                                  # the oracle draws the unconditional text as the model did
    kw = {k: v for k, v in KW.items()}
    ref = O.inference(O.reference_params(W.lm_state_dict(args, seed=21)), args, u["x"], u["y"], u["mask_interval"], kvcache=1,
                      noise_fn=lambda s: host[s], **kw)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3]
