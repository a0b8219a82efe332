"""GPU: per-token log-probabilities from the decode sampler (DESIGN.md Part I.27) — `ssrhip_sample_logp` against fp64 over every path of
the state machine and at the card's edges, the engine against the reference's fixtures, batches with refill and on the matrix-core rows,
the switched-off default, and the sample scores of `inference_samples`.

A kernel-level value is compared with fp64 computed from the SAME fp32 logits, per entry, within

    tol_k = (card + 16) * 2^-24 + 2^-22 * |ref|

— the worst-case rounding of a card-term fp32 sum plus expf / logf, and the subtraction. Derived, not measured."""
import argparse
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import inference_scale as S
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.data.tokenizer import write_wav
from test_gpu_lm import LOGIT_ATOL, _load, _model

pytestmark = pytest.mark.gpu
CANARY = -77.0
SENTINEL = -77


def tol_k(card, ref):
    return (card + 16) * 2.0 ** -24 + 2.0 ** -22 * np.abs(ref)


def ref_logp(edited, temperature, tokens):
    """fp64 log_softmax(fp32(edited / T))[token] per codebook: edited [K, card] fp32 (what the sampler's edits left), tokens [K]"""
    z = np.asarray(edited, dtype=np.float32)
    if temperature != 1.0:
        z = z / np.float32(temperature)                     # fp32 division, round to nearest: what the kernel does
    z = z.astype(np.float64)
    m = z.max(-1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(-1))
    return z[np.arange(z.shape[0]), np.asarray(tokens)] - lse


def forced_rule(num_gen, num_eog, audio_pos, K, argmax0, eog, text_len):
    """The positions of a step the state machine decides, from the state at kernel entry (include/ssrhip.h ssrhip_sample_logp)."""
    return np.array([(num_gen < K - 1 and k > num_gen) or (num_eog > 0 and k <= num_eog) or
                     (num_eog == 0 and k == 0 and (argmax0 == eog or audio_pos + 1 > 10 * text_len)) for k in range(K)])


# ---------------------------------------------------------------------------------------------------------------- the kernel, stepped
def _drive(args, K, knobs, logits_seq, noise, *, text_len, audio_pos0, max_steps, logp, embed=None, preset_done=()):
    """ssrhip_sample (logp False) or ssrhip_sample_logp (True) on len(knobs) utterances, one launch per entry of logits_seq ([rows, K,
    card]); noise [n_utt, max_steps, K, card]. Every output buffer starts as SENTINEL / CANARY. Stops once every utterance is done.
    Returns one dict of host copies per launch: pre (the states before it), state (bytes), generated, next_tok, next_pos, kv_pos,
    row_len, dbg, logp, x."""
    L = _lib.lib()
    n_utt = len(knobs)
    card = args.audio_vocab_size + args.n_special + args.max_n_spans
    rows = [2 if kn["aug_text"] else 1 for kn in knobs]
    assert len(set(rows)) == 1
    B = rows[0] * n_utt
    cfgs, sts = (_lib.SamplerCfg * n_utt)(), (_lib.SamplerState * n_utt)()
    for u, kn in enumerate(knobs):
        c, st = cfgs[u], sts[u]
        c.top_k, c.top_p, c.temperature, c.stop_repetition = kn["top_k"], kn["top_p"], kn["temperature"], kn["stop_repetition"]
        c.cfg_coef, c.cfg_one_minus, c.cfg_stride, c.use_cfg = kn["cfg_coef"], 1 - kn["cfg_coef"], kn["cfg_stride"], int(kn["aug_text"])
        c.n_silence = len(kn["silence_tokens"])
        for i, t in enumerate(kn["silence_tokens"]):
            c.silence[i] = t
        c.text_len, c.n_spans, c.max_steps, c.use_noise = text_len, 1, max_steps, 1
        c.empty_token, c.eog, c.eos, c.sos, c.mts, c.max_n_spans = args.empty_token, args.eog, args.eos, args.sos, args.mts, args.max_n_spans
        st.num_cfg_tag, st.prev_token, st.audio_pos, st.done = 1, -1, audio_pos0, int(u in preset_done)
    dcfg = torch.frombuffer(bytearray(bytes(cfgs)), dtype=torch.uint8).cuda()
    dst = torch.frombuffer(bytearray(bytes(sts)), dtype=torch.uint8).cuda()
    dnoise = noise.float().contiguous().cuda()
    full = lambda *shape, dtype=torch.int32, v=SENTINEL: torch.full(shape, v, dtype=dtype, device="cuda")
    gen, next_tok, next_pos, row_len = full(n_utt, max_steps, K), full(B, 4), full(B), full(B)
    kv_pos = torch.arange(5, 5 + B, dtype=torch.int32, device="cuda")
    dbg = full(n_utt, K, card, dtype=torch.float32)
    lp = full(n_utt, max_steps, K, dtype=torch.float32, v=CANARY)
    a = _lib.SampleArgs()
    a.n_utt, a.K, a.card, a.cfg, a.state, a.noise = n_utt, K, card, dcfg.data_ptr(), dst.data_ptr(), dnoise.data_ptr()
    a.generated, a.next_tok, a.next_pos, a.kv_pos, a.row_len, a.dbg_logits = gen.data_ptr(), next_tok.data_ptr(), next_pos.data_ptr(), kv_pos.data_ptr(), row_len.data_ptr(), dbg.data_ptr()
    x = None
    if embed is not None:
        D, audio_emb, pe = embed
        dae, dpe = audio_emb.cuda(), pe.cuda()
        x = full(16, D, dtype=torch.float32)
        e = a.embed
        e.audio_emb, e.pe, e.alpha_audio, e.R, e.D, e.K, e.card, e.out, e.out_tiled = dae.data_ptr(), dpe.data_ptr(), 0.7, B, D, K, card, x.data_ptr(), 0
    states = lambda: list((_lib.SamplerState * n_utt).from_buffer_copy(dst.cpu().numpy().tobytes()))
    out = []
    for lg in logits_seq:
        pre = states()
        if all(s.done for s in pre):
            break
        dl = lg.float().contiguous().cuda()
        a.logits = dl.data_ptr()
        if logp:
            _lib.check(L.ssrhip_sample_logp(C.byref(a), lp.data_ptr(), _lib.stream_ptr()), "ssrhip_sample_logp")
        else:
            _lib.check(L.ssrhip_sample(C.byref(a), _lib.stream_ptr()), "ssrhip_sample")
        torch.cuda.synchronize()
        out.append(dict(pre=pre, state=dst.cpu().numpy().tobytes(), generated=gen.cpu().numpy(), next_tok=next_tok.cpu().numpy(),
                        next_pos=next_pos.cpu().numpy(), kv_pos=kv_pos.cpu().numpy(), row_len=row_len.cpu().numpy(), dbg=dbg.cpu().numpy(),
                        logp=lp.cpu().numpy(), x=None if x is None else x.cpu().numpy()))
    return out


SAME = ("generated", "state", "next_tok", "next_pos", "kv_pos", "row_len", "dbg", "x")


def _assert_same_run(with_lp, plain):
    """the run with the output against ssrhip_sample on fresh buffers: everything but the output, bit for bit, after every step"""
    assert len(with_lp) == len(plain)
    for s, (o, p) in enumerate(zip(with_lp, plain)):
        for name in SAME:
            if o[name] is None:
                assert p[name] is None
            elif isinstance(o[name], bytes):
                assert o[name] == p[name], (s, name)
            else:
                assert np.array_equal(o[name].view(np.int32), p[name].view(np.int32)), (s, name)
        assert (p["logp"] == CANARY).all()


def _check_step(o, prev_logp, u, s, K, card, args, temperature, text_len):
    """row s of utterance u after the launch that wrote it: NaN exactly where the rule says, fp64 within tol_k elsewhere; returns the
    (mask, worst error / tolerance)"""
    st = o["pre"][u]
    assert st.n_steps == s and not st.done
    edited = o["dbg"][u]
    mask = forced_rule(st.num_gen, st.num_eog, st.audio_pos, K, int(np.argmax(edited[0])), args.eog, text_len)
    got = o["logp"][u, s]
    assert np.array_equal(np.isnan(got), mask), (u, s, got, mask)
    ref = ref_logp(edited, temperature, o["generated"][u, s])
    err, tol = np.abs(got.astype(np.float64) - ref)[~mask], tol_k(card, ref)[~mask]
    assert (err <= tol).all(), (u, s, got, ref, err, tol)
    # nothing but this row changed in this utterance's block
    before = prev_logp[u].copy()
    before[s] = got
    assert np.array_equal(before.view(np.int32), o["logp"][u].view(np.int32)), (u, s)
    return mask, float((err / tol).max()) if err.size else 0.0


@pytest.mark.parametrize("case", ["greedy_cfg", "topk_topp", "topp_temp", "silence", "nocfg_topk"])
def test_kernel_against_fp64_over_the_state_machine_scripts(golden_dir, case):
    """The five scripted runs of tests/golden/sampler_script.npz (start-of-span delay, stop by argmax and by the length cap, eog cascade,
    silence penalty, temperature, top-k / top-p, with and without CFG) through ssrhip_sample_logp, step by step."""
    from tests_script_knobs import SCRIPT_KNOBS
    g = np.load(os.path.join(golden_dir, "sampler_script.npz"))
    args = W.lm_args_tiny()
    K, card = args.n_codebooks, args.audio_vocab_size + args.n_special + args.max_n_spans
    kn = dict(SCRIPT_KNOBS[case], silence_tokens=[3, 7, 11])
    logits, noise = torch.from_numpy(g[f"{case}_logits"]), torch.from_numpy(g[f"{case}_noise"])
    text_len, audio_pos0 = int(g[f"{case}_text_len"]), int(g[f"{case}_audio_pos0"])
    Sn = logits.shape[0]
    run = functools.partial(_drive, args, K, [kn], [l for l in logits], noise.unsqueeze(0), text_len=text_len, audio_pos0=audio_pos0, max_steps=Sn)
    got, plain = run(logp=True), run(logp=False)
    assert len(got) == Sn
    _assert_same_run(got, plain)
    assert np.array_equal(got[-1]["generated"][0], g[f"{case}_samples"])           # (the fixture's tokens, as in the existing test)
    prev = np.full((1, Sn, K), CANARY, dtype=np.float32)
    kinds, worst, n_forced = set(), 0.0, 0
    for s, o in enumerate(got):
        np.testing.assert_array_equal(o["dbg"][0], g[f"{case}_edited_logits"][s])
        mask, w = _check_step(o, prev, 0, s, K, card, args, kn["temperature"], text_len)
        prev, worst, n_forced = o["logp"], max(worst, w), n_forced + int(mask.sum())
        st = o["pre"][0]
        kinds |= {"delay"} if (st.num_gen < K - 1) else set()
        kinds |= {"cascade"} if st.num_eog > 0 else set()
        kinds |= {"stop"} if (st.num_eog == 0 and mask[0]) else set()
    print(f"{case}: {Sn} steps, {n_forced} forced entries ({sorted(kinds)}), worst |err| / tol_k = {worst:.3f}")
    assert {"delay", "cascade"} <= kinds and n_forced < Sn * K


def _edge_script(card, K, Sn=6):
    """three utterances with CFG, knobs of their own (greedy | top-k + top-p | top-p at temperature 2); no stop inside the script. From
    step K on, utterance 0 holds one entry at +10000 in every codebook (both rows) and utterance 2 two equal entries above all others."""
    args = W.lm_args_tiny() if card == 72 else (W.lm_args_830m() if card == 2056 else W.lm_args_tiny(vocab=card - 8))
    assert card == args.audio_vocab_size + args.n_special + args.max_n_spans
    sil = [3, 7, 11]
    knobs = [dict(kn, stop_repetition=2, silence_tokens=sil, cfg_coef=1.5, cfg_stride=2, aug_text=True)
             for kn in (dict(top_k=1, top_p=1.0, temperature=1.0), dict(top_k=12, top_p=0.8, temperature=1.0), dict(top_k=0, top_p=0.7, temperature=2.0))]
    g = torch.Generator().manual_seed(card + K)
    logits = torch.randn(Sn, 3, 2, K, card, generator=g) * 2.0
    logits[..., args.eog] -= 30.0
    hot = [int(torch.randint(12, args.audio_vocab_size, (1,), generator=g)) for _ in range(K)]          # (12: behind the silence tokens)
    tie = [sorted((12 + torch.randperm(args.audio_vocab_size - 12, generator=g)[:2]).tolist()) for _ in range(K)]
    for s in range(K, Sn):
        for k in range(K):
            logits[s, 0, :, k, hot[k]] = 10000.0
            logits[s, 2, :, k, tie[k][0]] = logits[s, 2, :, k, tie[k][1]] = 30.0
    noise = torch.empty(3, Sn + 2, K, card).exponential_(1, generator=g)
    D = 64
    emb = (D, torch.randn(K, card, D, generator=g), torch.randn(8 + Sn + 2, D, generator=g))
    return args, knobs, [logits[s].reshape(6, K, card) for s in range(Sn)], noise, emb, hot, tie


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("K", [4, 1])
@pytest.mark.parametrize("card", [72, 2056, 2304])
def test_kernel_at_the_card_edges_with_a_done_neighbour(card, K, fused):
    """card 72 (not a multiple of 64: one partly filled element slot), 2056 (the 830M card: nine slots, the last partly) and 2304 (the
    kernel's limit: every slot of every lane); K = 4 and 1; three utterances, the middle one done on entry — its rows keep the canary; an
    entry at +10000 (log-probability 0) and exact ties at the top; with and without the fused embed (the barrier the output shares)."""
    args, knobs, seq, noise, emb, hot, tie = _edge_script(card, K)
    Sn = len(seq)
    run = functools.partial(_drive, args, K, knobs, seq, noise, text_len=100, audio_pos0=8, max_steps=Sn + 2, embed=emb if fused else None,
                            preset_done=(1,))
    got, plain = run(logp=True), run(logp=False)
    assert len(got) == Sn
    _assert_same_run(got, plain)
    prev = np.full((3, Sn + 2, K), CANARY, dtype=np.float32)
    worst = 0.0
    for s, o in enumerate(got):
        for u in (0, 2):
            mask, w = _check_step(o, prev, u, s, K, card, args, knobs[u]["temperature"], 100)
            worst = max(worst, w)
            assert mask.sum() == max(K - 1 - s, 0)
        assert (o["logp"][1] == CANARY).all() and (o["generated"][1] == SENTINEL).all()
        prev = o["logp"]
        if s >= K:
            assert o["generated"][0, s].tolist() == hot and (np.abs(o["logp"][0, s]) <= tol_k(card, 0.0)).all()   # certain: log-probability 0
            for k in range(K):
                assert int(o["generated"][2, s, k]) in tie[k]                     # the draw picks among the two equal entries (top_p 0.7 keeps both)
    print(f"card {card} K {K} fused {fused}: worst |err| / tol_k = {worst:.3f}")


def test_null_buffer_is_an_argument_error_not_a_launch():
    L = _lib.lib()
    a = _lib.SampleArgs()
    gen = torch.full((1, 4, 4), SENTINEL, dtype=torch.int32, device="cuda")
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    a.logits = a.cfg = a.state = a.next_tok = a.next_pos = a.kv_pos = a.row_len = buf.data_ptr()
    a.generated, a.n_utt, a.K, a.card = gen.data_ptr(), 1, 4, 72
    assert L.ssrhip_sample_logp(C.byref(a), None, _lib.stream_ptr()) < 0
    assert b"ssrhip_sample_logp" in L.ssrhip_last_error() and b"logp" in L.ssrhip_last_error()
    torch.cuda.synchronize()
    assert (gen == SENTINEL).all() and (buf == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the engine
def _replay_forced(tokens, logits, K, eog, text_len, audio_pos0):
    """The sampler's counters replayed on the host over the steps of one utterance (all its spans): forced mask [S, K]."""
    num_gen = num_eog = 0
    ap, out = audio_pos0, []
    for s in range(tokens.shape[0]):
        out.append(forced_rule(num_gen, num_eog, ap, K, int(np.argmax(logits[s, 0])), eog, text_len))
        if num_eog > 0:
            num_eog += 1
        elif tokens[s, 0] == eog:
            num_eog = 1
        num_gen += 1
        ap += 1
        if num_eog == K:                                   # span hand-over: the counters start again
            num_gen = num_eog = 0
    return np.stack(out)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["tts_sample_topp_temp", "edit_3span_greedy"])
def test_inference_logprobs_against_the_reference_fixtures(golden_dir, name, use_graph):
    g, args, kw = _load(golden_dir, name)
    m = _model(args, int(g["weight_seed"]))
    K, card = args.n_codebooks, args.audio_vocab_size + args.n_special + args.max_n_spans
    Lx = g["x"].shape[1]
    x, y = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
    extra = dict(uncond_x=torch.from_numpy(g["uncond_x"]))
    if "sample" in name:
        extra["noise"] = torch.from_numpy(g["step_noise"])
    px, py = torch.from_numpy(g["prompt_x"]).cuda(), torch.from_numpy(g["prompt"]).cuda()
    out = m.inference(x, torch.LongTensor([Lx]).cuda(), px, torch.LongTensor([px.shape[1]]).cuda(), y, py, torch.from_numpy(g["mask_interval"]).cuda(),
                      use_graph=use_graph, return_logprobs=True, **kw, **extra)
    assert len(out) == 5
    res, marks, masks, nmi, lp = out
    assert np.array_equal(res.cpu().numpy(), g["res"]) and np.array_equal(marks.numpy(), g["marks"])
    assert np.array_equal(np.asarray(masks), g["masks"]) and np.array_equal(np.asarray(nmi), g["non_mask_intervals"])
    eng = next(iter(m._engines.values()))
    assert eng.want_logprobs and eng.lib.ssrhip_lm_logprobs(eng._ctx) == 1
    logits, T = g["step_logits"], float(kw["temperature"])
    Sn = logits.shape[0]
    tokens = eng.tokens(0, Sn)                              # what was written to `generated` (the fixture's res, checked above, holds them)
    assert m.last_run["steps"] == Sn
    assert isinstance(lp, LY.TokenLogprobs) and lp.steps.shape == (Sn, K) and lp.steps.dtype == np.float32
    cated = LY.build_layout(g["y"][0].T, g["mask_interval"][0], args)[0]
    mask = _replay_forced(tokens, logits, K, args.eog, Lx, cated.shape[1])
    assert np.array_equal(np.isnan(lp.steps), mask)
    assert np.array_equal(tokens[~mask], g["step_samples"][..., 0][~mask])         # where the draw decided, the reference drew the same
    ref = np.stack([ref_logp(logits[s], T, tokens[s]) for s in range(Sn)])
    err, tol = np.abs(lp.steps - ref)[~mask], (2 * LOGIT_ATOL / T + tol_k(card, ref))[~mask]
    print(f"{name} graph={use_graph}: {Sn} steps, {int(mask.sum())} forced, worst |err| = {err.max():.2e} (tolerance there {tol[err.argmax()]:.2e})")
    assert (err <= tol).all()
    # frames: aligned with res — NaN exactly at the kept frames and the forced entries, the same finite values as `steps`
    assert lp.frames.shape == (1,) + g["res"].shape[1:] and lp.frames.dtype == np.float32
    ends = [0] + [int(e) for e in m.last_run["span_end"][: len(nmi) - 1]]
    idx = np.arange(Sn * K, dtype=np.int64).reshape(Sn, K)
    where = LY.assemble(np.full(g["y"][0].T.shape, -1, dtype=np.int64), [idx[ends[i]:ends[i + 1]] for i in range(len(ends) - 1)],
                        [tuple(r) for r in g["non_mask_intervals"]], args)[0]          # the step * K + codebook behind every frame, -1 = kept
    want_nan = (where < 0) | mask.reshape(-1)[np.maximum(where, 0)]
    assert np.array_equal(np.isnan(lp.frames[0]), want_nan)
    assert np.array_equal(np.isnan(lp.frames[0]).all(0), g["marks"][0] == 0)
    fin = ~np.isnan(lp.frames[0])
    assert np.array_equal(lp.frames[0][fin], lp.steps.reshape(-1)[where[fin]])
    in_frames = np.zeros(Sn * K, dtype=bool)
    in_frames[where[where >= 0]] = True
    # drawn entries of no frame: only an eog that codebook 0 drew (no stop rule fired) — it sits in the eog column `assemble` drops
    drawn_outside = (~mask.reshape(-1) & ~in_frames).reshape(Sn, K)
    assert not drawn_outside[:, 1:].any() and (tokens[:, 0][drawn_outside[:, 0]] == args.eog).all()
    assert sorted(lp.frames[0][fin].tolist()) == sorted(lp.steps[~mask & ~drawn_outside].tolist())
    assert lp.count == int((~mask).sum()) and lp.total == float(lp.steps[~mask].astype(np.float64).sum()) and lp.mean == lp.total / lp.count


def _utts(n, g):
    out = []
    for (L, T) in [(5, 6), (7, 9), (4, 5)][:n]:
        out.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                        mask_interval=torch.LongTensor([[[T, T]]])))
    return out


@pytest.mark.parametrize("aug_text,group,rows", [(False, 2, 2), (True, 3, 6)])
def test_batch_logprobs_equal_the_batch1_runs(aug_text, group, rows):
    """Three short utterances through two slots without CFG (2 rows, one refill) and through three slots with CFG (6 rows: the
    matrix-core step): the tokens of the call without the keyword, and per utterance the NaN mask and — within the bound the suite
    grants the logits of two engines, twice, plus tol_k — the values of `inference(return_logprobs=True)` of that utterance alone."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 21)
    card = args.audio_vocab_size + args.n_special + args.max_n_spans
    utts = _utts(3, torch.Generator().manual_seed(3))
    T = 1.5
    kw = dict(top_k=12, top_p=0.9, temperature=T, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=aug_text)
    plain = m.inference_batch(utts, seed=100, group=group, **kw)
    assert all(len(r) == 4 for r in plain)
    batch = m.inference_batch(utts, seed=100, group=group, return_logprobs=True, **kw)
    eng = next(iter(m._engines.values()))
    assert eng.B == rows and eng.want_logprobs and eng.n_admitted == 3 and eng.n_refills == 3 - group
    assert len(eng.queue_logprobs) == 3
    for i, u in enumerate(utts):
        assert len(batch[i]) == 5
        assert torch.equal(batch[i][0], plain[i][0]) and torch.equal(batch[i][1], plain[i][1]) and batch[i][2:4] == plain[i][2:4], i
        assert np.array_equal(eng.queue_logprobs[i].view(np.int32), batch[i][4].steps.view(np.int32)), i      # one entry per job, in job order
    for i, u in enumerate(utts):
        torch.manual_seed(100 + i)
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, return_logprobs=True, **kw)
        assert torch.equal(batch[i][0], one[0])
        a, b = batch[i][4], one[4]
        assert a.steps.shape == b.steps.shape and np.array_equal(np.isnan(a.steps), np.isnan(b.steps)) and a.count == b.count > 0
        ok = ~np.isnan(b.steps)
        err = np.abs(a.steps[ok].astype(np.float64) - b.steps[ok])
        tol = 2 * LOGIT_ATOL / T + tol_k(card, b.steps[ok].astype(np.float64))
        print(f"rows {rows} utterance {i}: {a.count} drawn tokens, worst |batch - alone| = {err.max():.2e}")
        assert (err <= tol).all(), (i, err.max())
        assert np.array_equal(np.isnan(a.frames), np.isnan(b.frames)) and a.frames.shape == (1,) + tuple(batch[i][0].shape[1:])


def test_off_means_off():
    """A model that never asks: 4-tuples, an engine without the buffer whose step ends in ssrhip_sample; and the setter is refused once
    the step is captured."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 21)
    u = _utts(1, torch.Generator().manual_seed(4))[0]
    L = u["x"].shape[1]
    call = lambda **k: m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                                   u["mask_interval"].cuda(), top_k=1, stop_repetition=2, aug_text=False, **k)
    out = call()
    assert len(out) == 4
    assert len(m._engines) == 1
    eng = next(iter(m._engines.values()))
    assert eng.logp is None and not eng.want_logprobs and eng.lib.ssrhip_lm_logprobs(eng._ctx) == 0
    with pytest.raises(RuntimeError, match="logprobs=True"):
        eng.logprobs(0, 1)
    buf = torch.zeros(eng.n_utt, eng.max_steps, args.n_codebooks, device="cuda")
    assert eng.lib.ssrhip_lm_set_logprobs(eng._ctx, buf.data_ptr()) < 0                    # the step was captured by the run above
    assert b"ssrhip_lm_set_logprobs" in eng.lib.ssrhip_last_error() and b"captured" in eng.lib.ssrhip_last_error()
    assert eng.lib.ssrhip_lm_logprobs(eng._ctx) == 0
    out5 = call(return_logprobs=True)                                                      # another engine; the tokens are the same
    assert len(out5) == 5 and torch.equal(out5[0], out[0])
    eng5 = next(iter(m._engines.values()))
    assert eng5 is not eng and eng5.logp is not None and eng5.lib.ssrhip_lm_logprobs(eng5._ctx) == 1
    assert len(call()) == 4 and next(iter(m._engines.values())).logp is None               # and back: the flag is part of the engine's key


# ---------------------------------------------------------------------------------------------------------------- a reused engine
def _two_utterances():
    """The sample-score test's model and two utterances for it: 15 and 35 phonemes behind prompts of 20 and 17 frames (the length rule
    lets them generate 131 and 334 steps). Under CFG they are the 4 rows of one engine; rows of 36 and 53 positions that generate past
    position 128, into the second page of their caches."""
    from test_gpu_stream_batch import FakePhonemizer, PHN2NUM, _pipeline
    args, m, _ = _pipeline()
    g = torch.Generator().manual_seed(27)
    utts = []
    for text, T in (("hello world again", 20), ("a much longer line of text to read out loud", 17)):
        utts.append({"x": S._phoneme_ids(FakePhonemizer(), PHN2NUM, text), "y": torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g),
                     "mask_interval": torch.LongTensor([[[T, T]]])})
    return args, m, utts


def _assert_same_bits(runs, names):
    """runs: one tuple of arrays per decode; every decode equals the first one bit for bit"""
    for i, run in enumerate(runs[1:], 1):
        for name, got, want in zip(names, run, runs[0]):
            got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
            assert got.shape == want.shape, (i, name)
            same = got.view(np.int32) == want.view(np.int32) if got.dtype == np.float32 else got == want
            assert same.all(), (f"decode {i} against decode 0", name, int((~same).sum()), "of", same.size)


def test_a_hand_stepped_decode_does_not_depend_on_what_its_engine_decoded_before():
    """ONE engine, two utterances under CFG (4 rows: the row-per-wave merge prologue, d_model 128), fixed noise, 110 single steps, four
    times over; before the fourth, `part_ml` — the buffer DESIGN.md Part I.27 traced the difference to — is filled with 3.0e38. The
    logits handed to the sampler after every step, the tokens and the log-probabilities of all four decodes are the same bits."""
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
    args, m, utts = _two_utterances()
    arena = LMWeightsArena(args, m.state_dict(), torch.device("cuda"))
    K, steps = args.n_codebooks, 110
    g = torch.Generator().manual_seed(28)
    rows, cols, knobs = [], [], []
    for u, ut in enumerate(utts):
        Lx = ut["x"].shape[1]
        cated, _, num_task, _ = LY.build_layout(ut["y"][0].T.numpy(), ut["mask_interval"][0].numpy(), args)
        rows += [ut["x"][0].numpy(), torch.randint(0, args.text_vocab_size + 1, (Lx,), generator=g).numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=40, top_p=0.8, temperature=1.0, stop_repetition=2, silence_tokens=(3, 7, 11), cfg_coef=1.5, cfg_stride=2,
                                 use_cfg=True, text_len=Lx, n_spans=num_task, seed=11 + u))
    noise = torch.empty(2, steps, K, arena.card).exponential_(1, generator=g).cuda()
    eng = DecodeEngine(arena, 2, True, 256, 128, debug_logits=True, logprobs=True)
    assert eng.B == 4 and eng.max_pages >= 2

    def decode():
        eng.start(rows, cols, knobs, noise=noise)
        logits = []
        for _ in range(steps):
            eng.decode(1, use_graph=True)
            torch.cuda.synchronize()
            logits.append(eng.dbg_logits.clone())
        assert int(eng.row_len.min()) > _lib.PAGE and not any(s.done for s in eng.states())       # every row crossed into its second page
        return (torch.stack(logits).cpu().numpy(), np.stack([eng.tokens(u, steps) for u in range(2)]),
                np.stack([eng.logprobs(u, steps) for u in range(2)]))

    try:
        runs = [decode() for _ in range(3)]
        eng.part_ml.fill_(3.0e38)
        runs.append(decode())
    finally:
        eng.close()
    assert np.isfinite(runs[0][0]).any() and np.isfinite(runs[0][2]).any()
    _assert_same_bits(runs, ("logits", "tokens", "logprobs"))


def test_a_queued_decode_does_not_depend_on_what_its_engine_decoded_before():
    """The same through `inference_batch` (`run_queue`, the host's noise feed, 16-step chunks, graph replay): four calls on the engine
    the first one built, `part_ml` filled with 3.0e38 before the fourth. Tokens, log-probabilities and the last step's logits."""
    args, m, utts = _two_utterances()
    kw = dict(top_k=40, top_p=0.8, temperature=1, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, aug_text=True, seed=11, return_logprobs=True)
    before = m.debug_logits
    m.debug_logits = True
    try:
        runs, engines = [], []
        for i in range(4):
            if i == 3:
                engines[0].part_ml.fill_(3.0e38)
            res = m.inference_batch(utts, **kw)
            eng = next(iter(m._engines.values()))
            engines.append(eng)
            torch.cuda.synchronize()
            runs.append(tuple(r[0].cpu().numpy() for r in res) + tuple(r[4].steps for r in res) + (eng.dbg_logits.cpu().numpy(),))
        assert all(e is engines[0] for e in engines) and engines[0].B == 4
        for u, ut in enumerate(utts):                                     # each utterance generated into the second page of its cache
            assert ut["x"].shape[1] + ut["y"].shape[1] + runs[0][2 + u].shape[0] > _lib.PAGE
    finally:
        m.debug_logits = before
    _assert_same_bits(runs, ("res0", "res1", "logprobs0", "logprobs1", "last logits"))


# ---------------------------------------------------------------------------------------------------------------- the samples
def test_sample_scores_rank_the_samples_of_one_utterance(tmp_path):
    from test_gpu_stream_batch import FakePhonemizer, PHN2NUM, _pipeline
    args, m, tok = _pipeline()
    margs = argparse.Namespace(**vars(args))
    fn = str(tmp_path / "prompt.wav")
    write_wav(fn, torch.randn(1, 20 * 320 - 7, generator=torch.Generator().manual_seed(1)) * 0.2, 16000)
    dc = {"top_k": 40, "top_p": 0.8, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    call = (m, margs, PHN2NUM, FakePhonemizer(), tok, fn, "hello world", "hello world again", torch.LongTensor([[20, 20]]), 1.5, 2, True, False,
            False, True, "cuda", dc)
    seeds = [11, 12]
    # every decode below reuses the engine of the one before it where the shapes allow: a decode's bits do not depend on what its engine
    # decoded before (DESIGN.md Part I.27; the tests above hold the engine to that)
    plain = S.inference_samples(*call, seeds=seeds)
    waves, scores = S.inference_samples(*call, seeds=seeds, return_scores=True)
    assert len(waves) == len(plain) == len(scores) == 2
    for w, p in zip(waves, plain):
        assert w.shape == p.shape and torch.equal(w.view(torch.int32), p.view(torch.int32))
    y, _ = S._prompt_codes(tok, fn, 4)
    one = {"x": S._phoneme_ids(FakePhonemizer(), PHN2NUM, "hello world again"), "y": y, "mask_interval": torch.LongTensor([[[20, 20]]])}
    res = m.inference_batch([one] * 2, top_k=40, top_p=0.8, temperature=1, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, aug_text=True,
                            seed=11, return_logprobs=True)
    for i, (sc, r) in enumerate(zip(scores, res)):
        assert set(sc) == {"seed", "mean_logprob", "total_logprob", "count", "frames"}
        assert sc["seed"] == seeds[i] and sc["count"] == r[4].count > 0 and sc["frames"] == int(r[1].sum()) > 0
        assert sc["mean_logprob"] == r[4].mean and sc["total_logprob"] == r[4].total and sc["mean_logprob"] < 0
        assert sc["mean_logprob"] == sc["total_logprob"] / sc["count"]
    assert scores[0]["mean_logprob"] != scores[1]["mean_logprob"]                          # two seeds, two draws
