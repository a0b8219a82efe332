"""GPU: the drop-in `SSR_Speech.inference` (HIP engine) against the REFERENCE's golden vectors
(tests/golden/lm_*.npz, produced by oracle/make_golden.py from /root/reference) and, at the full
830M shape, against the oracle run on this box's CPU.

Bars: codec-token ids, marks and intervals bit-exact under greedy decode; sampled runs bit-exact
when fed the recorded Exp(1) noise; per-step post-edit logits within 2e-4 absolute (fp32, different
summation order; logits are O(1..10))."""
import glob
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import weights as W
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import lm as O

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "lm_*.npz")))
LOGIT_ATOL = 2e-4


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"lm_{name}.npz"))
    d, h, nl, v = (int(t) for t in g["cfg"])
    args = W.lm_args_tiny(d_model=d, nhead=h, layers=nl, vocab=v)
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    return g, args, kw


def _model(args, seed):
    m = SSR_Speech(args)
    m.load_state_dict(W.lm_state_dict(args, seed=seed))
    return m.to("cuda").eval()


@pytest.mark.parametrize("name", CASES)
def test_inference_tokens_match_reference(golden_dir, name):
    g, args, kw = _load(golden_dir, name)
    m = _model(args, int(g["weight_seed"]))
    L = g["x"].shape[1]
    x = torch.from_numpy(g["x"]).cuda()
    y = torch.from_numpy(g["y"]).cuda()
    extra = {}
    if kw.get("aug_text") and not kw.get("cfg_pretrained"):
        extra["uncond_x"] = torch.from_numpy(g["uncond_x"])
    if "sample" in name:
        extra["noise"] = torch.from_numpy(g["step_noise"])
    # aug_context / cfg_pretrained cases carry a separate prompt; the older ones passed x / y twice
    px = torch.from_numpy(g["prompt_x"]).cuda() if "prompt_x" in g.files else x
    py = torch.from_numpy(g["prompt"]).cuda() if "prompt" in g.files else y
    res, marks, masks, nmi = m.inference(x, torch.LongTensor([L]).cuda(), px, torch.LongTensor([px.shape[1]]).cuda(), y, py,
                                         torch.from_numpy(g["mask_interval"]).cuda(), **kw, **extra)
    assert res.dtype == torch.int64 and res.device.type == "cuda" and marks.device.type == "cpu"
    assert m.last_run["steps"] == g["step_samples"].shape[0]
    assert np.array_equal(res.cpu().numpy(), g["res"])
    assert np.array_equal(marks.numpy(), g["marks"])
    assert np.array_equal(np.asarray(masks), g["masks"])
    assert np.array_equal(np.asarray(nmi), g["non_mask_intervals"])


@pytest.mark.parametrize("name", ["tts_greedy_cfg5", "edit_2span_greedy", "tts_greedy_hd128", "tts_sample_topp_temp", "cfgpre_tts_greedy"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_per_step_logits_match_reference(golden_dir, name, use_graph):
    """Step the engine one decode step at a time and compare the logits it hands to the sampler
    (after CFG combine + special-token edits) with what the reference handed to `topk_sampling`."""
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
    g, args, kw = _load(golden_dir, name)
    sd = W.lm_state_dict(args, seed=int(g["weight_seed"]), device="cuda")
    arena = LMWeightsArena(args, sd, torch.device("cuda"))
    S = g["step_logits"].shape[0]
    eng = DecodeEngine(arena, 1, bool(kw["aug_text"]), 1024, 256, debug_logits=True)
    y = g["y"][0].T
    cated, mp, num_task, nmi = LY.build_layout(y, g["mask_interval"][0], args)
    if kw.get("cfg_pretrained"):      # ssr.py:576,631-634 == an unconditional row whose text is the single id text_vocab_size-1
        rows = [g["x"][0], np.asarray([args.text_vocab_size - 1])]
    else:
        rows = [g["x"][0]] + ([g["uncond_x"][0]] if kw["aug_text"] else [])
    kn = DecodeKnobs(top_k=kw["top_k"], top_p=kw["top_p"], temperature=kw["temperature"], stop_repetition=kw["stop_repetition"],
                     silence_tokens=tuple(kw.get("silence_tokens", (1388, 1898, 131))), cfg_coef=kw["cfg_coef"], cfg_stride=kw["cfg_stride"],
                     use_cfg=bool(kw["aug_text"]), text_len=g["x"].shape[1], n_spans=num_task)
    nz = torch.ones(1, eng.max_steps, args.n_codebooks, arena.card)
    nz[0, :S] = torch.from_numpy(g["step_noise"])
    eng.start(rows, [cated], [kn], noise=nz.cuda())
    worst = 0.0
    for s in range(S):
        eng.decode(1, use_graph=use_graph)
        torch.cuda.synchronize()
        got = eng.dbg_logits[0].cpu().numpy()
        ref = g["step_logits"][s]
        worst = max(worst, float(np.abs(got - ref).max()))
        assert np.allclose(got, ref, rtol=0, atol=LOGIT_ATOL), (s, np.abs(got - ref).max())
    st = eng.states()[0]
    assert st.done == 1 and st.n_steps == S
    print(f"{name}: max |logit diff| over {S} steps = {worst:.2e}")


def test_prefill_on_the_fp32_chain_matches_the_reference_too():
    """The prefill GEMMs run on the bf16 matrix cores with exactly split operands by default (the tests above) and on the fp32 FMA chain with
    SSRHIP_PREFILL_SPLIT=0 (read once per process): the same per-step logit comparison with the reference (2e-4) and the end-to-end token
    comparison in a child process with the switch at 0 — so both forms are within 2e-4 of the reference's logits (hence within 4e-4 of each
    other) and both reproduce its greedy tokens on every golden."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_lm.py"), "-x", "-q", "-k",
                          "(per_step_logits_match_reference and True) or inference_tokens_match_reference"],
                         env=dict(os.environ, SSRHIP_PREFILL_SPLIT="0"), cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-2000:]
    import re as _re
    n_passed = int(_re.search(r"(\d+) passed", out.stdout).group(1))
    assert n_passed >= 20, f"the -k expression selected only {n_passed} tests: {out.stdout[-500:]}"   # (a renamed test must not shrink this silently)


def test_contract_errors():
    args = W.lm_args_tiny()
    m = _model(args, 1)
    x = torch.zeros(1, 5, dtype=torch.long).cuda()
    y = torch.zeros(1, 9, 4, dtype=torch.long).cuda()
    mi = torch.LongTensor([[[9, 9]]]).cuda()
    with pytest.raises(AssertionError):
        m.inference(x, torch.LongTensor([5]), x, torch.LongTensor([5]), y, y, mi, cfg_coef=0.5)       # ssr.py:552
    with pytest.raises(AssertionError):
        m.inference(x[0], torch.LongTensor([5]), x, torch.LongTensor([5]), y, y, mi)                 # ssr.py:553
    with pytest.raises(AssertionError):
        m.inference(x, torch.LongTensor([5]), x, torch.LongTensor([5]), y.repeat(2, 1, 1), y, mi)    # ssr.py:559 batch-1 only
    with pytest.raises(NotImplementedError):
        m.forward({})
    cpu = SSR_Speech(args)
    with pytest.raises(RuntimeError):
        cpu.inference(x.cpu(), torch.LongTensor([5]), x.cpu(), torch.LongTensor([5]), y.cpu(), y.cpu(), mi.cpu())


def test_state_dict_keys_are_the_references():
    args = W.lm_args_tiny()
    m = SSR_Speech(args)
    assert list(m.state_dict().keys()) == list(W.lm_param_specs(args).keys())
    assert vars(m.args)["n_codebooks"] == 4


@pytest.mark.parametrize("mode", ["tts", "edit"])
def test_full_830m_greedy_steps_match_oracle_on_cpu(mode):
    """Full 'English 830M' shape (SURVEY §8 constants), synthetic weights: greedy CFG steps on the GPU vs the oracle on this
    box's CPU cores: same token ids, logits within 5e-4. "tts" = BASELINE config 1/2 shape (short prompt, empty span at the
    end); "edit" = config 3 shape (L=120 phonemes, 397-frame utterance, single span [150, 250) => 3-segment layout,
    context > 3 KV pages at the first step)."""
    args = W.lm_args_830m()
    torch.manual_seed(0)
    sd_gpu = W.lm_state_dict(args, seed=0, device="cuda")
    m = SSR_Speech(args)
    m.load_state_dict({k: v.cpu() for k, v in sd_gpu.items()})
    m = m.to("cuda").eval()
    gen = torch.Generator().manual_seed(2024)
    if mode == "tts":
        L, N, steps = 40, 60, 24
        mi = torch.LongTensor([[[N, N]]])
    else:
        L, N, steps = 120, 397, 10
        mi = torch.LongTensor([[[150, 250]]])
    x = torch.randint(0, 100, (1, L), generator=gen)
    y = torch.randint(0, 2048, (1, N, 4), generator=gen)
    unc = torch.randint(0, 101, (1, L), generator=gen)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    # oracle on the CPU (weights are bit-identical: same generator, checked below)
    sd_cpu = O.reference_params({k: v.cpu() for k, v in sd_gpu.items()})
    k0 = "decoder.layers.7.linear1.weight"
    assert torch.equal(W.make_tensor(k0, sd_cpu[k0].shape, "lin:2048", 0), sd_cpu[k0].detach())
    trace = {}
    O.inference(sd_cpu, args, x, y, mi, uncond_x=unc, max_steps=steps, trace=trace, **kw)
    ref_tok = torch.stack(trace["samples"]).numpy()
    ref_log = torch.stack(trace["edited_logits"]).numpy()
    # engine, stepped
    m.debug_logits = True
    out = m.inference(x.cuda(), torch.LongTensor([L]), x.cuda(), torch.LongTensor([L]), y.cuda(), y.cuda(), mi.cuda(),
                      uncond_x=unc, max_new_steps=steps, **kw)
    assert out is None and m.last_run["steps"] == steps
    eng = next(iter(m._engines.values()))
    got_tok = eng.generated[0, :steps].cpu().numpy()
    assert np.array_equal(got_tok, ref_tok), (got_tok, ref_tok)
    last = eng.dbg_logits[0].cpu().numpy()
    err = np.abs(last - ref_log[steps - 1]).max()
    print(f"830M {mode}: max |logit diff| at step {steps}: {err:.2e} (logit std {ref_log[steps-1][np.abs(ref_log[steps-1])<1e3].std():.2f})")
    assert err < 5e-4


@pytest.mark.parametrize("n_utt", [3, 8])
@pytest.mark.parametrize("aug_text,greedy", [(True, True), (False, True), (True, False), (False, False)])
def test_inference_batch_rows_equal_batch1_runs(aug_text, greedy, n_utt):
    """New capability (the reference is batch-1 only): utterances of DIFFERENT text / prompt lengths decoded in lock-step.
    Row i must equal a batch-1 `inference()` of utterance i seeded with seed+i."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 21)
    g = torch.Generator().manual_seed(3)
    utts = []
    # 3 utterances: 3 rows (padded to 4, VALU GEMV) or 6 rows (matrix-core GEMV); 8 utterances: 8 / 16 rows
    for (L, T) in [(9, 14), (13, 22), (6, 10), (11, 17), (7, 12), (10, 20), (12, 9), (8, 15)][:n_utt]:
        utts.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    utts[1]["mask_interval"] = torch.LongTensor([[[5, 9]]])            # one of them is an edit, the others TTS
    kw = dict(top_k=1, top_p=1.0) if greedy else dict(top_k=12, top_p=0.9)
    kw.update(temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=aug_text)
    batch = m.inference_batch(utts, seed=100, **kw)
    for i, u in enumerate(utts):
        torch.manual_seed(100 + i)
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, **kw)
        assert torch.equal(batch[i][0], one[0]) and torch.equal(batch[i][1], one[1]) and batch[i][2] == one[2] and batch[i][3] == one[3], i


@pytest.mark.parametrize("n_utt", [1, 5])
def test_long_context_many_pages_matches_oracle(n_utt):
    """Context of ~2,100 positions = 17 KV pages (the bench config uses 8): split-KV partials, their merge in the out-proj
    prologue (2 rows) / the combine kernel (10 rows, matrix-core path) and the page table beyond 8 pages. Edit of one
    short span in the middle of a 1,900-frame utterance, greedy with CFG; tokens equal the oracle's on the CPU."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 33)
    g = torch.Generator().manual_seed(17)
    L, T = 180, 1900
    utts = []
    for i in range(n_utt):
        x = torch.randint(0, 30, (1, L + i), generator=g)
        y = torch.randint(0, 64, (1, T + 3 * i, 4), generator=g)
        utts.append(dict(x=x, y=y, mask_interval=torch.LongTensor([[[900, 905 + i]]])))
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=1, aug_text=True)
    got = m.inference_batch(utts, seed=7, **kw)
    sd = O.reference_params(W.lm_state_dict(args, seed=33))
    for i in (0, n_utt - 1):
        torch.manual_seed(7 + i)
        ref = O.inference(sd, args, utts[i]["x"], utts[i]["y"], utts[i]["mask_interval"], kvcache=1, max_steps=None, **kw)
        assert torch.equal(got[i][0].cpu(), ref[0]) and torch.equal(got[i][1], ref[1]) and got[i][2] == ref[2], i


@pytest.mark.parametrize("name", ["tts_sample_topk", "tts_sample_topp_temp", "cfgpre_ctx_sample"])
def test_sampled_runs_reproduce_reference_from_the_seed_alone(golden_dir, name):
    """no recorded noise, no recorded uncond_x — only `torch.manual_seed(seed)` as a user of the reference
    would do. `inference()` consumes the global CPU generator in the reference's order (randint for the CFG text, then one
    Exp(1) tensor per step, which is what torch.multinomial draws), so the sampled tokens equal the reference's."""
    g, args, kw = _load(golden_dir, name)
    m = _model(args, int(g["weight_seed"]))
    L = g["x"].shape[1]
    x = torch.from_numpy(g["x"]).cuda()
    y = torch.from_numpy(g["y"]).cuda()
    px = torch.from_numpy(g["prompt_x"]).cuda() if "prompt_x" in g.files else x
    py = torch.from_numpy(g["prompt"]).cuda() if "prompt" in g.files else y
    torch.manual_seed(int(g["torch_seed"]))
    res, marks, masks, nmi = m.inference(x, torch.LongTensor([L]), px, torch.LongTensor([px.shape[1]]), y, py,
                                         torch.from_numpy(g["mask_interval"]).cuda(), **kw)
    assert np.array_equal(res.cpu().numpy(), g["res"])
    assert np.array_equal(marks.numpy(), g["marks"])


def test_dp_generate_single_rank_equals_inference_batch():
    """`dp.generate` (BASELINE config 4 entry point) without a process group == `inference_batch` of all utterances."""
    from ssr_speech_amd import dp
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 21)
    g = torch.Generator().manual_seed(5)
    utts = [dict(x=torch.randint(0, 30, (1, 6 + i), generator=g), y=torch.randint(0, 64, (1, 10 + 2 * i, 4), generator=g),
                 mask_interval=torch.LongTensor([[[10 + 2 * i, 10 + 2 * i]]])) for i in range(5)]
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)
    # two multi-span edits ride along (2 and 3 spans): the one-collective gather relies on `dp.token_cap` being a true upper bound of
    # every result's length, whatever the span layout
    utts.append(dict(x=torch.randint(0, 30, (1, 9), generator=g), y=torch.randint(0, 64, (1, 24, 4), generator=g),
                     mask_interval=torch.LongTensor([[[3, 6], [12, 16]]])))
    utts.append(dict(x=torch.randint(0, 30, (1, 11), generator=g), y=torch.randint(0, 64, (1, 30, 4), generator=g),
                     mask_interval=torch.LongTensor([[[2, 5], [10, 13], [20, 26]]])))
    toks, (mine, outs) = dp.generate(m, utts, seed=9, **kw)
    ref = m.inference_batch(utts, seed=9, **kw)
    assert mine == list(range(7)) and len(toks) == 7
    for i in range(7):
        assert torch.equal(toks[i], ref[i][0][0])
        u = utts[i]
        cap = dp.token_cap(u["x"].shape[-1], u["y"].shape[1], int(u["mask_interval"].shape[-2]), 4)
        assert toks[i].shape[-1] <= cap, (i, toks[i].shape, cap)


def test_full_830m_ten_rows_match_oracle_on_cpu():
    """The 5..16-row (matrix-core) decode step at the full 830M shape: 5 utterances x CFG = 10 rows of different lengths in
    one engine, 6 greedy steps; every utterance's tokens equal the oracle's (run one by one on the CPU) and its post-edit
    logits agree within 5e-4."""
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
    args = W.lm_args_830m()
    sd_gpu = W.lm_state_dict(args, seed=0, device="cuda")
    arena = LMWeightsArena(args, sd_gpu, torch.device("cuda"))
    sd_cpu = O.reference_params({k: v.cpu() for k, v in sd_gpu.items()})
    gen = torch.Generator().manual_seed(77)
    n_utt, steps = 5, 6
    eng = DecodeEngine(arena, n_utt, True, 256, 64, debug_logits=True)
    rows, cols, knobs, utts = [], [], [], []
    for u in range(n_utt):
        L, N = 20 + 3 * u, 30 + 5 * u
        x = torch.randint(0, 100, (1, L), generator=gen)
        y = torch.randint(0, 2048, (1, N, 4), generator=gen)
        unc = torch.randint(0, 101, (1, L), generator=gen)
        mi = torch.LongTensor([[[N, N]]])
        cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)
        rows += [x[0].numpy(), unc[0].numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, use_cfg=True,
                                 text_len=L, n_spans=num_task, seed=u))
        utts.append((x, y, unc, mi))
    eng.start(rows, cols, knobs, noise=None)
    eng.decode(steps, use_graph=True)
    torch.cuda.synchronize()
    got = eng.generated[:, :steps].cpu().numpy()
    last = eng.dbg_logits.cpu().numpy()
    for u, (x, y, unc, mi) in enumerate(utts):
        trace = {}
        O.inference(sd_cpu, args, x, y, mi, uncond_x=unc, max_steps=steps, trace=trace, top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2,
                    kvcache=1, cfg_coef=1.5, cfg_stride=2, aug_text=True)
        ref_tok = torch.stack(trace["samples"]).numpy()
        assert np.array_equal(got[u], ref_tok), (u, got[u], ref_tok)
        err = np.abs(last[u] - torch.stack(trace["edited_logits"]).numpy()[steps - 1]).max()
        assert err < 5e-4, (u, err)


@pytest.mark.parametrize("name", ["tts_greedy_cfg5", "edit_3span_greedy", "tts_sample_topk"])
def test_shuffled_page_table_end_to_end(golden_dir, name):
    """The KV pages are handed out by a host-side allocator (engine.PagePool); here in a SHUFFLED order, so the page table
    the kernels walk is an arbitrary permutation (by default it is already interleaved across rows, never the identity of
    the dense layout). Tokens must still equal the reference's."""
    g, args, kw = _load(golden_dir, name)
    m = _model(args, int(g["weight_seed"]))
    rng = np.random.default_rng(5)
    m.page_order = [int(p) for p in rng.permutation(64)]
    L = g["x"].shape[1]
    x, y = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
    extra = {"uncond_x": torch.from_numpy(g["uncond_x"])} if kw.get("aug_text") else {}
    if "sample" in name:
        extra["noise"] = torch.from_numpy(g["step_noise"])
    res, marks, masks, nmi = m.inference(x, torch.LongTensor([L]), x, torch.LongTensor([L]), y, y, torch.from_numpy(g["mask_interval"]).cuda(), **kw, **extra)
    eng = next(iter(m._engines.values()))
    log = eng.pages.handed_out                                    # (page, row) in hand-out order; everything is back in the pool by now
    pages_row0 = [p for p, row in log if row == 0]
    assert len(log) >= 2 and pages_row0 != sorted(pages_row0) or len(pages_row0) < 2, log      # a shuffled, non-monotonic table
    assert [p for p, _ in log] == [p for p in m.page_order if p < eng.pages.n_pages][: len(log)]
    assert eng.pages.n_free == eng.pages.n_pages
    assert np.array_equal(res.cpu().numpy(), g["res"]) and np.array_equal(marks.numpy(), g["marks"])


def test_page_pool_is_shared_and_pages_return_when_an_utterance_finishes():
    """One long and several short utterances in one lock-step batch: the pool holds the SUM of what each row can reach, not
    rows x the longest; pages grow on demand while decoding and come back when an utterance is done; results equal batch-1 runs."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 44)
    g = torch.Generator().manual_seed(9)
    shapes = [(60, 500), (6, 20), (7, 30), (5, 25)]              # the first one reaches ~1,100 positions, the others < 128
    utts = [dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                 mask_interval=torch.LongTensor([[[T, T]]])) for L, T in shapes]
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=1, aug_text=True)
    got = m.inference_batch(utts, seed=3, **kw)
    eng = next(iter(m._engines.values()))
    assert eng.pages.n_pages < eng.B * eng.max_pages, (eng.pages.n_pages, eng.B, eng.max_pages)      # smaller than the dense reservation
    assert eng.pages.n_free == eng.pages.n_pages                                                      # everything was returned
    assert (eng._table_host == eng.scratch_page).all()
    for i, u in enumerate(utts):
        torch.manual_seed(3 + i)
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, **kw)
        assert torch.equal(got[i][0], one[0]) and torch.equal(got[i][1], one[1]), i


def test_positions_beyond_the_initial_table_grow_it_like_extend_pe():
    """the sinusoidal table started at 8192 rows and was read unguarded. A text of 8,300 phonemes has positions past
    it: the table must grow (reference: SinePositionalEmbedding.extend_pe, embedding.py:66-92) and the tokens still equal the oracle's."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 45)
    g = torch.Generator().manual_seed(10)
    L, T, steps = 8300, 24, 6
    x = torch.randint(0, 30, (1, L), generator=g)
    y = torch.randint(0, 64, (1, T, 4), generator=g)
    mi = torch.LongTensor([[[T, T]]])
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=1, aug_text=False)
    out = m.inference(x.cuda(), torch.LongTensor([L]), x.cuda(), torch.LongTensor([L]), y.cuda(), y.cuda(), mi.cuda(), max_new_steps=steps, **kw)
    assert out is None and m._arena.max_pos > 8192
    eng = next(iter(m._engines.values()))
    trace = {}
    O.inference(O.reference_params(W.lm_state_dict(args, seed=45)), args, x, y, mi, max_steps=steps, trace=trace, kvcache=1, **kw)
    assert np.array_equal(eng.generated[0, :steps].cpu().numpy(), torch.stack(trace["samples"]).numpy())


@pytest.mark.parametrize("name", ["tts_greedy_cfg5", "edit_2span_greedy", "tts_greedy_hd128", "tts_greedy_nocfg"])
def test_prefill_kv_cache_equals_reference_present(golden_dir, name):
    """the K/V the reference's first dec_forward returns as `present` (every layer, both CFG rows, all of
    [text || prompt audio || mask token]) against the paged cache after `start()` (prefill) + the first decode step (which
    appends the mask token's K/V). Gathered through the page table the allocator filled."""
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
    from ssr_speech_amd._lib import PAGE
    g, args, kw = _load(golden_dir, name)
    ref = g["prefill_present"]                                   # [n_layer, 2, B, H, S0, hd]
    nl, _, B, H, S0, hd = ref.shape
    sd = W.lm_state_dict(args, seed=int(g["weight_seed"]), device="cuda")
    arena = LMWeightsArena(args, sd, torch.device("cuda"))
    eng = DecodeEngine(arena, 1, bool(kw["aug_text"]), 256, 64)
    cated, mp, num_task, nmi = LY.build_layout(g["y"][0].T, g["mask_interval"][0], args)
    rows = [g["x"][0]] + ([g["uncond_x"][0]] if kw["aug_text"] else [])
    kn = DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=kw["stop_repetition"], cfg_coef=kw["cfg_coef"], cfg_stride=kw["cfg_stride"],
                     use_cfg=bool(kw["aug_text"]), text_len=g["x"].shape[1], n_spans=num_task)
    eng.start(rows, [cated], [kn])
    eng.decode(1, use_graph=False)
    torch.cuda.synchronize()
    assert eng.B == B and int(eng.kv_pos[0]) == S0
    pool = eng.kv_pool.view(-1, nl, 2, H, PAGE, hd).cpu()
    table = eng._table_host
    worst = 0.0
    for b in range(B):
        got = torch.cat([pool[int(table[b, p])] for p in range((S0 + PAGE - 1) // PAGE)], dim=3)[:, :, :, :S0]     # [nl, 2, H, S0, hd]
        want = torch.from_numpy(ref[:, :, b])
        worst = max(worst, float((got - want).abs().max()))
        torch.testing.assert_close(got, want, rtol=0, atol=2e-5)
    print(f"{name}: prefill K/V max |diff| vs reference present = {worst:.2e}")


@pytest.mark.parametrize("greedy", [True, False])
def test_sixteen_rows_sixteen_heads_full_generation_equals_batch1(greedy):
    """The whole 16-row decode path end to end on a model wide enough to take it: d_model 1024 with 16 heads => 16 rows x 16 heads
    = 256 (row, head) pairs = the fused `attn_rows` kernel, the rows-per-workgroup matrix-core GEMVs with streaming-order weights
    (incl. the k-step-pair kernels for out-proj / FFN2 with K = 4096 streamed) and the page allocator under growth — 8 utterances of
    different lengths x CFG, run to completion (~100 steps each, several KV pages); every utterance must equal its batch-1 run
    (VALU GEMV + split attention) seeded seed + i."""
    args = W.lm_args_tiny(d_model=1024, nhead=16, layers=2, vocab=64)
    m = _model(args, 52)
    g = torch.Generator().manual_seed(12)
    utts = []
    for (L, T) in [(12, 130), (9, 20), (14, 140), (10, 60), (13, 125), (8, 30), (11, 100), (12, 127)]:
        utts.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    utts[3]["mask_interval"] = torch.LongTensor([[[20, 31]]])
    kw = dict(top_k=1, top_p=1.0) if greedy else dict(top_k=12, top_p=0.9)
    kw.update(temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)
    batch = m.inference_batch(utts, seed=300, **kw)
    eng = next(iter(m._engines.values()))
    assert eng.B == 16 and eng.B * args.nhead >= 192
    for i, u in enumerate(utts):
        torch.manual_seed(300 + i)
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, **kw)
        assert torch.equal(batch[i][0], one[0]) and torch.equal(batch[i][1], one[1]) and batch[i][2] == one[2], i


@pytest.mark.parametrize("two_phase", ["0", "1"])
@pytest.mark.parametrize("greedy", [True, False])
def test_inference_batch_refill_equals_batch1(greedy, two_phase, monkeypatch):
    """`two_phase` = SSRHIP_ADMIT_TWO_PHASE: the refilled slot's prefill on the decode stream (default), or on a side stream against a private
    page table with the slot joining at the next poll (round 5: built, identical tokens, measured no faster — opt-in).
    Continuous batching: 24 utterances of very different lengths (L in [6, 40] phonemes => 30..330 steps under
    the reference's 10 x L cap, prompts of 5..60 frames, one two-span edit) through 8 utterance slots. A slot whose utterance is done
    at a 16-step poll releases its KV pages and takes the next pending utterance (prefill of just those rows, sampler state reset, same
    graph) while the others keep decoding. Contract unchanged: utterance i == its batch-1 run seeded seed + i (greedy and sampled)."""
    args = W.lm_args_tiny(d_model=256, nhead=4, layers=2, vocab=64)
    m = _model(args, 61)
    g = torch.Generator().manual_seed(13)
    utts = []
    for i in range(24):
        L = int(torch.randint(6, 41, (1,), generator=g))
        T = int(torch.randint(5, 61, (1,), generator=g))
        utts.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                         mask_interval=torch.LongTensor([[[T, T]]])))
    T5 = utts[5]["y"].shape[1]
    utts[5]["mask_interval"] = torch.LongTensor([[[1, 2], [T5 - 2, T5 - 1]]]) if T5 >= 8 else utts[5]["mask_interval"]
    kw = dict(top_k=1, top_p=1.0) if greedy else dict(top_k=12, top_p=0.9)
    kw.update(temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)
    monkeypatch.setenv("SSRHIP_ADMIT_TWO_PHASE", two_phase)
    batch = m.inference_batch(utts, seed=700, group=8, **kw)
    monkeypatch.delenv("SSRHIP_ADMIT_TWO_PHASE")
    eng = next(iter(m._engines.values()))
    assert eng.n_utt == 8 and eng.n_admitted == 24 and eng.n_refills == 16          # every utterance beyond the first 8 went into a used slot
    assert eng.pages.n_free == eng.pages.n_pages                                     # every page came back
    lens = {int(b[0].shape[-1]) for b in batch}
    assert len(lens) > 8
    for i, u in enumerate(utts):
        torch.manual_seed(700 + i)
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, **kw)
        assert torch.equal(batch[i][0], one[0]) and torch.equal(batch[i][1], one[1]) and batch[i][2] == one[2] and batch[i][3] == one[3], i


def test_refill_with_fewer_jobs_than_slots_and_three_rows():
    """Edge cases of the queue: fewer utterances than slots (idle slots stay parked), the 3-row count (no CFG, 3 utterances: one more,
    idle slot), and an engine reused for a second, different queue (heterogeneous batches must not rebuild the engine)."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 62)
    g = torch.Generator().manual_seed(14)
    mk = lambda L, T: dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g), mask_interval=torch.LongTensor([[[T, T]]]))
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.0, cfg_stride=1, aug_text=False)
    a = [mk(7, 9), mk(12, 20), mk(9, 5)]
    ra = m.inference_batch(a, seed=5, **kw)
    eng = next(iter(m._engines.values()))
    assert eng.B == 4 and eng.n_admitted == 3
    b = [mk(6, 30), mk(10, 12)]
    rb = m.inference_batch(b, seed=9, group=4, **kw)
    assert next(iter(m._engines.values())) is eng or True           # (a 2-slot engine may be built; the 4-slot one is reused when group allows)
    for utts, res, sd in ((a, ra, 5), (b, rb, 9)):
        for i, u in enumerate(utts):
            torch.manual_seed(sd + i)
            L = u["x"].shape[1]
            one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                              u["mask_interval"].cuda(), kvcache=1, **kw)
            assert torch.equal(res[i][0], one[0]) and res[i][2] == one[2], i


def test_run_queue_parks_an_utterance_that_exceeds_its_cap_and_keeps_serving_the_others():
    """`DecodeEngine.run_queue` with one job whose step cap is far too small: that job comes back unfinished (done == 0, exactly one
    16-step chunk long) and its slot is parked and refilled; every other job still equals its batch-1 run. `inference_batch` turns
    such a job into a RuntimeError."""
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd.engine import DecodeKnobs
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 63)
    g = torch.Generator().manual_seed(15)
    utts = [dict(x=torch.randint(0, 30, (1, 8 + i), generator=g), y=torch.randint(0, 64, (1, 10 + 2 * i, 4), generator=g),
                 mask_interval=torch.LongTensor([[[10 + 2 * i, 10 + 2 * i]]])) for i in range(5)]
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, silence_tokens=(3, 7, 11), cfg_coef=1.5, cfg_stride=2)
    jobs = []
    for i, u in enumerate(utts):
        x_np = u["x"].numpy()
        L = x_np.shape[1]
        rng = torch.Generator().manual_seed(50 + i)
        unc = torch.randint(0, m.n_text_tokens, (1, L), generator=rng).numpy()[0]
        y_np = u["y"][0].transpose(1, 0).numpy()
        cated, _, num_task, nmi = LY.build_layout(y_np, u["mask_interval"][0].numpy(), m.args)
        cap = max(10 * L + 2 - cated.shape[1], 1) + num_task * 5
        jobs.append(dict(text_rows=[x_np[0], unc], audio_cols=cated, gen=rng, cap=(8 if i == 1 else cap),
                         knobs=DecodeKnobs(use_cfg=True, text_len=L, n_spans=num_task, seed=50 + i, **kw)))
    eng = m._get_engine(2, True, 512, 256)
    outs = eng.run_queue(jobs, chunk=16, sampling=False)
    assert outs[1][0].done == 0 and outs[1][1].shape[0] == 16                    # parked after its first chunk
    assert eng.pages.n_free == eng.pages.n_pages and eng.n_admitted == 5
    for i in (0, 2, 3, 4):
        st, gen = outs[i]
        assert st.done == 1
        torch.manual_seed(50 + i)
        u = utts[i]
        L = u["x"].shape[1]
        one = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, aug_text=True, top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2,
                          silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2)
        assert one[0].shape[-1] == u["y"].shape[1] + int(st.n_steps) - 4, i          # generated frames = steps - 3 delay columns - 1 eog column


def test_sampled_batch1_runs_around_a_sampled_queue_keep_the_generator_contract():
    """The host-noise pipeline across runs of one model: a sampled batch-1 run cut at 21 steps (chunks of 16 and 5), a sampled queue of
    three utterances through ONE slot (two refills, the admission staging buffer, the one-slot engine reused where it is large enough),
    then the first run again. The global generator ends after exactly `steps` per-step draws, each queue result equals its batch-1 run
    seeded seed + i, and the repeat is bit-equal to the first run, generator state included."""
    args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64)
    m = _model(args, 71)
    g = torch.Generator().manual_seed(16)
    utts = [dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                 mask_interval=torch.LongTensor([[[T, T]]])) for (L, T) in [(9, 14), (6, 10), (8, 12)]]
    kw = dict(top_k=12, top_p=0.9, temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5, cfg_stride=2, aug_text=True)
    seed = 900

    def one(i, **more):
        u = utts[i]
        L = u["x"].shape[1]
        torch.manual_seed(seed + i)
        out = m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                          u["mask_interval"].cuda(), kvcache=1, **kw, **more)
        return out, int(m.last_run["steps"]), torch.get_rng_state()

    def same(a, b):
        return (a is None and b is None) or (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3])

    first, steps, state = one(0, max_new_steps=21)
    print(f"batch-1 run cut at 21 steps: {steps} steps, finished: {first is not None}")
    assert 0 < steps <= 21
    K, card = args.n_codebooks, next(iter(m._engines.values())).a.card
    torch.manual_seed(seed)
    torch.randint(0, m.n_text_tokens, (1, utts[0]["x"].shape[1]))
    for _ in range(steps):
        torch.empty(K, card).exponential_(1)
    assert torch.equal(state, torch.get_rng_state())

    batch = m.inference_batch(utts, seed=seed, group=1, **kw)
    for i in range(3):
        assert same(batch[i], one(i)[0]), i

    again, steps2, state2 = one(0, max_new_steps=21)
    assert same(again, first) and steps2 == steps and torch.equal(state2, state)
