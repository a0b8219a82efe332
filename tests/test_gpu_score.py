"""GPU: `SSR_Speech.score` — the reference's training-forward numbers (models/ssr.py:280-379) from the HIP layer loop, heads and
`ssrhip_xent_rank`:

  * every tests/golden/score_*.npz fixture (the reference's own forward): the dict within 1e-5 relative, per-position cross entropy
    within 5e-5, top-10 hits identical;
  * the 830M shape with seeded weights, three ragged items of ~300 audio rows, against the oracle's teacher-forced forward on the CPU;
  * the same on the fp32 FMA chain (SSRHIP_PREFILL_SPLIT=0, read once per process: a child process);
  * batching and chunking do not change an item's result; the kernel alone against fp64; scoring leaves `inference` untouched.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib, score as SC
from ssr_speech_amd import weights as W
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import lm as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "score_*.npz")))


def _fixture_args(g):
    d, h, layers, vocab = (int(v) for v in g["cfg"])
    args = W.lm_args_tiny(d_model=d, nhead=h, layers=layers, vocab=vocab)
    args.predict_mask_token = int(g["flag_predict_mask_token"])
    args.predict_all = int(g["flag_predict_all"])
    cw = str(g["flag_codebook_weight"])
    args.codebook_weight = cw if cw else None
    return args


def _model(args, seed, sd=None):
    m = SSR_Speech(args)
    m.load_state_dict(sd if sd is not None else W.lm_state_dict(args, seed=seed))
    return m.to("cuda").eval()


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-30)


def _check_dict(out, g):
    ref_loss = float(g["loss"])
    if np.isnan(ref_loss):
        assert torch.isnan(out["loss"]).item()
    else:
        assert _rel(out["loss"], ref_loss) <= 1e-5, (float(out["loss"]), ref_loss)
    for k, v in enumerate(out["top10acc_by_codebook"]):
        ref = float(g["top10acc_by_codebook"][k])
        assert (float(v) == 0.0) if ref == 0 else _rel(v, ref) <= 1e-5, (k, float(v), ref)
    assert _rel(out["top10acc"], g["top10acc"]) <= 1e-5
    assert out["effective_ntoken"].device.type == "cuda" and int(out["effective_ntoken"]) == int(g["effective_ntoken"])
    assert out["loss"].device.type == "cuda" and out["loss"].dtype == torch.float32


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_score_matches_the_reference_forward_on_the_fixtures(path):
    g = np.load(path)
    args = _fixture_args(g)
    m = _model(args, int(g["weight_seed"]))
    batch = {k: torch.from_numpy(g[k]) for k in ("x", "x_lens", "y", "y_lens")}
    out = m.score(batch)
    _check_dict(out, g)
    # per position: the fixture's CE / rank at the scored rows, in score's order (items in batch order, positions 0 .. y_len - 2)
    got_nll, got_rank = m.last_score["nll"].cpu().numpy(), m.last_score["rank"].cpu().numpy()
    ref_nll = np.concatenate([g["ce"][:, b, : int(g["y_lens"][b]) - 1] for b in range(len(g["y_lens"]))], 1)
    ref_rank = np.concatenate([g["rank"][:, b, : int(g["y_lens"][b]) - 1] for b in range(len(g["y_lens"]))], 1)
    assert got_nll.shape == ref_nll.shape
    err = np.abs(got_nll - ref_nll).max()
    assert err <= 5e-5, err
    flips = int(((got_rank < 10) != (ref_rank < 10)).sum())
    print(f"{os.path.basename(path)}: max |CE diff| {err:.2e}, top-10 hit flips {flips}, rank equal on "
          f"{float((got_rank == ref_rank).mean()) * 100:.1f}% of rows")
    assert flips == 0
    # the rescoring keys: per item the unweighted CE sum over the loss positions
    assert out["nll_by_item"].shape == (len(g["y_lens"]),) and int(out["ntoken_by_item"].sum()) > 0


def _items_830m(args, g, n=3):
    """Ragged items: text 40-70 ids, ~300 audio frames of random codes with the first span's mask token at a third of the way (so
    the loss positions are the two thirds after it) — x [L], y [K, T] int64."""
    K, V = args.n_codebooks, args.audio_vocab_size
    items = []
    for i in range(n):
        L = int(torch.randint(40, 70, (1,), generator=g))
        T = 280 + 17 * i
        y = torch.randint(0, V, (K, T), generator=g)
        y[:, T // 3] = args.mts
        y[:, 0] = args.sos
        items.append((torch.randint(0, args.text_vocab_size, (L,), generator=g), y))
    return items


def _collate(items, args):
    x = torch.nn.utils.rnn.pad_sequence([x for x, _ in items], batch_first=True, padding_value=args.text_pad_token)
    y = torch.nn.utils.rnn.pad_sequence([y.transpose(1, 0) for _, y in items], padding_value=args.audio_pad_token).permute(1, 2, 0)
    return dict(x=x, x_lens=torch.LongTensor([len(x) for x, _ in items]), y=y.contiguous(),
                y_lens=torch.LongTensor([y.shape[1] for _, y in items]))


def _oracle_item(sd, args, x, y):
    """The teacher-forced forward of ONE unpadded item on the CPU (oracle.lm restates models/ssr.py:214-278, :175-179) -> CE and rank
    [K, T-1] of y[:, 1:]."""
    K = args.n_codebooks
    L, T = x.shape[0], y.shape[1]
    pe = O.sine_pe(max(L, T) + 8, args.d_model)
    x_in = O.pos_embed(F.embedding(x[None], sd["text_embedding.word_embeddings.weight"]), sd["text_positional_embedding.alpha"], pe)
    y_in = O.pos_embed(O.embed_y(sd, y[:, :, None], K), sd["audio_positional_embedding.alpha"], pe)
    with torch.no_grad():
        y_out, _ = O.dec_forward(sd, args, x_in, L, torch.triu(torch.ones(L, L), diagonal=1).bool(), torch.zeros(1, L, dtype=torch.bool),
                                 y_in, T, torch.triu(torch.ones(T, T), diagonal=1).bool(), torch.zeros(1, T, dtype=torch.bool), None)
        lg = O.predict_heads(sd, args, y_out)[0][:, :-1]                         # [K, T-1, card]
    tg = y[:, 1:]
    ce = F.cross_entropy(lg.reshape(-1, lg.shape[-1]), tg.reshape(-1), reduction="none").reshape(tg.shape)
    rank = (lg > lg.gather(-1, tg.unsqueeze(-1))).sum(-1)
    return ce, rank.to(torch.int32)


def test_score_830m_matches_the_oracle_item_by_item():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    args = W.lm_args_830m()
    sd_gpu = W.lm_state_dict(args, seed=3, device="cuda")
    sd_cpu = O.reference_params({k: v.cpu() for k, v in sd_gpu.items()})
    m = _model(args, 3, sd={k: v.cpu() for k, v in sd_gpu.items()})
    del sd_gpu
    items = _items_830m(args, torch.Generator().manual_seed(3))
    batch = _collate(items, args)
    out = m.score(batch)
    got = m.last_score["nll"].cpu()
    ces, ranks = zip(*[_oracle_item(sd_cpu, args, x, y) for x, y in items])
    ref = torch.cat(ces, 1)
    err = float((got - ref).abs().max())
    # the oracle's dict from the same reducer fed the oracle's CE / rank
    work = [it for it in SC.validate(batch, args) if it.n_scored > 0]
    idx = SC.scored_index(work)
    tgt = torch.cat([y[:, 1:] for _, y in items], 1)
    ref_out = SC.reduce(ref, torch.cat(ranks, 1), tgt, torch.from_numpy(idx["item"]), torch.from_numpy(idx["pos"]), len(items), args)
    split = os.environ.get("SSRHIP_PREFILL_SPLIT", "1")[:1] != "0"
    print(f"830M ({'split bf16' if split else 'fp32 chain'}): {got.shape[1]} scored rows, max |CE diff| {err:.2e}, "
          f"loss {float(out['loss']):.6f} vs oracle {float(ref_out['loss']):.6f} (rel {_rel(out['loss'], ref_out['loss']):.2e})")
    assert err <= 5e-4, err
    assert _rel(out["loss"], ref_out["loss"]) <= 1e-4
    assert int(out["effective_ntoken"]) == int(ref_out["effective_ntoken"])


def test_score_on_the_fp32_chain_matches_too():
    """SSRHIP_PREFILL_SPLIT=0 (read once per process): the fixtures and the 830M comparison again, in a child process."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k", "fixtures or 830m_matches"],
                         env=dict(os.environ, SSRHIP_PREFILL_SPLIT="0"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    import re
    n = int(re.search(r"(\d+) passed", out.stdout).group(1))
    assert n == len(FIXTURES) + 1, out.stdout[-1500:]
    assert "fp32 chain" in out.stdout


def test_batched_and_chunked_equal_one_item_at_a_time():
    args = W.lm_args_tiny(d_model=256, nhead=2, layers=2, vocab=128)
    m = _model(args, 7)
    g = torch.Generator().manual_seed(7)
    items = []
    for i in range(6):
        L, T = int(torch.randint(3, 20, (1,), generator=g)), int(torch.randint(20, 90, (1,), generator=g))
        y = torch.randint(0, args.audio_vocab_size, (args.n_codebooks, T), generator=g)
        y[:, T // 4] = args.mts
        items.append((torch.randint(0, args.text_vocab_size, (L,), generator=g), y))
    whole = m.score(_collate(items, args))
    assert m.last_score["chunks"] == 1
    alone = torch.stack([m.score(_collate([it], args))["nll_by_item"][0] for it in items])
    rel = float(((whole["nll_by_item"] - alone).abs() / alone.abs()).max())
    print(f"batched vs one at a time: max rel {rel:.2e}, bit-identical {bool(torch.equal(whole['nll_by_item'], alone))}")
    assert rel <= 1e-6
    rows = sum(len(x) + y.shape[1] for x, y in items)
    chunked = m.score(_collate(items, args), max_rows=rows // 4)
    assert m.last_score["chunks"] >= 3
    rel_c = float(((chunked["nll_by_item"] - whole["nll_by_item"]).abs() / whole["nll_by_item"].abs()).max())
    print(f"{m.last_score['chunks']} chunks vs one launch: max rel {rel_c:.2e}")
    assert rel_c <= 1e-6
    assert _rel(chunked["loss"], whole["loss"]) <= 1e-6 and int(chunked["effective_ntoken"]) == int(whole["effective_ntoken"])


@pytest.mark.parametrize("card,ld", [(70, 72), (70, 80), (2054, 2056), (2056, 2060)])
def test_xent_rank_kernel_against_fp64(card, ld):
    L = _lib.lib()
    g = torch.Generator().manual_seed(card + ld)
    M = 333
    logits = torch.randn(M, ld, generator=g) * 3.0
    logits[: M // 3] = torch.rand(M // 3, ld, generator=g) * 160.0 - 80.0      # logits of magnitude up to 80
    target = torch.randint(0, card, (M,), generator=g)
    target[0], target[1] = 0, card - 1
    # constructed exact ties: rows whose target logit is shared by other columns, some of them at the 10th place
    for r in range(2, 40):
        t = int(target[r])
        others = [c for c in range(card) if c != t][: (r % 12) + 1]
        logits[r, others] = float(logits[r, t])
    for r in range(40, 60):                                           # the target exactly 10th: nine larger, two equal
        order = torch.argsort(logits[r, :card], descending=True)
        t = int(order[9])
        target[r] = t
        logits[r, int(order[10])] = float(logits[r, t])
        logits[r, int(order[11])] = float(logits[r, t])
    logits[:, card:] = 1e30                                           # padding columns must never be read
    d_log = logits.cuda()
    d_t = target.to(torch.int32).cuda()
    nll = torch.full((M,), -1.0, device="cuda")
    rank = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.ssrhip_xent_rank(d_log.data_ptr(), ld, card, d_t.data_ptr(), M, nll.data_ptr(), rank.data_ptr(), _lib.stream_ptr()),
               "ssrhip_xent_rank")
    torch.cuda.synchronize()
    lg64 = logits[:, :card].double()
    ref_nll = torch.logsumexp(lg64, -1) - lg64.gather(1, target[:, None]).squeeze(1)
    tl = logits[:, :card].gather(1, target[:, None])
    ref_rank = (logits[:, :card] > tl).sum(-1)
    got_nll, got_rank = nll.cpu().double(), rank.cpu().long()
    rel = ((got_nll - ref_nll).abs() / ref_nll.abs().clamp(min=1.0)).max().item()
    print(f"card {card} ld {ld}: max nll error {rel:.2e} (relative, absolute below 1)")
    assert rel <= 2e-6
    assert torch.equal(got_rank, ref_rank)
    assert (got_rank[40:60] == 9).all()                               # the tie at the 10th place is a hit


def test_score_between_inference_calls_leaves_the_tokens_unchanged():
    args = W.lm_args_tiny()
    m = _model(args, 9)
    fresh = _model(args, 9)
    g = torch.Generator().manual_seed(9)
    L, T = 10, 18
    x = torch.randint(0, args.text_vocab_size, (1, L), generator=g)
    y = torch.randint(0, args.audio_vocab_size, (1, T, 4), generator=g)
    unc = torch.randint(0, args.text_vocab_size + 1, (1, L), generator=g)
    mi = torch.LongTensor([[[T, T]]])
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True, uncond_x=unc)
    call = lambda mm: mm.inference(x.cuda(), torch.LongTensor([L]), x.cuda(), torch.LongTensor([L]), y.cuda(), y.cuda(), mi.cuda(), **kw)[0].cpu()
    before = call(m)
    items = []
    for i in range(3):
        yy = torch.randint(0, args.audio_vocab_size, (4, 30 + 5 * i), generator=g)
        yy[:, 7] = args.mts
        items.append((torch.randint(0, args.text_vocab_size, (6 + i,), generator=g), yy))
    s1 = m.score(_collate(items, args))
    after = call(m)
    s2 = m.score(_collate(items, args))
    assert torch.equal(before, after) and torch.equal(after, call(fresh))
    assert torch.equal(s1["nll_by_item"], s2["nll_by_item"])
