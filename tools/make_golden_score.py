"""Fixtures of `SSR_Speech.score` (tests/golden/score_*.npz): the REFERENCE's training forward (models/ssr.py:280-379) run on the CPU
in the host-independent mode of oracle/numerics.py, weights from `weights.lm_state_dict(args, seed)`.

    python tools/make_golden_score.py [--out DIR]        (from the repository root; needs the reference checkout)

Each fixture holds the collated batch (x, x_lens, y, y_lens; y built with the reference model's own rearrange / shift / insert_mask /
cat_y and padded like data/gigaspeech.py:298-321), the flags, the reference's returned dict, and per position (k, b, t) the cross entropy
and the rank of the target (logits strictly above it) derived from the logits the reference's `predict_layer[k]` produced, captured with
forward hooks.

The reference's `torchmetrics.MulticlassAccuracy` is not installed here: before the reference is imported, a `torchmetrics` module is
installed whose `MulticlassAccuracy(top_k=10, average="micro")` restates top-k micro accuracy (a target counts when it is among
`preds.topk(top_k)`; no rows -> 0). Every fixture says so in its `metric_note`.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import numerics  # noqa: E402

assert "torch" not in sys.modules, "oracle/numerics.py's mode must be set before torch starts"
os.environ.update(numerics.ENV)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

METRIC_NOTE = ("torchmetrics is not installed: MulticlassAccuracy(top_k, average='micro') is restated as the fraction of rows whose "
               "target is in preds.topk(top_k) (0 for no rows)")


def install_torchmetrics():
    tm = types.ModuleType("torchmetrics")
    tmc = types.ModuleType("torchmetrics.classification")

    class MulticlassAccuracy(torch.nn.Module):
        def __init__(self, num_classes, top_k=1, average="micro", multidim_average="global", ignore_index=None):
            super().__init__()
            assert average == "micro" and multidim_average == "global" and ignore_index is None
            self.top_k = top_k

        def forward(self, preds, target):
            if target.numel() == 0:
                return torch.tensor(0.0)
            hit = (preds.topk(self.top_k, dim=-1).indices == target.unsqueeze(-1)).any(-1)
            return hit.float().mean()

    tmc.MulticlassAccuracy = MulticlassAccuracy
    tm.classification = tmc
    sys.modules["torchmetrics"] = tm
    sys.modules["torchmetrics.classification"] = tmc


# name, tiny-config kwargs, flags, items [(text len, audio frames, mask intervals)], pad_x width (0 = pad_sequence), weight seed
CASES = [
    ("ragged_b3", dict(), dict(predict_mask_token=1, predict_all=0, codebook_weight=None),
     [(7, 20, [[4, 9]]), (12, 31, [[3, 6], [15, 22]]), (5, 26, [[2, 5], [9, 12], [20, 24]])], 0, 41),
    ("all_cw_hd128", dict(d_model=256, nhead=2, layers=2, vocab=128), dict(predict_mask_token=0, predict_all=1, codebook_weight="[3,1,1,1]"),
     [(9, 24, [[5, 11]]), (14, 18, [[18, 18]]), (6, 30, [[0, 4], [20, 27]])], 0, 42),
    ("pad_x", dict(), dict(predict_mask_token=1, predict_all=0, codebook_weight=None),
     [(8, 22, [[6, 10]]), (13, 17, [[2, 8]])], 20, 43),
    ("empty_tmp_cb3", dict(), dict(predict_mask_token=0, predict_all=0, codebook_weight=None),
     [(6, 19, [[5, 9]]), (10, 25, [[4, 7], [14, 18]])], 0, 44),
]


def build_y(m, args, T, mi, g):
    """One item's y [K, T'] the reference's way (models/ssr.py:381-502)."""
    K = args.n_codebooks
    codes = torch.randint(0, args.audio_vocab_size, (K, T), generator=g)
    starts = [a for a, _ in mi] + [T]
    ends = [0] + [b for _, b in mi]
    nmi = list(zip(ends, starts))
    rearranged = m.rearrange(codes, nmi, [tuple(v) for v in mi])
    shifted = m.shift(rearranged)
    inserted, _ = m.insert_mask(shifted)
    cated, _ = m.cat_y(inserted)
    return cated


def make_case(ssr, case):
    from ssr_speech_amd import weights as W
    name, cfg, flags, spec, pad_x, seed = case
    args = W.lm_args_tiny(**cfg)
    for k, v in flags.items():
        setattr(args, k, v)
    m = ssr.SSR_Speech(args).eval()
    sd = W.lm_state_dict(args, seed=seed)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("accuracy_metrics") for k in res.missing_keys), res
    g = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for L, T, mi in spec:
        xs.append(torch.randint(0, args.text_vocab_size, (L,), generator=g))
        ys.append(build_y(m, args, T, mi, g))
    if name.startswith("empty_tmp"):
        # the last codebook of every item: its last mask token moved to 3 before the end, then only empty tokens -> tmp_mask empty
        for y in ys:
            y[-1, -3] = args.mts
            y[-1, -2:] = args.empty_token
    if pad_x:
        x = torch.stack([F.pad(v, (0, pad_x - v.shape[0]), value=args.text_pad_token) for v in xs])
    else:
        x = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True, padding_value=args.text_pad_token)
    y = torch.nn.utils.rnn.pad_sequence([v.transpose(1, 0) for v in ys], padding_value=args.audio_pad_token).permute(1, 2, 0)
    batch = dict(x=x, x_lens=torch.LongTensor([v.shape[0] for v in xs]), y=y.contiguous(), y_lens=torch.LongTensor([v.shape[1] for v in ys]))
    logits = {}
    hooks = [m.predict_layer[k].register_forward_hook(lambda mod, inp, out, k=k: logits.__setitem__(k, out.detach().clone()))
             for k in range(args.n_codebooks)]
    try:
        with torch.no_grad():
            out = m.forward(dict(batch))
    finally:
        for h in hooks:
            h.remove()
    lg = torch.stack([logits[k] for k in range(args.n_codebooks)])[:, :, :-1]          # [K, B, S-1, card]
    tg = batch["y"][:, :, : int(batch["y_lens"].max())].permute(1, 0, 2)[:, :, 1:]     # [K, B, S-1]
    ce = F.cross_entropy(lg.reshape(-1, lg.shape[-1]), tg.reshape(-1), reduction="none").reshape(tg.shape)
    tl = lg.gather(-1, tg.unsqueeze(-1))
    rank = (lg > tl).sum(-1)                                                           # strictly above: the target column never counts
    flag_np = {f"flag_{k}": np.asarray("" if v is None else v) for k, v in flags.items()}
    d = dict(cfg=np.asarray([args.d_model, args.nhead, args.num_decoder_layers, args.audio_vocab_size]), weight_seed=np.asarray(seed),
             x=batch["x"].numpy(), x_lens=batch["x_lens"].numpy(), y=batch["y"].numpy(), y_lens=batch["y_lens"].numpy(),
             loss=out["loss"].numpy(), top10acc=out["top10acc"].numpy(),
             top10acc_by_codebook=torch.stack(out["top10acc_by_codebook"]).numpy(), effective_ntoken=out["effective_ntoken"].numpy(),
             ce=ce.numpy(), rank=rank.numpy().astype(np.int32), torch_version=np.asarray(torch.__version__),
             metric_note=np.asarray(METRIC_NOTE), **flag_np)
    print(f"  score_{name}: B={x.shape[0]} loss={float(out['loss']):.6g} top10acc={float(out['top10acc']):.6g} "
          f"ntoken={int(out['effective_ntoken'])}")
    return d


def main(out_dir=None):
    torch.set_num_threads(numerics.THREADS)
    out_dir = out_dir or os.path.join(ROOT, "tests", "golden")
    install_torchmetrics()
    from oracle import ref_import
    ssr = ref_import.import_lm()
    for case in CASES:
        np.savez_compressed(os.path.join(out_dir, f"score_{case[0]}.npz"), **make_case(ssr, case))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(ap.parse_args().out)
