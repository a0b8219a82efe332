"""Throughput of `SSR_Speech.score` at the 830M shape: 64 utterances (text 60-140 ids, 250-1000 audio frames, 1-3 masked spans), seeded
weights, one warm-up pass and five timed passes (hipEvents around each pass, host planning included). Prints one JSON line.

    python tools/score_bench.py [--utts 64] [--passes 5] [--max-rows 16384] [--out FILE] [--arms]

--arms: three models in one process, their timed passes alternating — fp32, weight_dtype="bf16" with three planes per matrix, and bf16
with one plane (`SSRHIP_PREFILL_W1`, set here while each model's planes are built; DESIGN I.13). The JSON line then carries per arm the
median ms per pass, its spread (max - min) and rows/s, and whether the two bf16 arms returned the same loss bit for bit.

FLOPs counted: 2 x (layer weights) x rows + 2 x (head weights) x scored rows + causal attention (QK^T and PV over the n(n+1)/2 visible
pairs of every item and layer: 4 x D x n(n+1)/2)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402


def make_batch(args, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    K, V = args.n_codebooks, args.audio_vocab_size
    xs, ys = [], []
    for _ in range(n):
        L = int(torch.randint(60, 141, (1,), generator=g))
        T = int(torch.randint(250, 1001, (1,), generator=g))
        y = torch.randint(0, V, (K, T), generator=g)
        y[:, 0] = args.sos
        n_spans = int(torch.randint(1, 4, (1,), generator=g))
        cut = sorted(torch.randperm(T - 2, generator=g)[: 2 * n_spans].add(1).tolist())
        for i in range(n_spans):                      # each span's mask token twice: where the span was, and where its codes follow
            y[:, cut[i]] = args.mts + i
            y[:, cut[n_spans + i]] = args.mts + i
        xs.append(torch.randint(0, args.text_vocab_size, (L,), generator=g))
        ys.append(y)
    x = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True, padding_value=args.text_pad_token)
    y = torch.nn.utils.rnn.pad_sequence([v.transpose(1, 0) for v in ys], padding_value=args.audio_pad_token).permute(1, 2, 0).contiguous()
    return dict(x=x, x_lens=torch.LongTensor([len(v) for v in xs]), y=y, y_lens=torch.LongTensor([v.shape[1] for v in ys]))


def arms(a):
    """fp32 | bf16 x 3 planes | bf16 x 1 plane, alternating passes in one process"""
    import statistics
    args = W.lm_args_830m()
    sd = {k: v.cpu() for k, v in W.lm_state_dict(args, seed=0, device="cuda").items()}
    batch = make_batch(args, a.utts)
    models, out = {}, {}
    for name, dtype, w1 in (("fp32", "fp32", "0"), ("bf16x3", "bf16", "0"), ("bf16x1", "bf16", "1")):
        m = SSR_Speech(args)
        m.load_state_dict(sd)
        m = m.to("cuda").eval()
        m.set_weight_dtype(dtype)
        os.environ["SSRHIP_PREFILL_W1"] = w1                     # read once, where this model's planes are built: the warm-up pass
        out[name] = m.score(batch, max_rows=a.max_rows)
        torch.cuda.synchronize()
        models[name] = m
    os.environ.pop("SSRHIP_PREFILL_W1")
    ms = {name: [] for name in models}
    for _ in range(a.passes):
        for name, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = m.score(batch, max_rows=a.max_rows)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    rows = models["fp32"].last_score["rows"]
    res = dict(metric="score_830m_arms", utts=a.utts, rows=rows, passes=a.passes, max_rows=a.max_rows,
               bf16_losses_equal=bool(torch.equal(out["bf16x3"]["loss"], out["bf16x1"]["loss"])), arms={})
    for name, m in models.items():
        med = statistics.median(ms[name])
        res["arms"][name] = dict(planes=m._arena.split_planes, plane_bytes=m._arena.split_plane_bytes(), ms_median=round(med, 3),
                                 ms_spread=round(max(ms[name]) - min(ms[name]), 3), ms_all=[round(v, 3) for v in ms[name]],
                                 rows_per_s=round(rows / med * 1e3, 1), loss=float(out[name]["loss"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arms", action="store_true")
    a = ap.parse_args()
    if a.arms:
        line = json.dumps(arms(a))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    args = W.lm_args_830m()
    sd = W.lm_state_dict(args, seed=0, device="cuda")
    m = SSR_Speech(args)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    del sd
    m = m.to("cuda").eval()
    batch = make_batch(args, a.utts)
    out = m.score(batch, max_rows=a.max_rows)              # warm-up: arena, split planes, workspaces
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = m.score(batch, max_rows=a.max_rows)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = m.last_score
    D, F, L = args.d_model, 4 * args.d_model, args.num_decoder_layers
    K, V = args.n_codebooks, args.audio_vocab_size
    Hh, card = V // 2, V + args.n_special + args.max_n_spans
    layer_w = L * (4 * D * D + 2 * D * F)
    head_w = K * (D * Hh + Hh * card)
    lens = (batch["x_lens"] + batch["y_lens"]).tolist()
    attn = sum(L * 4 * D * n * (n + 1) // 2 for n in lens)
    flops = 2 * layer_w * st["rows"] + 2 * head_w * st["scored_rows"] + attn
    best = min(ms)
    res = dict(metric="score_830m", utts=a.utts, rows=st["rows"], scored_rows=st["scored_rows"], chunks=st["chunks"], max_rows=a.max_rows,
               ms_per_pass=round(sum(ms) / len(ms), 3), ms_best=round(best, 3), ms_all=[round(v, 3) for v in ms],
               rows_per_s=round(st["rows"] / (sum(ms) / len(ms)) * 1e3, 1), tflops=round(flops / (sum(ms) / len(ms)) / 1e9, 1),
               loss=float(out["loss"]), top10acc=float(out["top10acc"]), effective_ntoken=int(out["effective_ntoken"]),
               peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
