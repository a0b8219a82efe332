"""Does the host-side noise feed keep up with a batched sampled decode, and what does the device-side source buy (DESIGN.md Part I.21)?

Sampled `inference_batch` (top_k=40, top_p=0.8, CFG stride 5) on bench.py's dp64 input (64 utterances, L = 67, 150-frame prompts, seeds
1000+i / 2000+i) at `group` 8 and 16, and the batch-1 step (group 1, the first --batch1-utts utterances), 830M shape, one GPU. The arms
`torch_cpu` and `philox` (SSR_Speech.set_sampling_rng) run in ONE process, alternating, --reps rounds after one untimed pass per arm and
grouping. Per arm: the wall time of every round, codec-tokens/s at the median, the host seconds spent per chunk drawing (`feed.draw`) or
enqueueing (`PhiloxNoise.send`) the noise, the GPU time per 16-step chunk (events around every `DecodeEngine.decode`), and whether the
tokens are equal across the rounds of the arm. The verdict is I.11's gate: the philox median below the torch_cpu median of the same process
by more than the philox arm's spread and by at least 1 %. The two arms draw different noise, so they choose different tokens and decode
different numbers of frames in different numbers of chunks: the gate is applied twice, to the wall time per generated frame (which is
codec-tokens/s, and depends on how long the utterances of an arm happen to run) and to the wall time per 16-step chunk (which does not).

  python tools/noise_feed_ab.py [--reps 4] [--groups 8,16,1] [--out profiles/noise_feed_ab.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import engine as E  # noqa: E402
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--groups", default="8,16,1")
ap.add_argument("--utts", type=int, default=64)
ap.add_argument("--batch1-utts", type=int, default=8, help="how many of the utterances the group-1 rows decode (one after the other)")
ap.add_argument("--tiny", action="store_true", help="a tiny model instead of the 830M shape (a dry run of the tool itself)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
args = W.lm_args_tiny(d_model=128, nhead=2, layers=2, vocab=64) if a.tiny else W.lm_args_830m()
model = SSR_Speech(args)
model.load_state_dict(W.lm_state_dict(args, seed=0, device=dev))
model = model.to(dev).eval()
V, NT = int(args.audio_vocab_size), int(args.text_vocab_size)
utts = []
for i in range(a.utts):
    gx = torch.Generator().manual_seed(1000 + i)
    gy = torch.Generator().manual_seed(2000 + i)
    utts.append({"x": torch.randint(0, min(100, NT), (1, 67), generator=gx), "y": torch.randint(0, V, (1, 150, 4), generator=gy),
                 "mask_interval": torch.LongTensor([[[150, 150]]])})
kw = dict(top_k=40, top_p=0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True)

# ---- the probes: host seconds in the noise source, GPU time of every decode call
host = {"s": 0.0, "calls": 0}
chunks = []


def timed(fn):
    def wrapped(*args_, **kw_):
        t0 = time.perf_counter()
        out = fn(*args_, **kw_)
        host["s"] += time.perf_counter() - t0
        host["calls"] += 1
        return out
    return wrapped


E.TorchCpuNoiseFeed.draw = timed(E.TorchCpuNoiseFeed.draw)          # one call per utterance and chunk
E.PhiloxNoise.send = timed(E.PhiloxNoise.send)                      # one call per chunk, whatever the number of utterances
_decode = E.DecodeEngine.decode


def decode(self, n_steps, use_graph=True):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _decode(self, n_steps, use_graph)
    e1.record()
    chunks.append((e0, e1))


E.DecodeEngine.decode = decode

ARMS = ("torch_cpu", "philox")
groups = [int(g) for g in a.groups.split(",")]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def save():
    """after every grouping: a run that is cut short leaves what it measured"""
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def one_pass(arm, g):
    model.set_sampling_rng(arm)
    work = utts if g > 1 else utts[: a.batch1_utts]
    host["s"], host["calls"] = 0.0, 0
    del chunks[:]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = model.inference_batch(work, seed=0, group=g, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    gpu_ms = sum(e0.elapsed_time(e1) for e0, e1 in chunks)
    frames = sum(int(r[0].shape[-1]) - 150 for r in res)
    return dict(wall=wall, frames=frames, chunks=len(chunks), gpu_ms=gpu_ms, host_s=host["s"], host_calls=host["calls"],
                tokens=[r[0].cpu() for r in res])


say("# Sampled batch decode: host-drawn torch_cpu noise against device-side philox noise")
say()
say(f"`tools/noise_feed_ab.py --reps {a.reps} --groups {a.groups}`" + (" --tiny" if a.tiny else "") +
    f": {'tiny' if a.tiny else '830M'} shape, {a.utts} utterances (group 1: the first {a.batch1_utts}), top_k=40, top_p=0.8, CFG stride 5, "
    "one process, arms alternating, one untimed pass per arm and grouping first. us/frame = wall time per generated frame, tok/s = 4 codec "
    "tokens per frame; wall ms/chunk = wall time per 16-step engine pass (prefills included). The arms draw different noise: they decode "
    "different numbers of frames in different numbers of chunks, so tok/s also depends on how long an arm's utterances happen to run; wall "
    "ms/chunk does not.")
say()
for g in groups:
    for arm in ARMS:                                   # untimed: engine, graph capture, pinned staging
        one_pass(arm, g)
    runs = {arm: [] for arm in ARMS}
    for rep in range(a.reps):
        for arm in ARMS:
            runs[arm].append(one_pass(arm, g))
    say(f"## group {g} ({2 * g} rows)")
    say()
    say("| arm | us/frame, median | all rounds | spread (max - min) | tok/s at the median | wall ms/chunk, median | all rounds | spread | frames | "
        "chunks | host ms per chunk in the noise source (calls per chunk) | GPU ms per chunk | tokens equal across rounds |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    stat = {}
    for arm in ARMS:
        rs = runs[arm]
        per = [1e6 * r["wall"] / r["frames"] for r in rs]
        med, spread = statistics.median(per), max(per) - min(per)
        same = all(len(r["tokens"]) == len(rs[0]["tokens"]) and all(torch.equal(x, y) for x, y in zip(r["tokens"], rs[0]["tokens"])) for r in rs)
        r0 = rs[0]
        pc = [1e3 * r["wall"] / r["chunks"] for r in rs]
        stat[arm] = ((med, spread), (statistics.median(pc), max(pc) - min(pc)))
        say(f"| `{arm}` | {med:.2f} | {' '.join(f'{v:.2f}' for v in per)} | {spread:.2f} | {4e6 / med:.0f} | {stat[arm][1][0]:.3f} | "
            f"{' '.join(f'{v:.3f}' for v in pc)} | {stat[arm][1][1]:.3f} | {r0['frames']} | {r0['chunks']} | "
            f"{statistics.median(1e3 * r['host_s'] / r['chunks'] for r in rs):.3f} ({r0['host_calls'] / r0['chunks']:.2f}) | "
            f"{statistics.median(r['gpu_ms'] / r['chunks'] for r in rs):.3f} | {same} |")
    say()
    say("Gate (philox median below the torch_cpu median by more than the philox arm's spread and by at least 1 %):")
    for i, unit in enumerate(("us/frame", "wall ms/chunk")):
        (mt, _), (mp, sp) = stat["torch_cpu"][i], stat["philox"][i]
        gain = mt - mp
        ok = gain > sp and gain >= 0.01 * mt
        say(f"- {unit}: {mt:.3f} - {mp:.3f} = {gain:.3f} ({100 * gain / mt:.1f} %) against a spread of {sp:.3f}: **{'holds' if ok else 'does not hold'}**.")
    say()
    save()
say("Whichever way the gate falls, the default stays `torch_cpu`.")
save()
