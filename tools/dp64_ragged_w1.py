"""Does the shorter one-plane prefill (DESIGN I.13) show where every admission stalls the batch? bench.py's `dp64_ragged` workload — 64
utterances, L uniform in 20..120 phonemes, 150-frame prompts, greedy + CFG, 8 utterance slots with refill, one GPU — on two
`weight_dtype="bf16"` models in ONE process: three planes per matrix (`SSRHIP_PREFILL_W1=0` while its planes are built) against one plane
(`=1`), one warm-up run each, then `--rounds` alternating runs. Prints one JSON line: tokens/s per round, median and spread per arm, and
whether both arms produced the same tokens.

    python tools/dp64_ragged_w1.py [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    args = W.lm_args_830m()
    sd = {k: v.cpu() for k, v in W.lm_state_dict(args, seed=0, device="cuda").items()}
    g = torch.Generator().manual_seed(77)
    utts = []
    for _ in range(64):
        L = int(torch.randint(20, 121, (1,), generator=g))
        utts.append({"x": torch.randint(0, 100, (1, L), generator=g), "y": torch.randint(0, 2048, (1, 150, 4), generator=g),
                     "mask_interval": torch.LongTensor([[[150, 150]]])})
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True)

    def run(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.inference_batch(utts, seed=0, refill=True, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        crc = 0
        for r in res:
            crc = zlib.crc32(r[0].cpu().numpy().astype("<i8").tobytes(), crc)
        return 4 * sum(int(r[0].shape[-1]) - 150 for r in res) / dt, 1000 * dt, crc

    models, tps, crcs = {}, {}, set()
    for name, w1 in (("bf16x3", "0"), ("bf16x1", "1")):
        m = SSR_Speech(args)
        m.load_state_dict(sd)
        m = m.to("cuda").eval()
        m.set_weight_dtype("bf16")
        os.environ["SSRHIP_PREFILL_W1"] = w1                     # read once, where this model's planes are built: the warm-up run
        crcs.add(run(m)[2])
        models[name], tps[name] = m, []
    os.environ.pop("SSRHIP_PREFILL_W1")
    for _ in range(o.rounds):
        for name, m in models.items():
            t, _, crc = run(m)
            tps[name].append(round(t, 1))
            crcs.add(crc)
    res = dict(metric="dp64_ragged_refill_bf16_arms", rounds=o.rounds, same_tokens=len(crcs) == 1, arms={})
    for name, m in models.items():
        res["arms"][name] = dict(planes=m._arena.split_planes, tokens_per_s_median=statistics.median(tps[name]),
                                 tokens_per_s_spread=round(max(tps[name]) - min(tps[name]), 1), tokens_per_s_all=tps[name],
                                 admissions=next(iter(m._engines.values())).n_admitted)
    line = json.dumps(res)
    print(line)
    if o.out:
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
