"""One-GPU config 4 (bench.py's dp64 input: 64 utterances, L = 67, 150-frame prompts, seeds 1000+i / 2000+i, greedy, CFG stride 5)
through `dp.generate` with 8 utterances x CFG per engine pass (group=8, the default: 16 rows) and 16 (group=16: 32 rows), alternating in
ONE process. Prints one JSON line: per group the decode wall time of every round, codec-tokens/s at the best round, and whether the tokens
of the two groupings are identical. The first pass of each grouping (engine build, graph capture) is untimed.

  python tools/dp64_group_ab.py [--reps 2] [--out profiles/xxx.json]
`--wt16` compares, at ONE grouping (the first of --groups, default 8 = 16 rows), a bf16 model whose 16-row engine streams the rounded fp32
masters (SSRHIP_GEMVM_W16=0) against one that streams the packed bf16 streaming-order copies (SSRHIP_GEMVM_W16=1; DESIGN.md Part I.11):
the arena and the engine are rebuilt for every arm of every round (the switch is read when an engine is built), one untimed pass, one timed.
  python tools/dp64_group_ab.py --wt16 --reps 2 --out profiles/wt16_dp64_group8.json
`--wt32` is the same comparison at group 16 = 32 rows (the two-panel step's bf16 stream, DESIGN.md Part I.12; identical tokens asserted):
  python tools/dp64_group_ab.py --wt32 --reps 2 --out profiles/wt32_dp64_group16.json
`--wt8` compares, at group 8 = 16 rows, three arms of an e4m3 model (DESIGN.md Part I.22): the fp32 streaming-order masters
(SSRHIP_GEMVM_W16=0), the 2-byte copies (SSRHIP_GEMVM_W16=1) and the 1-byte codes (SSRHIP_GEMVM_W8=1); per arm the decode wall times, their
median and spread (max - min); identical tokens asserted:
  python tools/dp64_group_ab.py --wt8 --reps 3 --out profiles/wt8_dp64_group8.json
`--kv_dtype bf16` compares, at every grouping of --groups, the model with its fp32 KV cache against `set_kv_dtype("bf16")` (DESIGN.md Part
I.14), the arms alternating within a round; per arm the decode wall times, their median and spread (max - min), and whether the two arms
chose the same tokens (not expected: the cache type changes the numerics):
  python tools/dp64_group_ab.py --kv_dtype bf16 --reps 3 --out profiles/kv16_dp64.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import dp  # noqa: E402
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.engine import W16_STREAMS  # noqa: E402
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--groups", default="8,16")
ap.add_argument("--out", default=None)
ap.add_argument("--wt16", action="store_true", help="bf16 model, group 8: fp32 masters against the packed bf16 stream of the 16-row step")
ap.add_argument("--wt32", action="store_true", help="bf16 model, group 16: fp32 masters against the packed bf16 stream of the 32-row step")
ap.add_argument("--wt8", action="store_true", help="e4m3 model, group 8: fp32 masters against the 2-byte and the 1-byte stream of the 16-row step")
ap.add_argument("--kv_dtype", choices=["fp32", "bf16"], default="fp32", help="bf16: at every grouping, the fp32 KV cache against the bf16 KV cache")
a = ap.parse_args()

dev = torch.device("cuda", 0)
args = W.lm_args_830m()
model = SSR_Speech(args)
model.load_state_dict(W.lm_state_dict(args, seed=0, device=dev))
model = model.to(dev).eval()
utts = []
for i in range(64):
    gx = torch.Generator().manual_seed(1000 + i)
    gy = torch.Generator().manual_seed(2000 + i)
    utts.append({"x": torch.randint(0, 100, (1, 67), generator=gx), "y": torch.randint(0, 2048, (1, 150, 4), generator=gy),
                 "mask_interval": torch.LongTensor([[[150, 150]]])})
kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True)
groups = [int(g) for g in a.groups.split(",")]

if a.wt16 or a.wt32:
    st = next(s for s in reversed(W16_STREAMS) if getattr(a, s.name, False))      # --wt32 wins over --wt16
    kind = st.name
    g = 16 if a.wt32 else groups[0]
    arms = (("bf16_masters", "0"), ("bf16_" + kind, "1"))
    res = {name: {"decode_ms": [], "tokens": None, "launches": 0} for name, _ in arms}
    for rep in range(a.reps):
        for name, sw in arms:
            os.environ[st.switch] = sw
            model.set_weight_dtype("fp32")
            model.set_weight_dtype("bf16")              # drops the arena and the engines: the next call builds them under this switch
            dp.generate(model, utts[:2 * g], seed=0, group=g, **kw)      # untimed: arena, engine, graph capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _ = dp.generate(model, utts, seed=0, group=g, **kw)
            torch.cuda.synchronize()
            res[name]["decode_ms"].append(1000 * (time.perf_counter() - t0))
            res[name]["launches"] = getattr(next(iter(model._engines.values())), kind + "_launches_per_step")
            if res[name]["tokens"] is None:
                res[name]["tokens"] = [t.cpu() for t in toks]
    ref = res["bf16_masters"]["tokens"]
    n_new = sum(int(t.shape[-1]) - 150 for t in ref)
    out = {"workload": "bench.py dp64 input on one GPU through dp.generate (decode only, no codec), bf16 weights", "group": g,
           "rows_per_engine": 2 * g, "new_frames_total": n_new, "reps": a.reps}
    for name, _ in arms:
        best = min(res[name]["decode_ms"])
        out[name] = {"decode_ms": [round(v, 1) for v in res[name]["decode_ms"]], "codec_tokens_per_s": round(4 * n_new / (best * 1e-3), 1),
                     kind + "_launches_per_step": res[name]["launches"]}
    out["tokens_identical"] = all(torch.equal(x, y) for x, y in zip(res["bf16_" + kind]["tokens"], ref))
    assert out["tokens_identical"], "the two bf16 arms must choose the same tokens"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

if a.wt8:
    import statistics
    g = 8
    arms = (("e4m3_masters", {"SSRHIP_GEMVM_W16": "0"}), ("e4m3_wt16", {"SSRHIP_GEMVM_W16": "1"}), ("e4m3_wt8", {"SSRHIP_GEMVM_W8": "1"}))
    res = {name: {"decode_ms": [], "tokens": None} for name, _ in arms}
    for rep in range(a.reps):
        for name, env in arms:
            for k in ("SSRHIP_GEMVM_W16", "SSRHIP_GEMVM_W8"):
                os.environ.pop(k, None)
            os.environ.update(env)
            model.set_weight_dtype("fp32")
            model.set_weight_dtype("e4m3")              # drops the arena and the engines: the next call builds them under these switches
            dp.generate(model, utts[:2 * g], seed=0, group=g, **kw)      # untimed: arena, engine, graph capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _ = dp.generate(model, utts, seed=0, group=g, **kw)
            torch.cuda.synchronize()
            res[name]["decode_ms"].append(1000 * (time.perf_counter() - t0))
            eng = next(iter(model._engines.values()))
            res[name]["launches"] = {"wt16": eng.wt16_launches_per_step, "wt8": eng.wt8_launches_per_step}
            if res[name]["tokens"] is None:
                res[name]["tokens"] = [t.cpu() for t in toks]
    ref = res["e4m3_masters"]["tokens"]
    n_new = sum(int(t.shape[-1]) - 150 for t in ref)
    out = {"workload": "bench.py dp64 input on one GPU through dp.generate (decode only, no codec), e4m3 weights", "group": g,
           "rows_per_engine": 2 * g, "new_frames_total": n_new, "reps": a.reps}
    for name, _ in arms:
        ms = res[name]["decode_ms"]
        med = statistics.median(ms)
        out[name] = {"decode_ms": [round(v, 1) for v in ms], "median_ms": round(med, 1), "spread_ms": round(max(ms) - min(ms), 1),
                     "codec_tokens_per_s": round(4 * n_new / (med * 1e-3), 1), "launches_per_step": res[name]["launches"]}
    out["tokens_identical"] = all(torch.equal(x, y) for name, _ in arms[1:] for x, y in zip(res[name]["tokens"], ref))
    assert out["tokens_identical"], "the three e4m3 arms must choose the same tokens"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

if a.kv_dtype == "bf16":
    import statistics
    arms = ("kv_fp32", "kv_bf16")
    res = {(g, arm): {"decode_ms": [], "tokens": None, "launches": 0} for g in groups for arm in arms}
    for rep in range(a.reps):
        for g in groups:
            for arm in arms:
                model.set_kv_dtype(arm[3:])             # drops the engines: the next call builds one with this cache type
                dp.generate(model, utts[:2 * g], seed=0, group=g, **kw)      # untimed: engine, graph capture
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks, _ = dp.generate(model, utts, seed=0, group=g, **kw)
                torch.cuda.synchronize()
                r = res[(g, arm)]
                r["decode_ms"].append(1000 * (time.perf_counter() - t0))
                eng = next(iter(model._engines.values()))
                r["launches"], r["kv_pool_bytes"] = eng.kv16_launches_per_step, eng.kv_pool_bytes
                if r["tokens"] is None:
                    r["tokens"] = [t.cpu() for t in toks]
    out = {"workload": "bench.py dp64 input on one GPU through dp.generate (decode only, no codec), fp32 weights", "reps": a.reps}
    for g in groups:
        o = {"rows_per_engine": 2 * g}
        for arm in arms:
            r = res[(g, arm)]
            n_new = sum(int(t.shape[-1]) - 150 for t in r["tokens"])
            med = statistics.median(r["decode_ms"])
            o[arm] = {"decode_ms": [round(v, 1) for v in r["decode_ms"]], "median_ms": round(med, 1), "spread_ms": round(max(r["decode_ms"]) - min(r["decode_ms"]), 1),
                      "new_frames_total": n_new, "codec_tokens_per_s": round(4 * n_new / (med * 1e-3), 1), "kv16_launches_per_step": r["launches"],
                      "kv_pool_bytes": r["kv_pool_bytes"]}
        o["tokens_identical"] = all(torch.equal(x, y) for x, y in zip(res[(g, "kv_fp32")]["tokens"], res[(g, "kv_bf16")]["tokens"]))
        out[f"group{g}"] = o
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

res = {g: {"decode_ms": [], "tokens": None} for g in groups}
for g in groups:                                   # untimed: engine, graph capture
    dp.generate(model, utts[:2 * g], seed=0, group=g, **kw)
for rep in range(a.reps):
    for g in groups:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks, _ = dp.generate(model, utts, seed=0, group=g, **kw)
        torch.cuda.synchronize()
        res[g]["decode_ms"].append(1000 * (time.perf_counter() - t0))
        if res[g]["tokens"] is None:
            res[g]["tokens"] = [t.cpu() for t in toks]
n_new = sum(int(t.shape[-1]) - 150 for t in res[groups[0]]["tokens"])
out = {"workload": "bench.py dp64 input on one GPU through dp.generate (decode only, no codec)", "new_frames_total": n_new, "reps": a.reps}
for g in groups:
    best = min(res[g]["decode_ms"])
    out[f"group{g}"] = {"rows_per_engine": 2 * g, "decode_ms": [round(v, 1) for v in res[g]["decode_ms"]],
                        "codec_tokens_per_s": round(4 * n_new / (best * 1e-3), 1)}
ref = res[groups[0]]["tokens"]
out["tokens_identical"] = all(len(res[g]["tokens"]) == len(ref) and all(torch.equal(x, y) for x, y in zip(res[g]["tokens"], ref)) for g in groups)
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
