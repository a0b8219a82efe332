"""A/B of decode-step variants in ONE process on ONE box (round 5): the 830M weights are generated once, then for every variant — a set
of environment knobs the C side reads when a launch is ENQUEUED, i.e. at graph capture — a fresh DecodeEngine is built, started on
bench.py's config-2 input and timed exactly like bench.py's headline (W untimed steps, K timed, wall clock around `eng.decode`), plus
the per-category graph-chained launch times. Variants alternate over `--reps` rounds; per variant the list of ms/step is printed with
its minimum and median (box-to-box spread is 3-5 %, so only same-box alternating runs can resolve a 1 % change).

  python tools/decode_ab.py [--utts U] [--steps K] [--warmup W] [--reps R] name[@U]:KNOB=v,KNOB=v ...
  e.g. python tools/decode_ab.py base:SSRHIP_GEMV_SEGU=0,SSRHIP_ATTN_PIN=0 segu4: segu2:SSRHIP_GEMV_SEGU=2
`@U` gives a variant its own utterance count (default --utts), so that step widths can be compared in one process, alternating:
  python tools/decode_ab.py --warmup 180 --steps 100 rows16@8: rows32@16:     (16 against 32 rows, timed around context ~520)
Utterance u decodes bench.py's synth_inputs(u) prompt (config 4's input); codec-tokens/s = 4 codebooks x U / step time.
A lower-case `weight_dtype=bf16` among a variant's knobs is not an environment variable: that variant runs on a second arena built with
weight_dtype="bf16" (rounded masters + packed copies, 3.3 + 1.65 GB beside the fp32 one), e.g. the four arms of the bf16 weight stream:
  python tools/decode_ab.py fp32_paired: fp32_unpaired:SSRHIP_GEMV_PAIR=0 bf16_masters:weight_dtype=bf16,SSRHIP_GEMV_W16=0 bf16_w16:weight_dtype=bf16
(`tokens == <first variant>` is then expected to be False across dtypes and True between the two bf16 arms.)
The same at 5..16 rows (DESIGN.md Part I.11; `SSRHIP_GEMVM_W16` is the switch of those engines, `wt16 launches` their counter):
  python tools/decode_ab.py --utts 8 --greedy --warmup 180 --steps 100 fp32: bf16_masters:weight_dtype=bf16,SSRHIP_GEMVM_W16=0 bf16_wt16:weight_dtype=bf16,SSRHIP_GEMVM_W16=1
and at 17..32 rows (DESIGN.md Part I.12; the same switch, `wt32 launches` the counter):
  python tools/decode_ab.py --utts 16 --greedy --warmup 180 --steps 100 fp32: bf16_masters:weight_dtype=bf16,SSRHIP_GEMVM_W16=0 bf16_wt32:weight_dtype=bf16,SSRHIP_GEMVM_W16=1
A lower-case `kv_dtype=bf16` is not an environment variable either: that variant's engine keeps its KV cache in 2-byte entries (DESIGN.md
Part I.14; 5..32 rows, `kv16 launches` its counter), independent of `weight_dtype`:
  python tools/decode_ab.py --utts 16 --greedy --warmup 180 --steps 100 fp32: kv16:kv_dtype=bf16 bf16_wt:weight_dtype=bf16,SSRHIP_GEMVM_W16=1 bf16_wt_kv16:weight_dtype=bf16,SSRHIP_GEMVM_W16=1,kv_dtype=bf16
A lower-case `share_prompt=0|1` (DESIGN.md Part I.15) gives the variant the input of `--sample_batch_size U`: U samples of ONE utterance —
every conditional row carries utterance 0's text, the unconditional rows keep their own (what `aug_text` draws) — and `share_prompt=1`
builds its engine with share_prompt=True (one prefill and one set of prompt pages for the conditional rows, the grouped attention walk;
`group launches` its counter). Both arms print the rows their first fill prefilled, its device time (the prefill and what the admission enqueues behind it: a sharing
engine's copies of the prompt's partial page) and the KV pages in use:
  python tools/decode_ab.py --utts 16 --greedy --warmup 180 --steps 100 unshared:share_prompt=0 shared:share_prompt=1
`weight_dtype=e4m3` builds a third arena (DESIGN.md Part I.18: OCP e4m3 codes with a power-of-two scale per row; 3.3 + 0.82 GB); `w8 launches`
is the counter of its <= 4-row stream, `SSRHIP_GEMV_W8=0` streams its fp32 masters instead, `SSRHIP_GEMV_W8_DEPTH` picks the ring:
  python tools/decode_ab.py --reps 4 fp32_paired: bf16_w16:weight_dtype=bf16 e4m3_masters:weight_dtype=e4m3,SSRHIP_GEMV_W8=0 e4m3_w8:weight_dtype=e4m3
The e4m3 weight stream at 5..16 rows (DESIGN.md Part I.22; `SSRHIP_GEMVM_W8=1` is the opt-in, `wt8 launches` the counter; an arm is also
compared with the first arm on the same weights and cache, here `e4m3_masters`):
  python tools/decode_ab.py --utts 8 --greedy --warmup 180 --steps 100 --reps 4 fp32: e4m3_masters:weight_dtype=e4m3,SSRHIP_GEMVM_W16=0 e4m3_wt16:weight_dtype=e4m3,SSRHIP_GEMVM_W16=1 e4m3_wt8:weight_dtype=e4m3,SSRHIP_GEMVM_W8=1
Pair launches over the bf16 weight stream (DESIGN.md Part I.19; `SSRHIP_GEMV_W16_PAIR=1` is the opt-in, `w16 pair launches` the counter,
`pairing` whether the arm's engine held the pairing slot):
  python tools/decode_ab.py --reps 4 fp32: bf16_w16:weight_dtype=bf16 bf16_w16_pair:weight_dtype=bf16,SSRHIP_GEMV_W16_PAIR=1
Pair launches over the e4m3 weight stream (DESIGN.md Part I.20; `SSRHIP_GEMV_W8_PAIR=1` is the opt-in, `w8 pair launches` the counter):
  python tools/decode_ab.py --reps 4 fp32: e4m3_w8:weight_dtype=e4m3 e4m3_w8_pair:weight_dtype=e4m3,SSRHIP_GEMV_W8_PAIR=1
Pair launches of the 4-row step over the fp32 weights (DESIGN.md Part I.24; `SSRHIP_GEMV_PAIR4=1` is the opt-in, `pair4` the counter):
  python tools/decode_ab.py --utts 2 --warmup 180 --steps 100 --reps 4 unpaired: pair4:SSRHIP_GEMV_PAIR4=1
Pair launches of the 4-row step over the packed streams (DESIGN.md Part I.26; `SSRHIP_GEMV_PAIR4_PK=1` is the opt-in, `pair4 pk` the counter):
  python tools/decode_ab.py --utts 2 --warmup 180 --steps 100 --reps 4 bf16:weight_dtype=bf16 bf16_pk:weight_dtype=bf16,SSRHIP_GEMV_PAIR4_PK=1 e4m3:weight_dtype=e4m3 e4m3_pk:weight_dtype=e4m3,SSRHIP_GEMV_PAIR4_PK=1
A lower-case `kv16_small=1` (DESIGN.md Part I.23; 1, 2 or 4 rows) builds the arm's engine with kv_dtype="bf16", kv16_small=True: the 2-byte
cache behind the landing cache of the split-KV step (`kv16 launches` its counter, `attn` its per-launch time), under any weight stream:
  python tools/decode_ab.py --reps 4 --warmup 180 --steps 100 fp32: fp32_kv16:kv16_small=1 e4m3_pair:weight_dtype=e4m3,SSRHIP_GEMV_W8_PAIR=1 e4m3_pair_kv16:weight_dtype=e4m3,SSRHIP_GEMV_W8_PAIR=1,kv16_small=1
A lower-case `logprobs=1` (DESIGN.md Part I.27; any row count) builds the arm's engine with logprobs=True: the step's sampler launch is
ssrhip_sample_logp (`sample` its per-launch time; the arm also prints how many log-probabilities of utterance 0 are not NaN, and their mean):
  python tools/decode_ab.py --reps 4 --warmup 180 --steps 100 default: logprobs:logprobs=1
  python tools/decode_ab.py --utts 8 --reps 4 --warmup 180 --steps 100 default: logprobs:logprobs=1
"""
import argparse
import dataclasses
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import layout as LY  # noqa: E402
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.engine import COUNTERS, W16_STREAMS, DecodeEngine, DecodeKnobs, LMWeightsArena  # noqa: E402
from bench import synth_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=1)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--greedy", action="store_true", help="top_k=1 instead of bench.py's sampling knobs (tokens comparable across variants)")
ap.add_argument("variants", nargs="+")
a = ap.parse_args()

variants = []
utts_of = {}
for v in a.variants:
    name, _, kn = v.partition(":")
    name, _, nu = name.partition("@")
    utts_of[name] = int(nu) if nu else a.utts
    variants.append((name, dict(kv.split("=", 1) for kv in kn.split(",") if kv)))
dtype_of = {name: d.pop("weight_dtype", "fp32") for name, d in variants}
kv_of = {name: d.pop("kv_dtype", "fp32") for name, d in variants}
small_of = {name: d.pop("kv16_small", "0") == "1" for name, d in variants}
kv_of = {name: "bf16" if small_of[name] else kv for name, kv in kv_of.items()}
logp_of = {name: d.pop("logprobs", "0") == "1" for name, d in variants}
share_of = {name: d.pop("share_prompt", None) for name, d in variants}      # None: U utterances; "0" / "1": U samples of utterance 0
all_knobs = sorted({k for _, d in variants for k in d})

dev = torch.device("cuda", 0)
args_lm = W.lm_args_830m()
sd = W.lm_state_dict(args_lm, seed=0, device=dev)
arenas = {dt: LMWeightsArena(args_lm, sd, dev, weight_dtype=dt) for dt in sorted(set(dtype_of.values()))}
del sd
x, y, unc = synth_inputs(args_lm, 0)
L, N = x.shape[1], y.shape[1]
total = a.warmup + a.steps
cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), np.asarray([[N, N]]), args_lm)
T0 = cated.shape[1]
text_rows = []
for u in range(max(utts_of.values())):
    xu, _, uu = (x, y, unc) if u == 0 else synth_inputs(args_lm, u)
    text_rows += [xu[0].numpy(), uu[0].numpy()]
kn = DecodeKnobs(top_k=1 if a.greedy else 40, top_p=1.0 if a.greedy else 0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5,
                 use_cfg=True, text_len=L, n_spans=num_task, seed=2024)

res = {name: {"ms": [], "gemv": [], "attn": [], "sample": [], "tok": None, **{st.name: 0 for st in W16_STREAMS}} for name, _ in variants}
for rep in range(a.reps):
    for name, knobs in variants:
        for k in all_knobs:
            os.environ.pop(k, None)
        os.environ.update(knobs)
        U = utts_of[name]
        eng = DecodeEngine(arenas[dtype_of[name]], U, True, ((L + T0 + total + 8 + 1023) // 1024) * 1024, ((total + 255) // 256) * 256,
                           kv_dtype=kv_of[name], share_prompt=share_of[name] == "1", kv16_small=True if small_of[name] else None, logprobs=logp_of[name])
        rows_in = text_rows[:2 * U] if share_of[name] is None else [text_rows[r] if r % 2 else text_rows[0] for r in range(2 * U)]
        launch, ev = eng._launch_prefill, (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

        def timed_prefill(p):                     # a device event in front of the prefill (the wrapper of tools/prefill_time.py) ...
            ev[0].record()
            launch(p)

        eng._launch_prefill = timed_prefill
        n_prefilled = eng.start(rows_in, [cated] * U, [dataclasses.replace(kn, seed=2024 + u) for u in range(U)], noise=None)
        ev[1].record()                            # ... and one behind everything the admission enqueued after it (a sharing engine's tail-page copies)
        torch.cuda.synchronize()
        res[name].setdefault("prefill_ms", []).append(ev[0].elapsed_time(ev[1]))
        res[name]["prefill_rows"] = n_prefilled
        eng.decode(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode(a.steps)
        torch.cuda.synchronize()
        ms = 1000 * (time.perf_counter() - t0) / a.steps
        n_done = int(eng.states()[0].n_steps)
        tok = eng.generated[0, :n_done].cpu().numpy().copy()
        r = res[name]
        for counter, _ in COUNTERS:
            r[counter] = getattr(eng, counter + "_launches_per_step")
        r["pairing"] = eng.pairing
        r["pages"] = eng.pages.n_pages - eng.pages.n_free
        lp = eng.logprobs(0, n_done) if logp_of[name] else np.full((0, 4), np.nan)
        r["logp"] = f"{int((~np.isnan(lp)).sum())} of {lp.size} finite, mean {np.nanmean(lp) if lp.size else float('nan'):.4f}"
        r["ms"].append(ms)
        r["gemv"].append(eng.time_category("gemv", 50)[0])
        r["attn"].append(eng.time_category("attn", 50)[0])
        us_s, n_s = eng.time_category("sample", 20)
        r["sample"].append(us_s)
        r.setdefault("launches", {"gemv": eng.time_category("gemv", 1)[1], "attn": eng.time_category("attn", 1)[1], "sample": n_s})
        if r["tok"] is None:
            r["tok"] = tok
        del eng, launch, timed_prefill
        gc.collect()                              # (the timed-prefill wrapper and the engine refer to each other) the pairing slot goes back now
        torch.cuda.empty_cache()

base = variants[0][0]
print(f"# {a.steps} timed steps after {a.warmup} (context {L + T0 + a.warmup} .. {L + T0 + total}), {a.reps} alternating rounds; "
      f"ms per step (wall), codec-tokens/s at the median, us per launch (graph-chained)")
for name, knobs in variants:
    r = res[name]
    same = "" if r["tok"] is None or res[base]["tok"] is None else f"  tokens == {base}: {bool(np.array_equal(r['tok'], res[base]['tok']))}"
    twin = next(n for n, _ in variants if (dtype_of[n], kv_of[n], utts_of[n]) == (dtype_of[name], kv_of[name], utts_of[name]))   # the first arm on the same weights and cache
    if twin not in (name, base) and r["tok"] is not None:
        same += f"  tokens == {twin}: {bool(np.array_equal(r['tok'], res[twin]['tok']))}"
    U = utts_of[name]
    print(f"{name:14s} {U:2d} utts x CFG = {2 * U:2d} rows  tok/s {4 * U / (statistics.median(r['ms']) * 1e-3):9.1f}  "
          f"ms/step min {min(r['ms']):.4f} med {statistics.median(r['ms']):.4f}  all {' '.join(f'{v:.4f}' for v in r['ms'])} | "
          f"gemv {min(r['gemv']):.3f} x {r['launches']['gemv']} attn {min(r['attn']):.3f} x {r['launches']['attn']} "
          f"sample {min(r['sample']):.3f} x {r['launches']['sample']} us{same}   [{dtype_of[name]}, kv {kv_of[name]}, {' + '.join(f'{r[st.name]} {st.name}' for st in W16_STREAMS)} + {r['w8']} w8 + {r['wt8']} wt8 + {r['w16_pair']} w16 pair + {r['w8_pair']} w8 pair + {r['pair4']} pair4 + {r['pair4_pk']} pair4 pk + {r['kv16']} kv16 + {r['group']} group launches; kv16_small={int(small_of[name])}; logprobs={int(logp_of[name])} ({r['logp']}); first fill {r['prefill_rows']} rows in {min(r['prefill_ms']):.2f} ms, {r['pages']} KV pages in use; share_prompt={share_of[name]}; pairing={r['pairing']}; {' '.join(f'{k}={v}' for k, v in knobs.items()) or 'defaults'}]")
