"""What rounding the decode step's matrices to bf16, or quantising them to e4m3 (DESIGN.md Part I.18), does to the 830M model's outputs, with
the synthetic weights (no real checkpoint: this characterises the feature, it does not judge quality and sets no bar).
  * greedy decode of bench.py's config-2 input by an fp32 engine and an engine of each `--dtypes` arm side by side: maximum and mean
    |difference| of the post-edit logits per step, for as long as both have chosen the same tokens (the histories are then identical:
    teacher-forced by agreement), up to --steps; the step at which the tokens first differ, if they do, and how many of the --steps
    steps chose the same tokens as fp32 (behind the first difference the histories differ too);
  * `SSR_Speech.score` loss (summed and per token) / top-10 accuracy of every arm on tools/score_bench.py's batch.
The result has one entry per arm, under the arm's name.
    python tools/w16_rounding.py [--steps 20] [--utts 16] [--dtypes bf16,e4m3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import layout as LY  # noqa: E402
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena  # noqa: E402
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402
from bench import synth_inputs  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtypes", default="bf16,e4m3", help="the arms compared with fp32, comma separated")
    opt = ap.parse_args(argv)
    arms = tuple(d for d in opt.dtypes.split(",") if d)
    dev = torch.device("cuda", 0)
    args = W.lm_args_830m()
    sd = W.lm_state_dict(args, seed=0, device=dev)
    x, y, unc = synth_inputs(args, 0)
    L, N = x.shape[1], y.shape[1]
    cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), np.asarray([[N, N]]), args)
    kn = DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, use_cfg=True, text_len=L,
                     n_spans=num_task, seed=2024)
    trace = {}
    for dt in ("fp32",) + arms:
        arena = LMWeightsArena(args, sd, dev, weight_dtype=dt)
        eng = DecodeEngine(arena, 1, True, 1024, 256, debug_logits=True)
        eng.start([x[0].numpy(), unc[0].numpy()], [cated], [kn])
        lg = []
        for _ in range(opt.steps):
            eng.decode(1)
            torch.cuda.synchronize()
            lg.append(eng.dbg_logits[0, :, :int(args.audio_vocab_size)].cpu().clone())     # the codec ids (special-token edits are +-inf / constants)
        trace[dt] = (torch.stack(lg), eng.tokens(0, opt.steps))
        eng.close()
        del eng, arena
        torch.cuda.empty_cache()
    l32, t32 = trace["fp32"]
    out = dict(tool="tools/w16_rounding.py", steps=opt.steps)
    for dt in arms:
        l16, t16 = trace[dt]
        agree = 0
        while agree < opt.steps and np.array_equal(t32[agree], t16[agree]):
            agree += 1
        n_cmp = min(agree + 1, opt.steps)                        # the step of the first disagreement still saw the same history
        fin = torch.isfinite(l32[:n_cmp]) & torch.isfinite(l16[:n_cmp])
        d = (l32[:n_cmp] - l16[:n_cmp]).abs()[fin]
        out[dt] = dict(steps_with_identical_history=n_cmp, first_token_difference_at_step=(agree if agree < opt.steps else None),
                       steps_with_the_tokens_of_fp32=sum(bool(np.array_equal(t32[s], t16[s])) for s in range(opt.steps)),
                       logit_abs_diff_max=float(d.max()), logit_abs_diff_mean=float(d.mean()), logit_abs_mean=float(l32[:n_cmp][fin].abs().mean()))
    from score_bench import make_batch  # noqa: E402
    m = SSR_Speech(args)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    del sd
    m = m.to(dev).eval()
    batch = make_batch(m.args, opt.utts)
    for dt in ("fp32",) + arms:
        m.set_weight_dtype(dt)
        r = m.score(batch)
        out[f"score_{dt}"] = dict(loss=float(r["loss"]), loss_per_token=float(r["loss"]) / float(r["effective_ntoken"]), top10acc=float(r["top10acc"]),
                                  ntoken=float(r["effective_ntoken"]))
    line = json.dumps(out)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
