"""What does the prefill cost, and what do bf16-valued weights change about it? Three arms of the 830M shape in ONE process, alternating
round by round, GPU time from device events around the `ssrhip_lm_prefill` call of `DecodeEngine.start()` (`DecodeEngine._launch_prefill`):

    fp32      an fp32 arena: three planes of the exact split, six products per k block (csrc/gemm_split.hip)
    bf16x3    a weight_dtype="bf16" arena with the same three planes (two of them zeros)
    bf16x1    the same arena with ONE plane per matrix (ssrhip_gemm_w1, DESIGN I.13)

for the bench prompt (1 utterance with CFG: 598 prompt rows) and for the prompt set of a 16-row engine (8 such utterances: 4,784 rows).
Then, with --gemm, the four layer GEMMs of both row counts launch by launch (three planes against one, alternating), each next to its
floor: the larger of 2 M N K x products / 2.5 PFLOP/s (dense bf16 peak) and (A + W planes + C) bytes / 8 TB/s. Prints a table and one JSON line.

--gemm-only skips the engines (under `SSRHIP_GEMM_SPLIT_DMA=0` it times the 4-wave kernels, three planes against one).

    python tools/prefill_time.py [--rounds 7] [--gemm | --gemm-only] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import _lib, layout as LY, weights as W  # noqa: E402
from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena  # noqa: E402

PEAK_BF16, HBM = 2.5e15, 8.0e12
ARMS = (("fp32", "fp32", 3), ("bf16x3", "bf16", 3), ("bf16x1", "bf16", 1))


def time_prefills(eng):
    """device events around every prefill of `eng`: wraps DecodeEngine._launch_prefill, the one place a prefill is enqueued from.
    Returns the list the milliseconds are appended to."""
    ms, launch = [], eng._launch_prefill

    def timed(p):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(p)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))

    eng._launch_prefill = timed
    return ms


def prompts(args, n_utt):
    g = torch.Generator().manual_seed(2024)
    L, N = 130, 160
    rows, cols, knobs = [], [], []
    for u in range(n_utt):
        x = torch.randint(0, 100, (1, L), generator=g)
        y = torch.randint(0, 2048, (1, N, 4), generator=g)
        unc = torch.randint(0, 101, (1, L), generator=g)
        cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), np.asarray([[N, N]]), args)
        rows += [x[0].numpy(), unc[0].numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=40, top_p=0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, use_cfg=True, text_len=L,
                                 n_spans=num_task, seed=1 + u))
    return rows, cols, knobs


def spread(v):
    return max(v) - min(v)


def gemm_arm(lib, M, N, K, act, residual, reps=20, rounds=5):
    """per-launch us of one layer GEMM: ssrhip_gemm on three planes against ssrhip_gemm_w1 on one, alternating rounds of `reps` launches"""
    g = torch.Generator().manual_seed(N + K)
    A = torch.randn(M, K, generator=g).cuda()
    Wt = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).float().cuda()
    b = torch.randn(N, generator=g).cuda()
    out = torch.zeros(M, N, device="cuda")
    three = torch.empty(3 * Wt.numel(), dtype=torch.int16, device="cuda")
    _lib.check(lib.ssrhip_split_weights(Wt.data_ptr(), three.data_ptr(), Wt.numel(), _lib.stream_ptr()))
    one = Wt.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
    a = _lib.GemmArgs()
    a.A, a.W, a.bias, a.C = A.data_ptr(), Wt.data_ptr(), b.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act, a.residual = M, N, K, K, N, act, residual
    us = {3: [], 1: []}
    for r in range(rounds + 1):                                            # round 0 = warm-up
        for planes, buf, entry in ((3, three, lib.ssrhip_gemm), (1, one, lib.ssrhip_gemm_w1)):
            a.W_split = buf.data_ptr()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                assert entry(C.byref(a), _lib.stream_ptr()) == 0
            e1.record()
            e1.synchronize()
            if r:
                us[planes].append(1000 * e0.elapsed_time(e1) / reps)
    res = {}
    for planes in (3, 1):
        flops = 2.0 * M * N * K * (6 if planes == 3 else 3)
        byts = 4.0 * M * K + 2.0 * planes * N * K + 4.0 * M * N * (2 if residual else 1)
        t_mm, t_mem = 1e6 * flops / PEAK_BF16, 1e6 * byts / HBM
        res[planes] = dict(us=round(statistics.median(us[planes]), 2), spread=round(spread(us[planes]), 2), floor_us=round(max(t_mm, t_mem), 2),
                           bound="matrix pipe" if t_mm >= t_mem else "bytes")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--gemm", action="store_true")
    ap.add_argument("--gemm-only", action="store_true")
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    dev = torch.device("cuda")
    args = W.lm_args_830m()
    sd = W.lm_state_dict(args, seed=0, device=dev)
    res = dict(metric="prefill_830m_arms", rounds=o.rounds, arms={})
    arenas = {}
    for name, dtype, planes in (() if o.gemm_only else ARMS):
        base = torch.cuda.memory_allocated()
        arena = LMWeightsArena(args, sd, dev, weight_dtype=dtype)
        masters = torch.cuda.memory_allocated() - base
        arena.ensure_split_planes(planes=planes)
        arena.ensure_head_split_planes()
        arenas[name] = arena
        res["arms"][name] = dict(planes=arena.split_planes, plane_bytes=arena.split_plane_bytes(), master_bytes=masters)
    for n_utt in (() if o.gemm_only else (1, 8)):
        rows, cols, knobs = prompts(args, n_utt)
        engines, timed = {}, {}
        for name, _, _ in ARMS:
            eng = DecodeEngine(arenas[name], n_utt, True, 1024, 256, stream_w16=False, stream_wt16=False)
            timed[name] = time_prefills(eng)
            engines[name] = eng
        host = {name: [] for name in engines}
        for r in range(o.rounds + 2):                                      # two warm-up rounds
            for name, eng in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.start(rows, cols, knobs, noise=None)
                torch.cuda.synchronize()
                host[name].append(1000 * (time.perf_counter() - t0))
        n_rows = None
        for name, eng in engines.items():
            ms = timed[name][2:]
            n_rows = eng._prefill_ws["x"].shape[0]
            res["arms"][name][f"rows{2 * n_utt}"] = dict(prompt_rows=int(n_rows), prefill_ms_median=round(statistics.median(ms), 3),
                                                         prefill_ms_spread=round(spread(ms), 3), prefill_ms_all=[round(v, 3) for v in ms],
                                                         start_wall_ms_median=round(statistics.median(host[name][2:]), 3))
            eng.close()
        print(f"--- {2 * n_utt}-row engine, {n_rows} prompt rows, {o.rounds} rounds (median ms, spread = max - min)")
        for name in engines:
            d = res["arms"][name][f"rows{2 * n_utt}"]
            print(f"  {name:7s} prefill {d['prefill_ms_median']:8.3f} ms  (spread {d['prefill_ms_spread']:.3f})   start() wall {d['start_wall_ms_median']:8.3f} ms")
        del engines
    for name in res["arms"]:
        d = res["arms"][name]
        print(f"  {name:7s} planes {d['planes']}: split planes {d['plane_bytes'] / 2 ** 30:.3f} GiB beside {d['master_bytes'] / 2 ** 30:.3f} GiB of masters and tables")
    if o.gemm or o.gemm_only:
        lib = _lib.lib()
        D, Fd = args.d_model, 4 * args.d_model
        res["gemm"] = {}
        for M in (598, 4784):
            for tag, N, K, act, rs in (("qkv", 3 * D, D, 0, 0), ("out_proj", D, D, 0, 1), ("ffn1", Fd, D, _lib.ACT_RELU, 0), ("ffn2", D, Fd, 0, 1)):
                r = gemm_arm(lib, M, N, K, act, rs)
                res["gemm"][f"{tag}_M{M}"] = r
                print(f"  {tag:8s} M={M:5d} N={N:5d} K={K:5d}: three planes {r[3]['us']:8.2f} us (floor {r[3]['floor_us']:.2f}, {r[3]['bound']}), "
                      f"one plane {r[1]['us']:8.2f} us (floor {r[1]['floor_us']:.2f}, {r[1]['bound']}), spreads {r[3]['spread']:.2f} / {r[1]['spread']:.2f}")
    line = json.dumps(res)
    print(line)
    if o.out:
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
