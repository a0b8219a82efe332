"""The bf16-rounded codec's A/B (DESIGN.md Parts I.30, I.31 and I.32): five models of the full-size wmencodec (synthetic weights) in ONE process,
in alternating rounds, median and spread (max - min) over the rounds:

    F   weight_dtype="fp32"                          three planes of the fp32 weights, six products per k block
    B   weight_dtype="bf16", SSRHIP_CODEC_W1=0       three planes of the rounded weights (same kernels as F)
    A0  weight_dtype="bf16", SSRHIP_LSTM_W1=0        one plane in the GEMMs and residual blocks, three planes of W_hh in the LSTM step
    A   weight_dtype="bf16", SSRHIP_LSTM_W1=1        ... and one plane of W_hh in the LSTM step (the same bits as A0 and B, checked here)
    A8  the model A with SSRHIP_LSTM_W1_DEPTH=8 in the environment while it runs: eight k-steps in flight in the one-plane LSTM step
    R   the model A built with act_dtype="bf16": activation operands rounded to bf16, one product per k block (OTHER bits than A: reported)

Workloads: `encode` / `decode` / `wmdecode(with_mark=False)` of B clips x seconds (config 5's shape is 256x30; on an out-of-memory error the
batch is halved), and a per-launch table — the GEMM shapes VERDICT r6 names and the residual blocks at 64 / 128 channels, three-plane
against one-plane entry against bf16-activation entry on the same rounded matrix, us and fp32-equivalent TFLOP/s next to the matrix
ceiling (2,500 / 6 for six products, 2,500 / 3 for three, 2,500 for one).

Usage: python tools/codec_w1_ab.py [--workloads 256x30,8x10] [--rounds 4] [--launches 1] [--out profiles/codec_w1_ab.md]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import _lib  # noqa: E402
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.codec.wmencodec import WMEncodecModel  # noqa: E402

PEAK = 2500.0                 # dense bf16 matrix TFLOP/s of one MI355X
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def build_arms():
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=0)
    assert "SSRHIP_CODEC_W1" not in os.environ, "the arms set the switch themselves"
    arms = {"F": WMEncodecModel(cfg, sd, "cuda", weight_dtype="fp32")}
    os.environ["SSRHIP_CODEC_W1"] = "0"
    try:
        arms["B"] = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
    finally:
        del os.environ["SSRHIP_CODEC_W1"]
    assert "SSRHIP_LSTM_W1" not in os.environ and "SSRHIP_LSTM_W1_DEPTH" not in os.environ, "the arms set the switches themselves"
    for name, knob in (("A0", "0"), ("A", "1")):
        os.environ["SSRHIP_LSTM_W1"] = knob
        try:
            arms[name] = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16")
        finally:
            del os.environ["SSRHIP_LSTM_W1"]
    arms["A8"] = arms["A"]                                           # the same model; `ARM_ENV` holds what differs while it runs
    arms["R"] = WMEncodecModel(cfg, sd, "cuda", weight_dtype="bf16", act_dtype="bf16")
    assert arms["R"].bf16_acts and arms["R"].lstm_one_plane and not arms["A"].bf16_acts
    assert arms["A"].one_plane and arms["A0"].one_plane and not arms["B"].one_plane
    assert arms["A"].lstm_one_plane and not arms["A0"].lstm_one_plane
    return cfg, arms


ARM_ENV = {"A8": {"SSRHIP_LSTM_W1_DEPTH": "8"}}                      # read by the library at every ssrhip_lstm_layer_w1 call
ORDER = ("F", "B", "A0", "A", "A8", "R")


def run_arm(name, fn, m):
    env = ARM_ENV.get(name, {})
    os.environ.update(env)
    try:
        return fn(m)
    finally:
        for k in env:
            del os.environ[k]


def plane_bytes(m):
    return sum(t.numel() * t.element_size() for v in m._plane_cache.values() for t in (v if isinstance(v, tuple) else (v,)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def workload(cfg, arms, B, secs, rounds):
    g = torch.Generator().manual_seed(0)
    wav = (torch.randn(B, 1, int(secs * cfg.sample_rate), generator=g) * 0.1).cuda()
    codes = arms["F"].encode(wav)[0].clone()                         # every arm decodes the SAME codes
    Tf = codes.shape[-1]
    marks = torch.zeros(B, Tf, dtype=torch.long, device="cuda")
    marks[:, Tf // 2:] = 1
    entries = {"encode": lambda m: m.encode(wav)[0], "decode": lambda m: m.decode(codes),
               "wmdecode": lambda m: m.wmdecode(codes, marks, wav[..., : Tf * cfg.hop], with_mark=False)[0]}
    got = {}
    L = _lib.lib()
    steps, a1 = {}, {}
    for name, m in arms.items():                                     # untimed: sizing passes, the allocator holds the blocks
        n0, r0 = L.ssrhip_lstm_w1_launches(), L.ssrhip_codec_a1_launches()
        got[name] = {e: run_arm(name, fn, m).clone() for e, fn in entries.items()}
        steps[name], a1[name] = L.ssrhip_lstm_w1_launches() - n0, L.ssrhip_codec_a1_launches() - r0
    same = all(torch.equal(got[n][e], got["B"][e]) for e in entries for n in ("A0", "A", "A8"))
    say(f"### {B} x {secs:g} s  ({Tf} frames per clip; A0 == A == A8 == B bit for bit on all three entries: {same})")
    say(f"  one-plane LSTM step launches in the untimed pass: " + ", ".join(f"{n} {steps[n]}" for n in ORDER))
    for e in ("decode", "wmdecode"):
        a, f = got["A"][e].double(), got["F"][e].double()
        say(f"  {e}: relative rms difference A vs F = {float((a - f).pow(2).mean().sqrt() / f.pow(2).mean().sqrt()):.4e}")
    say(f"  encode: {float((got['A']['encode'] != got['F']['encode']).double().mean()) * 100:.2f} % of the RVQ codes differ between A and F")
    say(f"  bf16-activation launches in the untimed pass: " + ", ".join(f"{n} {a1[n]}" for n in ORDER))
    for e in ("decode", "wmdecode"):
        r, a = got["R"][e].double(), got["A"][e].double()
        say(f"  {e}: relative rms difference R vs A = {float((r - a).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()):.4e}")
    say(f"  encode: {float((got['R']['encode'] != got['A']['encode']).double().mean()) * 100:.2f} % of the RVQ codes differ between R and A")
    del got
    ms = {n: {e: [] for e in entries} for n in arms}
    for r in range(rounds):
        for name in (ORDER if r % 2 == 0 else ORDER[::-1]):
            for e, fn in entries.items():
                t, out = timed(lambda: run_arm(name, fn, arms[name]))
                ms[name][e].append(t)
                del out
    say("| entry | F fp32 ms (spread) | B bf16 x3 ms (spread) | A0 bf16 x1, LSTM x3 ms (spread) | A bf16 x1 ms (spread) | A8 ms (spread) | R bf16 acts ms (spread) | A0 / B | A / A0 | A8 / A0 | A / F | R / A |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for e in entries:
        med = {n: statistics.median(ms[n][e]) for n in arms}
        sp = {n: max(ms[n][e]) - min(ms[n][e]) for n in arms}
        say(f"| {e} | " + " | ".join(f"{med[n]:.2f} ({sp[n]:.2f})" for n in ORDER) +
            f" | {med['A0'] / med['B']:.3f} | {med['A'] / med['A0']:.3f} | {med['A8'] / med['A0']:.3f} | {med['A'] / med['F']:.3f} | {med['R'] / med['A']:.3f} |")
        # the gate of DESIGN.md Part I.32 (I.11's rule): R below A by more than A's spread and by at least 1 %
        gap = med["A"] - med["R"]
        say(f"  gate {e}: A - R = {gap:.2f} ms ({gap / med['A'] * 100:.1f} %) against A's spread {sp['A']:.2f} ms -> "
            f"{'met' if gap > sp['A'] and gap >= 0.01 * med['A'] else ('LOSES' if -gap > sp['A'] else 'no difference')}")
        for n in ("A", "A8"):                                        # the gate of DESIGN.md Part I.31: below A0 by more than the larger spread
            gap, noise = med["A0"] - med[n], max(sp["A0"], sp[n])
            say(f"  gate {e}: A0 - {n} = {gap:.2f} ms against the larger spread {noise:.2f} ms -> {'met' if gap > noise else ('no difference' if abs(gap) <= noise else 'LOSES')}")
    say(f"  rounds = {rounds}, arms alternate {' '.join(ORDER)} / reversed; mallocs_in_flight A = {arms['A'].mallocs_in_flight}, A0 = {arms['A0'].mallocs_in_flight}")
    say()


def event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def gemm_launch(L, M, N, K, batch, act_in, tm_c=0, rounds=4, reps=5):
    g = torch.Generator().manual_seed(M + N + K)
    Wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).float().cuda()
    A = torch.randn(1, M, K, generator=g).cuda().expand(batch, M, K).contiguous()
    out = torch.empty(batch, M, N, device="cuda")
    three = torch.empty(3 * Wt.numel(), dtype=torch.int16, device="cuda")
    _lib.check(L.ssrhip_split_weights(Wt.data_ptr(), three.data_ptr(), Wt.numel(), _lib.stream_ptr()))
    one = Wt.to(torch.bfloat16).contiguous()
    a = _lib.GemmArgs()
    a.A, a.W, a.C = A.data_ptr(), Wt.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldc, a.act_in = M, N, K, K, N, act_in
    a.batch, a.strideA, a.strideC = batch, M * K, M * N
    if tm_c:
        a.tm_c, a.tm_lo, a.tm_hi = tm_c, 0, M * (N // tm_c)

    def run(entry, planes):
        a.W_split = planes.data_ptr()
        _lib.check(entry(C.byref(a), _lib.stream_ptr()))

    entry = {"x3": (L.ssrhip_gemm, three), "x1": (L.ssrhip_codec_gemm_w1, one), "a1": (L.ssrhip_codec_gemm_a1, one)}
    us = {k: [] for k in entry}
    for r in range(rounds):
        for arm in (tuple(entry) if r % 2 == 0 else tuple(entry)[::-1]):
            us[arm].append(event_us(lambda: run(*entry[arm]), reps))
    flop = 2.0 * M * N * K * batch
    return us, flop


def resblock_launch(L, Cc, T, B, rounds=4, reps=5):
    g = torch.Generator().manual_seed(Cc)
    Hh = Cc // 2
    x = torch.randn(1, T + 2, Cc, generator=g).cuda().expand(B, T + 2, Cc).contiguous()
    w3 = (torch.randn(Hh, 3 * Cc, generator=g) / math.sqrt(3 * Cc)).to(torch.bfloat16).float().cuda()
    w1 = (torch.randn(Cc, Hh, generator=g) / math.sqrt(Hh)).to(torch.bfloat16).float().cuda()
    b3, b1 = torch.zeros(Hh, device="cuda"), torch.zeros(Cc, device="cuda")
    kp = torch.arange(Hh, device="cuda")
    perm = 16 * (kp // 16) + (kp % 8) % 4 + 8 * ((kp % 8) // 4) + 4 * ((kp // 8) % 2)
    w1p = w1[:, perm].contiguous()
    p3 = torch.empty(3, Hh, 3 * Cc, dtype=torch.int16, device="cuda")
    p1 = torch.empty(3, Cc, Hh, dtype=torch.int16, device="cuda")
    _lib.check(L.ssrhip_split_weights(w3.data_ptr(), p3.data_ptr(), w3.numel(), _lib.stream_ptr()))
    _lib.check(L.ssrhip_split_weights(w1p.data_ptr(), p1.data_ptr(), w1p.numel(), _lib.stream_ptr()))
    o3, o1 = w3.to(torch.bfloat16).contiguous(), w1p.to(torch.bfloat16).contiguous()
    y = torch.empty(B, T, Cc, device="cuda")
    a = _lib.ResblockArgs()
    a.x, a.y, a.w3, a.b3, a.w1, a.b1 = x.data_ptr(), y.data_ptr(), w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), b1.data_ptr()
    a.B, a.T, a.C, a.x_bstride, a.y_bstride = B, T, Cc, (T + 2) * Cc, T * Cc

    def run(entry, planes):
        a.w3_split, a.w1_split = planes[0].data_ptr(), planes[1].data_ptr()
        _lib.check(entry(C.byref(a), _lib.stream_ptr()))

    entry = {"x3": (L.ssrhip_resblock, (p3, p1)), "x1": (L.ssrhip_resblock_w1, (o3, o1)), "a1": (L.ssrhip_resblock_a1, (o3, o1))}
    us = {k: [] for k in entry}
    for r in range(rounds):
        for arm in (tuple(entry) if r % 2 == 0 else tuple(entry)[::-1]):
            us[arm].append(event_us(lambda: run(*entry[arm]), reps))
    flop = 2.0 * B * T * (Hh * 3 * Cc + Cc * Hh)
    return us, flop


def launch_table(B):
    L = _lib.lib()
    ELU = _lib.ACT_ELU
    say(f"### per launch, batch {B} (three-plane entry on the rounded matrix = what arms F and B launch; one-plane entry = arm A; bf16-activation entry = arm R)")
    say(f"ring of the residual-block kernels: SSRHIP_RESBLOCK_RING={os.environ.get('SSRHIP_RESBLOCK_RING', 'unset (three planes: 2, one plane: 4)')}")
    say(f"| launch | x3 us (spread) | x3 TFLOP/s (of {PEAK / 6:.0f}) | x1 us (spread) | x1 TFLOP/s (of {PEAK / 3:.0f}) | x1 / x3 | a1 us (spread) | a1 TFLOP/s (of {PEAK:.0f}) | a1 / x1 |")
    say("|---|---|---|---|---|---|---|---|---|")

    def row(name, us, flop):
        m3, m1, ma = (statistics.median(us[k]) for k in ("x3", "x1", "a1"))
        sp = {k: max(us[k]) - min(us[k]) for k in us}
        say(f"| {name} | {m3:.0f} ({sp['x3']:.0f}) | {flop / m3 / 1e6:.0f} | {m1:.0f} ({sp['x1']:.0f}) | {flop / m1 / 1e6:.0f} | {m1 / m3:.3f} | "
            f"{ma:.0f} ({sp['a1']:.0f}) | {flop / ma / 1e6:.0f} | {ma / m1:.3f} |")

    # M x N x K: the decoder's transposed convolutions (ELU on load, time mask) and the encoder's strided ones at config 5's lengths
    shapes = [("12001x1280x1024 convtr s5", 12001, 1280, 1024, ELU, 256), ("1501x8192x2048 convtr s8", 1501, 8192, 2048, ELU, 1024),
              ("1500x1024x8192 conv s8", 1500, 1024, 8192, ELU, 0), ("12000x512x2560 conv s5", 12000, 512, 2560, ELU, 0),
              ("60001x512x512 convtr s4", 60001, 512, 512, ELU, 128), ("1500x2048x512 lstm in", 1500, 2048, 512, 0, 0)]
    for name, M, N, K, act_in, tm_c in shapes:
        row(f"gemm {name} x{B}", *gemm_launch(L, M, N, K, B, act_in, tm_c))
    for Cc, T in ((64, 480000), (128, 240000)):
        row(f"resblock C={Cc} T={T} x{B}", *resblock_launch(L, Cc, T, B))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="256x30,8x10")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=1, help="0: skip the per-launch table")
    ap.add_argument("--launch_batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    say(f"# codec_w1_ab: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say()
    if opt.workloads:
        cfg, arms = build_arms()
        say(f"plane bytes: F {plane_bytes(arms['F']) / 2**20:.1f} MiB, B {plane_bytes(arms['B']) / 2**20:.1f} MiB, A0 {plane_bytes(arms['A0']) / 2**20:.1f} MiB, "
            f"A {plane_bytes(arms['A']) / 2**20:.1f} MiB (W_hh packs are not in the plane cache: a third as large in A as in A0)")
        say()
        for wl in opt.workloads.split(","):
            B, secs = int(wl.split("x")[0]), float(wl.split("x")[1])
            while True:
                try:
                    workload(cfg, arms, B, secs, opt.rounds)
                    break
                except torch.cuda.OutOfMemoryError:
                    say(f"{B} x {secs:g} s does not fit: halving the batch")
                    torch.cuda.empty_cache()
                    B //= 2
        del arms
        torch.cuda.empty_cache()
    if opt.launches:
        launch_table(opt.launch_batch)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
