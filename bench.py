"""bench.py — AR-decode throughput of the HIP engine on the BASELINE.json configuration
"English 830M zero-shot TTS, cfg_stride=5 top-k sampling, batch=1 on one MI355X" (configs[1]).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

`--dump-outputs DIR` writes what the K timed steps computed (`dump_outputs`) as DIR/<name>.npy; the inputs depend on the
arguments only, so the files of two builds can be compared array for array.

A "step" is one decode step of the hot path (one codec frame = 4 codec tokens per utterance) over one
batch of synthetic input: 830M-shape weights from the deterministic generator (seed 0, fp32), L=130 random
phoneme ids, a 160-frame random prompt, CFG doubling (2 rows), top_k=40/top_p=0.8 sampling. Inputs and
weights are resident in HBM before the timed region. One utterance per GPU (weak scaling: rank r decodes
utterance r with seed+r, no data-path collective during decode).

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, `--dump-outputs`, and ONE JSON line
(rank 0) with `metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` and the workload's description.

`--full` adds, on the same line, everything else the benchmark measures and checks (never `value`): four more passes of the same
W + K steps (`ms_per_step_passes`), the same workload around context 700 (`ctx700`), `roofline` (dominant kernel = the
weight-streaming GEMV, HBM-bound, from per-kernel timing passes of its own), with N > 1 the ONE all_gather of the generated
tokens (`allgather_ms`, timed separately), `cpu_baseline` (the oracle = CPU restatement of the reference, timed on the host's
cores, bounded sample) and the extra legs below. `--no-ctx700`, `--no-extras`, `--legs` and `--no-cpu-baseline` trim what
`--full` adds.

Extras of `--full` (never `value`):
  rtf_10s_tts  wav -> wav through the public API (`inference_one_sample`: codec encode of the prompt wav, prefill, sampled AR
               decode with the host-side torch RNG stream, wmencodec decode), ~10 s generated; + time to the first 16 frames.
  dp64         BASELINE config 4: 64 utterances (L=67, 150-frame prompts, seeds 1000+i / 2000+i, greedy) through `dp.generate`
               (shard -> lock-step decode of 8 utterances x CFG per engine pass -> ONE all-gather), tokens/s/GPU + checksum.
  codec256     BASELINE config 5: wmencodec encode + decode of 256 clips x 30 s, 256/N clips per rank.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # multi-process RCCL on this driver needs dmabuf IPC (before HIP starts)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec peak
# HBM bytes moved by the GEMV launches of ONE step, from the PMC counters (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this
# command, gfx950 corrections of MI355X_MICROARCH.md: FETCH_SIZE x2 for wide coalesced reads). `traffic` in the JSON line is this figure
# divided by the step's number of GEMV launches (the paired launches of the 2-row step move the bytes of the two launches they replace).
# Not re-measured live (counters need rocprofv3): the constants are this round's profiles, named in `traffic_source`.
#   2 rows : round 5, final build: 118.57 x15 (FFN2 | QKV) + 101.75 (FFN2 | head-MLP1) + 85.31 x16 (out-proj | FFN1) + 50.65 (QKV of layer 0)
#             + 34.09 (head-MLP2) = 3,330.0 MB read + 4.6 MB written per step; algorithmic 3,290.2 MB: ratio 1.0135
#   16 rows: (59.30 x33 + 71.66 x16 + 18.17 x16 + 36.04) = 3,432 MB read + 20 MB written (x re-read through L2 by the streamed-x kernel; round 2)
TRAFFIC_BYTES_PER_STEP_GEMVS = {2: 3334.6e6, 16: 66 * 52.3e6}
TRAFFIC_SOURCE = {2: "profiles/r06_pmc_fetch_size.md + profiles/r06_pmc_write_size.md (3,330.0 MB read + 4.6 MB written by the 34 GEMV launches of a step; the same as round 5's passes)",
                  16: "profiles/r02_pmc_fetch_size_16rows.md + profiles/r02_pmc_write_size_16rows.md"}


DEMO_PROMPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "demo_5895_34622_000026_000002_160f.wav")


def demo_prompt_codes(dev):
    """Prompt of BASELINE configs 1-2: the first 160 frames (3.2 s) of the reference's demo/5895_34622_000026_000002.wav (a data fixture,
    oracle/make_golden_demo.py), tokenised by wmencodec with the bench's synthetic codec weights -> int64 [1, 160, 4] on the CPU; None if
    the fixture is not there (then the prompt codes are random, as before round 6). Untimed set-up."""
    if not os.path.exists(DEMO_PROMPT) or os.environ.get("BENCH_RANDOM_PROMPT", "0") not in ("", "0"):
        return None
    from ssr_speech_amd import weights as W
    from ssr_speech_amd.data.tokenizer import AudioTokenizer, tokenize_audio
    ccfg = W.codec_config_full()
    tok = AudioTokenizer(device=dev, config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=0))
    codes, _, _ = tokenize_audio(tok, DEMO_PROMPT)
    y = codes.transpose(2, 1).cpu().contiguous()
    assert tuple(y.shape) == (1, 160, 4), y.shape
    del tok            # (no empty_cache here: unmapping memory under `rocprofv3 --pmc` crashed the profiler's collector thread, round 6)
    return y


def synth_inputs(args_lm, rank, L=130, N=160, prompt_codes=None):
    g = torch.Generator().manual_seed(2024 + rank)
    x = torch.randint(0, 100, (1, L), generator=g)
    y = torch.randint(0, 2048, (1, N, 4), generator=g)
    unc = torch.randint(0, 101, (1, L), generator=g)
    if prompt_codes is not None and prompt_codes.shape[1] == N:
        y = prompt_codes.clone()                 # same draws from `g` either way: the text ids do not depend on the prompt's source
    return x, y, unc


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, eng, warmup, steps):
    """`--dump-outputs`: what the timed decode steps handed back, as `out_dir/<name>.npy` (float64 / float32), for comparing two
    builds output for output. tokens [U, steps, K]: the codec tokens of the timed steps; logits_last_step [2U, K, card]: the
    logits buffer after the last timed step; sampler_state [U, 12]: the per-utterance state (`_lib.SamplerState`, pad excluded).
    Untimed; called right after the timed pass, before anything else advances the engine."""
    total = warmup + steps
    tokens = np.stack([eng.tokens(u, total)[warmup:] for u in range(eng.n_utt)])
    states = eng.states()
    fields = [f for f, _ in states[0]._fields_ if f not in ("span_end", "pad")]
    state = np.asarray([[getattr(s, f) for f in fields] + list(s.span_end) for s in states], dtype=np.float64)
    arrays = {"tokens": tokens.astype(np.float64), "logits_last_step": eng.logits.detach().float().cpu().numpy(),
              "sampler_state": state}
    assert tokens.shape[1] == steps, (tokens.shape, steps)
    assert sum(v.nbytes for v in arrays.values()) <= DUMP_LIMIT_BYTES
    os.makedirs(out_dir, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)
    return {name: list(arr.shape) for name, arr in arrays.items()}


def cpu_baseline(args_lm, sd_gpu, x, y, unc, n_steps=25):
    """Oracle (port of the reference's CPU path) on this box's host cores; returns codec-tokens/s."""
    from oracle import lm as O
    ncpu = os.cpu_count() or 1
    # Thread count: the decode step is a memory-bound B=2 GEMV; torch with one thread per logical core of a
    # 256-thread host is pathological (measured 22 s/step), so a few counts are probed on consecutive blocks of
    # steps of the SAME run and the >= 25 measured steps then run at the fastest one (that favours the CPU).
    trial_threads = [t for t in (16, 32, 64) if t <= ncpu] or [ncpu]
    probe = 4                       # steps per thread count in the probe phase (the first after a switch is dropped)
    measured = max(int(n_steps), 25)  # >= 25 decode steps at ONE setting — the fastest of the probe
    n_probe = 2 + probe * len(trial_threads)
    total = n_probe + 1 + measured
    torch.set_num_threads(trial_threads[0])
    sd = O.reference_params({k: v.cpu() for k, v in sd_gpu.items()})
    marks = []
    chosen = {}

    class Clock(dict):          # the oracle touches trace["samples"] once per finished step
        def setdefault(self, k, d=None):
            if k == "samples":
                marks.append(time.perf_counter())
                done = len(marks)
                if done >= 2 and done < n_probe and (done - 2) % probe == 0:
                    torch.set_num_threads(trial_threads[(done - 2) // probe])
                if done == n_probe:                                  # probe finished: the rest of the run at the fastest count
                    dts_ = np.diff(np.asarray(marks))
                    per_ = {th: float(dts_[1 + i * probe + 1: 1 + (i + 1) * probe].mean()) for i, th in enumerate(trial_threads)}
                    chosen.update(per_)
                    torch.set_num_threads(min(per_, key=per_.get))
            return dict.setdefault(self, k, d)

    trace = Clock()
    mi = torch.LongTensor([[[y.shape[1], y.shape[1]]]])
    t0 = time.perf_counter()
    O.inference(sd, args_lm, x, y, mi, uncond_x=unc, max_steps=total, trace=trace, top_k=40, top_p=0.8, temperature=1.0,
                stop_repetition=2, kvcache=1, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    prefill_s = marks[0] - t0
    dts = np.diff(np.asarray(marks))
    best = min(chosen, key=chosen.get)
    steady = dts[n_probe: n_probe + measured]                        # the step right after the switch is dropped
    ms_step = float(steady.mean())
    return dict(value=round(4.0 / ms_step, 2), unit="codec-tokens/s", cores=best, kind="port",
                sample=f"oracle/lm.py (CPU restatement of models/ssr.py inference, op-for-op incl. per-step KV torch.cat), same 830M weights/inputs: "
                       f"prefill S0={x.shape[1] + y.shape[1] + 10} x2 rows ({prefill_s:.2f} s, {trial_threads[0]} threads), a probe of {probe} steps per thread count "
                       f"(ms/step {{{', '.join(f'{k}: {1000 * v:.1f}' for k, v in chosen.items())}}} on a {ncpu}-logical-core host), then {len(steady)} decode steps "
                       f"at the fastest count ({best} threads): {1000 * ms_step:.1f} ms/step")


def codec_leg(dev, with_cpu):
    """Extra (not `value`): wmencodec encode + decode throughput at the full SEANet config (SURVEY §8 rows B1-B7, config 5
    shape scaled to 16 clips x 10 s so that the default run stays short), and the oracle's CPU time on 4 clips x 30 s
    with the GPU's codes / waveform on the same clips beside it."""
    from ssr_speech_amd import weights as W
    from ssr_speech_amd.codec.wmencodec import WMEncodecModel
    cfg = W.codec_config_full()
    csd = W.codec_state_dict(cfg, seed=0)
    m = WMEncodecModel(cfg, csd, dev)
    g = torch.Generator().manual_seed(0)
    B, secs = 16, 10.0
    wav = (torch.randn(B, 1, int(secs * 16000), generator=g) * 0.1).to(dev)
    codes, _, _ = m.encode(wav)
    m.decode(codes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codes, _, _ = m.encode(wav)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out_wav = m.decode(codes)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    GF = 6.97e9                                   # FLOP per audio-second, encode and decode each
    audio_s = B * secs
    out = {"workload": f"{B} clips x {secs:.0f} s, 16 kHz, full wmencodec config, synthetic weights",
           "encode_ms": round(1000 * (t1 - t0), 2), "decode_ms": round(1000 * (t2 - t1), 2),
           "encode_audio_s_per_s": round(audio_s / (t1 - t0), 1), "decode_audio_s_per_s": round(audio_s / (t2 - t1), 1),
           "encode_tflops": round(GF * audio_s / (t1 - t0) / 1e12, 1), "decode_tflops": round(GF * audio_s / (t2 - t1) / 1e12, 1),
           "mfma_fp32_peak_tflops": 157.3, "out_shape": list(out_wav.shape)}
    if with_cpu:
        # "codec: one 30 s clip x B=4 scaled linearly to B=256" — the oracle on 4 clips x 30 s, and the GPU on the SAME clips
        # so that the comparison in this record means something (round 4 compared a 2 s cut on the CPU with the GPU's 10 s clip: different
        # right context through the non-causal convolutions and the LSTM, hence a meaningless 3 % "mismatch").
        from oracle import codec as OC
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        g4 = torch.Generator().manual_seed(1)
        w4 = torch.randn(4, 1, 30 * 16000, generator=g4) * 0.1
        c0 = time.perf_counter()
        ccodes, _, _ = OC.encode(csd, w4, cfg)
        c1 = time.perf_counter()
        cwav = OC.decode(csd, ccodes, cfg)
        c2 = time.perf_counter()
        gcodes, _, _ = m.encode(w4.to(dev))
        gwav = m.decode(ccodes.to(dev))
        n_diff = int((gcodes.cpu() != ccodes).sum())
        out["cpu_baseline"] = {"kind": "port", "cores": torch.get_num_threads(), "sample": "oracle/codec.py on 4 clips x 30 s (BASELINE.md: scaled linearly to 256 clips)",
                               "encode_audio_s_per_s": round(120.0 / (c1 - c0), 2), "decode_audio_s_per_s": round(120.0 / (c2 - c1), 2),
                               "encode_ms_scaled_to_256_clips": round(1000 * (c1 - c0) * 64, 0), "decode_ms_scaled_to_256_clips": round(1000 * (c2 - c1) * 64, 0),
                               "gpu_codes_differing_on_the_same_clips": n_diff, "codes_compared": int(ccodes.numel()),
                               "gpu_max_abs_wav_diff_on_the_same_codes": float((gwav.cpu() - cwav).abs().max())}
    return out


class CharPhonemizer:
    """Stands in for espeak in the API leg: one 'phoneme' per character (the front-end is out of scope)."""

    def __call__(self, texts):
        return [[c for c in t if c != " "] for t in texts]


def build_api_model(args_lm, sd, dev):
    """`SSR_Speech` (the drop-in class) on the 830M-shape weights. The second head Linear's bias is pushed to -30 for the special
    ids (>= 2048) so that a random-weight LM emits only codec ids the RVQ decoder accepts (the reference would raise on them
    too); generation then ends by the reference's own length cap (`y_len > 10 * L`, ssr.py:739)."""
    from ssr_speech_amd.models.ssr import SSR_Speech
    sd2 = dict(sd)
    for k in range(args_lm.n_codebooks):
        b = sd[f"predict_layer.{k}.2.bias"].clone()
        b[int(args_lm.audio_vocab_size):] = -30.0
        sd2[f"predict_layer.{k}.2.bias"] = b
    m = SSR_Speech(args_lm)
    m.load_state_dict({k: v.cpu() for k, v in sd2.items()})
    return m.to(dev).eval()


def rtf_leg(model, args_lm, dev, tmpdir):
    """RTF of one ~10 s zero-shot TTS THROUGH THE API: `inference_one_sample(wav file -> wav)`, sampling mode (top_k=40,
    top_p=0.8, cfg_stride=5, CFG), seeded by `torch.manual_seed` like the reference's CLI. L=67 phonemes and a 160-frame
    (3.2 s) prompt give ~505 generated frames (10.1 s) under the length cap."""
    import argparse as ap_
    from ssr_speech_amd import weights as W
    from ssr_speech_amd.data.tokenizer import AudioTokenizer, write_wav
    from ssr_speech_amd.inference_scale import inference_one_sample
    ccfg = W.codec_config_full()
    tok = AudioTokenizer(device=dev, config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=0))
    g = torch.Generator().manual_seed(7)
    n_prompt = 160
    fn = os.path.join(tmpdir, "bench_prompt.wav")
    noise_prompt = torch.randn(1, n_prompt * 320, generator=g) * 0.1          # (drawn either way: the texts below keep their values)
    if os.path.exists(DEMO_PROMPT):
        fn = DEMO_PROMPT                            # the prompt BASELINE configs 1-2 name, first 160 frames
    else:
        write_wav(fn, noise_prompt, 16000)
    symbols = [chr(ord("a") + i) for i in range(26)] + [chr(ord("A") + i) for i in range(26)]
    phn2num = {c: i for i, c in enumerate(symbols)}
    prompt_text = "".join(symbols[int(i)] for i in torch.randint(0, 52, (20,), generator=g))
    target_text = prompt_text + " " + "".join(symbols[int(i)] for i in torch.randint(0, 52, (47,), generator=g))      # 67 phonemes
    decode_config = {"top_k": 40, "top_p": 0.8, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    mi = torch.LongTensor([[n_prompt, n_prompt]])
    margs = ap_.Namespace(**vars(args_lm))
    call = lambda: inference_one_sample(model, margs, phn2num, CharPhonemizer(), tok, fn, prompt_text, target_text, mi, 1.5, 5, True, False,
                                        False, True, dev, decode_config)
    torch.manual_seed(1)
    call()                                         # warm-up: engine + graph capture + codec buffers
    torch.cuda.synchronize()
    best = None
    for rep in range(2):
        torch.manual_seed(1 + rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lr = model.last_run
        rec = {"wall_ms": round(1000 * (t1 - t0), 2), "generated_s": round(wav.shape[-1] / 16000.0, 3), "steps": int(lr["steps"]),
               "rtf": round((t1 - t0) / (wav.shape[-1] / 16000.0), 4),
               "time_to_first_16_frames_ms": round(1000 * (lr["t_first_chunk"] - t0), 2),
               "lm_inference_ms": round(1000 * (lr["t_end"] - lr["t_start"]), 2)}
        if best is None or rec["rtf"] < best["rtf"]:
            best = rec
    best["prompt"] = "demo/5895_34622_000026_000002.wav, first 160 frames" if fn == DEMO_PROMPT else "randn x 0.1, 160 frames"
    best["note"] = ("inference_one_sample(wav -> wav): read wav, wmencodec encode of the 3.2 s prompt, prefill, sampled decode with the torch CPU RNG "
                    "stream drawn 16 steps ahead of the GPU, wmencodec decode of all frames; the prompt part is cut from the output (tts)")
    return best


def dp64_leg(model, args_lm, dev, world, rank, dist):
    """BASELINE config 4 end to end through `dp.synthesize`: shard -> lock-step decode (8 utterances x CFG per engine
    pass) -> all-gather of the tokens -> every rank renders the waveforms of its own shard in one ragged pass of the wmencodec decoder
    (the code path tests/test_dp_gloo.py and tests/test_gpu_ragged.py cover)."""
    from ssr_speech_amd import dp, weights as W
    from ssr_speech_amd.data.tokenizer import AudioTokenizer
    import zlib
    ccfg = W.codec_config_full()
    tok = AudioTokenizer(device=dev, config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=0))
    utts = []
    for i in range(64):
        gx = torch.Generator().manual_seed(1000 + i)
        gy = torch.Generator().manual_seed(2000 + i)
        utts.append({"x": torch.randint(0, 100, (1, 67), generator=gx), "y": torch.randint(0, 2048, (1, 150, 4), generator=gy),
                     "mask_interval": torch.LongTensor([[[150, 150]]])})
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    n_mine = len(dp.balanced_shards([dp.utterance_cost(67, 150)] * 64, world)[rank])
    if n_mine:         # untimed: the codec's kernels and allocator blocks for this shard's decode shape (the LM engine warmed up in the rtf leg / first pass)
        tok.decode_batch([torch.zeros(1, 4, 520, dtype=torch.long, device=dev)] * n_mine)
    stats = {}
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    waves, mine, toks = dp.synthesize(model, tok, utts, seed=0, tts=True, stats=stats, device=dev, **kw)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t1 = time.perf_counter()
    wall = t1 - t0
    if dist is not None:
        tt = torch.tensor([wall, stats["decode_s"], stats["codec_s"], -stats["decode_s"]], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        wall, dec, cod, dec_min = float(tt[0]), float(tt[1]), float(tt[2]), -float(tt[3])
    else:
        dec, cod = stats["decode_s"], stats["codec_s"]
        dec_min = dec
    n_new = sum(int(t.shape[1]) - 150 for t in toks)
    crc = 0
    for t in toks:
        crc = zlib.crc32(t.cpu().numpy().astype("<i8").tobytes(), crc)
    # waveforms stay on the rank that rendered them; their CRCs are combined in utterance order on rank 0 (a few bytes per utterance)
    wcrc = torch.zeros(64, dtype=torch.int64, device=dev)
    wlen = torch.zeros(64, dtype=torch.int64, device=dev)
    for gi, w in zip(mine, waves):
        wcrc[gi] = zlib.crc32(w.detach().cpu().numpy().astype("<f4").tobytes())
        wlen[gi] = w.shape[-1]
    if dist is not None:
        dist.all_reduce(wcrc, op=dist.ReduceOp.SUM)
        dist.all_reduce(wlen, op=dist.ReduceOp.SUM)
    wav_crc = zlib.crc32(wcrc.cpu().numpy().astype("<i8").tobytes())
    gen_s = float(wlen.sum()) / 16000.0
    return {"workload": "64 utterances, L=67, 150-frame prompts, greedy + CFG (stride 5), <= 8 utterances x 2 rows per engine pass; "
                        "tokens all-gathered, then every rank renders its own shard's waveforms (ragged wmencodec decode, prompt cut off)",
            "n_gpus": world, "utterances_per_gpu": (64 + world - 1) // world, "new_frames_total": n_new,
            "wall_ms_with_codec": round(1000 * wall, 1), "decode_ms_max_rank": round(1000 * dec, 1), "decode_ms_min_rank": round(1000 * dec_min, 1), "allgather_ms": round(1000 * stats["allgather_s"], 3),
            "codec_ms_max_rank": round(1000 * cod, 1), "generated_audio_s": round(gen_s, 2), "rtf": round(wall / max(gen_s, 1e-9), 5),
            "codec_tokens_per_s_per_gpu": round(4 * n_new / dec / world, 1), "codec_tokens_per_s_total": round(4 * n_new / wall, 1),
            "tokens_crc32": f"{crc:08x}", "wav_crc32": f"{wav_crc:08x}",
            "note": "tokens_crc32 is identical for every world size by construction (utterance i uses seed + i); wav_crc32 (CRC of the per-utterance fp32 "
                    "waveform CRCs) is too as long as every rank's shard takes the same LSTM step kernel (batches of 5..112 items all do)"}


def dp64_ragged_leg(model, args_lm, dev):
    """Continuous batching vs lock-step groups (one GPU): 64 utterances whose text length is uniform in 20..120 phonemes (so that the
    reference's 10 x L cap ends them after ~45..1045 steps), 150-frame prompts, greedy + CFG, 8 utterance slots. Same tokens either way."""
    import zlib
    g = torch.Generator().manual_seed(77)
    utts = []
    for i in range(64):
        L = int(torch.randint(20, 121, (1,), generator=g))
        utts.append({"x": torch.randint(0, 100, (1, L), generator=g), "y": torch.randint(0, 2048, (1, 150, 4), generator=g),
                     "mask_interval": torch.LongTensor([[[150, 150]]])})
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, aug_text=True)
    out = {"workload": "64 utterances, L uniform in 20..120, 150-frame prompts, greedy + CFG (stride 5), 8 utterance slots x 2 rows, one GPU"}
    crcs = []
    for name, refill in (("lockstep_groups", False), ("refill", True), ("lockstep_groups", False), ("refill", True)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = model.inference_batch(utts, seed=0, refill=refill, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_new = sum(int(r[0].shape[-1]) - 150 for r in res)
        crc = 0
        for r in res:
            crc = zlib.crc32(r[0].cpu().numpy().astype("<i8").tobytes(), crc)
        crcs.append(crc)
        tps = 4 * n_new / dt
        if name + "_tokens_per_s" not in out or tps > out[name + "_tokens_per_s"]:
            out[name + "_tokens_per_s"], out[name + "_wall_ms"] = round(tps, 1), round(1000 * dt, 1)
        out["new_frames_total"] = n_new
    out["speedup"] = round(out["refill_tokens_per_s"] / out["lockstep_groups_tokens_per_s"], 3)
    out["same_tokens"] = len(set(crcs)) == 1
    out["tokens_crc32"] = f"{crcs[0]:08x}"
    return out


def codec256_leg(dev, world, rank, dist, all_ok=lambda ok: ok):
    """BASELINE config 5: encode + decode of 256 clips x 30 s (16 kHz), 256 / N clips per rank, no collective."""
    from ssr_speech_amd import dp, weights as W
    from ssr_speech_amd.codec.wmencodec import WMEncodecModel
    cfg = W.codec_config_full()
    lo, hi = dp.shard_range(256, world, rank)
    B, n = hi - lo, 480000
    err, enc, dec, out = None, 0.0, 0.0, None
    try:
        m = WMEncodecModel(cfg, W.codec_state_dict(cfg, seed=0), dev)
        g = torch.Generator(device=dev).manual_seed(1234 + rank)
        wav = torch.randn(B, 1, n, generator=g, device=dev) * 0.1
        c, _, _ = m.encode(wav)                            # untimed full-size pass: kernels loaded, the caching allocator holds blocks of
        m.decode(c)                                        # every activation shape (a first decode at this size spent ~0.5 s in hipMalloc)
        del c
        torch.cuda.synchronize()
    except Exception as e:                                 # noqa: BLE001
        err = e
    if not all_ok(err is None):
        raise RuntimeError(f"codec256 set-up failed on {'this' if err is not None else 'another'} rank: {err!r}")
    if dist is not None:
        dist.barrier()
    try:
        t0 = time.perf_counter()
        codes, _, _ = m.encode(wav)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = m.decode(codes)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        enc, dec = t1 - t0, t2 - t1
    except Exception as e:                                 # noqa: BLE001
        err = e
    if not all_ok(err is None):
        raise RuntimeError(f"codec256 failed on {'this' if err is not None else 'another'} rank: {err!r}")
    # the same encode + decode with every GEMM on the exact fp32 FMA chain (the default path runs the codec's large GEMMs on the bf16
    # matrix cores with exactly split fp32 operands, csrc/gemm_split.hip: fp32-accurate, not bit-identical to the chain)
    exact = {}
    try:
        m.split_gemm = False
        m.encode(wav[: max(B // 8, 1)])                       # touch the exact kernels once
        torch.cuda.synchronize()
        x0 = time.perf_counter()
        c_ex, _, e_ex = m.encode(wav)
        torch.cuda.synchronize()
        x1 = time.perf_counter()
        o_ex = m.decode(c_ex)
        torch.cuda.synchronize()
        x2 = time.perf_counter()
        del o_ex
        # the decoder alone, on the SAME codes in both modes: a waveform difference that is always a number
        o_same = m.decode(codes)
        wav_diff = float((o_same - out).abs().max())
        del o_same
        # every RVQ code that differs between the two modes must be an fp32 near-tie: top-1 minus top-2 score along the chain's own
        # residual path < 1e-4 at the FIRST differing stage of that frame (later stages of the frame follow from the first flip)
        flips = c_ex != codes
        n_flips, worst = int(flips.sum()), 0.0
        if n_flips:
            first = flips & (flips.float().cumsum(1) == 1)
            sdc = W.codec_state_dict(cfg, seed=0)
            for b in torch.nonzero(flips.any(2).any(1)).flatten().tolist():
                res = e_ex[b].t().clone()                              # [T, D] latent of the exact pass
                for q in range(cfg.n_q):
                    E = sdc[f"quantizer.vq.layers.{q}._codebook.embed"].to(dev)
                    score = -(res.pow(2).sum(1, keepdim=True) - 2 * res @ E.t() + E.t().pow(2).sum(0, keepdim=True))
                    top2 = score.topk(2, dim=-1).values
                    fq = first[b, q]
                    if bool(fq.any()):
                        worst = max(worst, float((top2[:, 0] - top2[:, 1])[fq].max()))
                    res = res - E[c_ex[b, q]]
        exact = {"enc": x1 - x0, "dec": x2 - x1, "max_abs_wav_diff_vs_default": wav_diff,
                 "code_mismatch_vs_default": float(flips.float().mean()), "code_flips": n_flips, "max_reference_margin_at_a_flip": worst}
        if worst >= 1e-4:
            raise RuntimeError(f"split vs chain: an RVQ code differs where the fp32 margin is {worst:.3g} (>= 1e-4): not a near-tie")
        del c_ex, e_ex
    except Exception as e:                                 # noqa: BLE001
        err = e
    finally:
        m.split_gemm = True
    if not all_ok(err is None):
        raise RuntimeError(f"codec256 exact-fp32 pass failed on {'this' if err is not None else 'another'} rank: {err!r}")
    # wmdecode (the --use_watermark product path, seanet.py:555-600; SURVEY §8d config 5: marks = second half ones), without and with
    # the detector pass. Its skip encoder keeps four feature maps alive beside the decoder's activations: run in 4 batch lanes
    # (WMEncodecModel.lanes: same results, a quarter of the peak memory at 2-4 % of the throughput).
    wm_ms = {}
    peak_plain = torch.cuda.max_memory_allocated()
    try:
        del out
        torch.cuda.empty_cache()
        m.lanes = 4 if B >= 32 else 1
        marks = torch.zeros(B, codes.shape[-1], dtype=torch.long, device=dev)
        marks[:, codes.shape[-1] // 2:] = 1
        for with_mark in (False, True):
            m.wmdecode(codes, marks, wav, with_mark=with_mark)       # untimed pass (allocator)
            torch.cuda.synchronize()
            for _rep in range(2):                                    # best of two: the caching allocator may still be moving blocks between
                w0 = time.perf_counter()                             # the lanes' stream pools on the first timed pass (seen: 5.4 s vs 1.3 s)
                out, _mk = m.wmdecode(codes, marks, wav, with_mark=with_mark)
                torch.cuda.synchronize()
                dt = time.perf_counter() - w0
                wm_ms[with_mark] = min(wm_ms.get(with_mark, dt), dt)
                del _mk
    except Exception as e:                                 # noqa: BLE001
        err = e
    if not all_ok(err is None):
        raise RuntimeError(f"codec256 wmdecode failed on {'this' if err is not None else 'another'} rank: {err!r}")
    if dist is not None:
        tt = torch.tensor([enc, dec, wm_ms[False], wm_ms[True], exact["enc"], exact["dec"]], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        enc, dec, wm_ms[False], wm_ms[True], exact["enc"], exact["dec"] = (float(v) for v in tt)
    GF, audio_s = 6.97e9, 256 * 30.0
    return {"workload": f"256 clips x 30 s, {B} per GPU, full wmencodec config, synthetic weights", "n_gpus": world,
            "wmdecode_ms": round(1000 * wm_ms[False], 1), "wmdecode_with_detector_ms": round(1000 * wm_ms[True], 1),
            "wmdecode_tflops_per_gpu": round(14.5e9 * audio_s / wm_ms[False] / 1e12 / world, 1),
            "wmdecode_with_detector_tflops_per_gpu": round(21.69e9 * audio_s / wm_ms[True] / 1e12 / world, 1),
            "wmdecode_note": f"marks = second half ones; {m.lanes} batch lane(s); 14.5 / 21.69 GFLOP per audio-second without / with the detector (SURVEY 8d)",
            "peak_mem_gib_encode_decode": round(peak_plain / 2 ** 30, 1),
            "gemm": "large GEMMs (N > 64) on the bf16 matrix cores, fp32 operands split exactly into 3 bf16 pieces, 6 cross products, fp32 accumulation "
                    "(csrc/gemm_split.hip, gemm_split_dma_kernel: 8 waves per workgroup, W global -> LDS by DMA; error vs fp64 <= the fp32 FMA chain's); "
                    "SSRHIP_GEMM_SPLIT=0 = the chain",
            "exact_fp32_chain": {"encode_ms": round(1000 * exact["enc"], 1), "decode_ms": round(1000 * exact["dec"], 1),
                                 "encode_tflops_per_gpu": round(GF * audio_s / exact["enc"] / 1e12 / world, 1),
                                 "decode_tflops_per_gpu": round(GF * audio_s / exact["dec"] / 1e12 / world, 1),
                                 "code_mismatch_vs_default": exact.get("code_mismatch_vs_default"), "code_flips": exact.get("code_flips"),
                                 "max_reference_margin_at_a_flip": exact.get("max_reference_margin_at_a_flip"),
                                 "max_abs_wav_diff_vs_default": exact.get("max_abs_wav_diff_vs_default"),
                                 "note": "wav diff = the DECODER alone on the default path's codes in both modes; every differing code is checked to be an "
                                         "fp32 near-tie (top-1 minus top-2 score < 1e-4 on the chain's own residual path) or the leg fails"},
            "encode_ms": round(1000 * enc, 1), "decode_ms": round(1000 * dec, 1),
            "encode_audio_s_per_s": round(audio_s / enc, 1), "decode_audio_s_per_s": round(audio_s / dec, 1),
            "encode_tflops_per_gpu": round(GF * audio_s / enc / 1e12 / world, 1), "decode_tflops_per_gpu": round(GF * audio_s / dec / 1e12 / world, 1),
            "mfma_fp32_peak_tflops": 157.3, "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), "out_shape": list(out.shape)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--utts", type=int, default=1, help="utterances decoded in lock-step per GPU (default 1 = the headline configuration)")
    ap.add_argument("--no-extras", action="store_true", help="skip the rtf_10s_tts / dp64 / dp64_ragged / codec256 / wmencodec legs")
    ap.add_argument("--no-ctx700", action="store_true", help="skip the second timed region around context 700 (counter-collection runs: rocprofv3 --pmc "
                    "crashed with ~400 graph replays in flight behind one synchronisation, round 6)")
    ap.add_argument("--legs", type=str, default="", help="comma separated subset of the extra legs to run (default: all)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="after the timed steps, write what they computed (codec tokens of the "
                    "timed steps, logits of the last step, sampler state) as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true", help="beside the headline, also the repeat passes, the context-700 region, the roofline, "
                    "the all_gather (N > 1), the extra legs and the CPU baseline (default: the headline alone)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full and (a.no_cpu_baseline or a.no_extras or a.no_ctx700 or a.legs):
        ap.error("--no-cpu-baseline, --no-extras, --no-ctx700 and --legs trim what --full adds: give --full with them")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # nccl == RCCL on ROCm

    import ssr_speech_amd  # noqa: F401
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd import weights as W
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena

    args_lm = W.lm_args_830m()
    sd = W.lm_state_dict(args_lm, seed=0, device=dev)
    arena = LMWeightsArena(args_lm, sd, dev)
    demo_y = demo_prompt_codes(dev)
    x, y, unc = synth_inputs(args_lm, rank, prompt_codes=demo_y)
    L, N = x.shape[1], y.shape[1]
    total = a.warmup + a.steps
    cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), np.asarray([[N, N]]), args_lm)
    T0 = cated.shape[1]
    assert T0 + 1 + total <= 10 * L, "bench would hit the reference's length cap (10*L): lower --steps"
    U = a.utts          # utterances decoded in lock-step on this GPU (1 = the headline configuration; 8 = SURVEY §8d config 4)
    # capacity: the timed pass, and the long-context pass below (context ~700 whatever --steps is) — at least 512 steps / 1024 positions
    eng = DecodeEngine(arena, U, True, ((max(L + T0 + total, 760) + 8 + 1023) // 1024) * 1024, max(((total + 255) // 256) * 256, 512))
    kn = DecodeKnobs(top_k=40, top_p=0.8, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=5, use_cfg=True,
                     text_len=L, n_spans=num_task, seed=2024 + rank)
    text_rows = []
    for u in range(U):          # utterance u > 0: same shapes, its own text ids
        xu, _, uu = (x, y, unc) if u == 0 else synth_inputs(args_lm, rank * 64 + u)
        text_rows += [xu[0].numpy(), uu[0].numpy()]
    seed_try = 0
    while True:
        kns = [dataclasses.replace(kn, seed=2024 + rank * 64 + u + 1000 * seed_try) for u in range(U)]
        eng.start(text_rows, [cated] * U, kns, noise=None)
        torch.cuda.synchronize()
        eng.decode(a.warmup, use_graph=not a.no_graph)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        eng.decode(a.steps, use_graph=not a.no_graph)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t1 = time.perf_counter()
        st = eng.states()[0]
        if all(s_.n_steps == total for s_ in eng.states()) or seed_try >= 3:
            break
        seed_try += 1           # the sampler drew <eog> inside the timed region: different stream, same workload
    elapsed = t1 - t0
    dumped = dump_outputs(a.dump_outputs, eng, a.warmup, a.steps) if a.dump_outputs and rank == 0 else None
    # the same W + K steps again (restart, warm-up, K timed steps: same context range), listed beside the headline: the driver's timed region
    # is ~17 ms and boxes differ by 3-5 %, so one pass cannot resolve a 1 % change. `ms_per_step` stays the FIRST pass.
    extra_passes = []
    if a.full and dist is None:
        for _rep in range(4):
            eng.start(text_rows, [cated] * U, kns, noise=None)
            torch.cuda.synchronize()
            eng.decode(a.warmup, use_graph=not a.no_graph)
            torch.cuda.synchronize()
            p0 = time.perf_counter()
            eng.decode(a.steps, use_graph=not a.no_graph)
            torch.cuda.synchronize()
            extra_passes.append(1000 * (time.perf_counter() - p0) / a.steps)
    if dist is not None:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if a.full and dist is not None:
        # the one collective of the path: gather every rank's generated codec tokens (before wmencodec decode)
        from ssr_speech_amd import dp
        mine = eng.generated[0, : st.n_steps].t().contiguous()          # [K, steps] of this rank's utterance
        torch.cuda.synchronize()
        g0 = time.perf_counter()
        everyone = dp.gather_tokens([mine], world, arena.K, pad_token=int(args_lm.empty_token), device=dev)
        torch.cuda.synchronize()
        allgather_ms = 1000 * (time.perf_counter() - g0)
        assert len(everyone) == world and torch.equal(everyone[rank].to(torch.int32), mine)
    else:
        allgather_ms = None

    out = None
    if rank == 0:
        ms_per_step = 1000 * elapsed / a.steps
        tokens_per_step = 4 * world * U                  # K=4 codebooks x 1 frame x U utterances per GPU
        value = tokens_per_step * a.steps / elapsed
        out = {
            "metric": "codec-tokens/sec/GPU (AR decode) + RTF for 10 s TTS, English 830M",
            "value": round(value, 1), "unit": "codec-tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"English-830M-shape zero-shot TTS decode, cfg_stride=5, top_k=40/top_p=0.8 sampling, batch={U} ({2 * U} CFG rows) per GPU; "
                                   f"L={L} phonemes, {N}-frame prompt ({'demo/5895_34622_000026_000002.wav, first 3.2 s, wmencodec codes' if demo_y is not None else 'random codes'}), "
                                   f"context {L + T0 + a.warmup}..{L + T0 + total}",
                       "utterances_per_gpu": U, "rows": 2 * U, "graph": not a.no_graph, "steps_completed": int(st.n_steps),
                       "pair_launches": bool(eng.pairing), "pair_launches_why": eng.pairing_why},
            "per_gpu_value": round(value / world, 1),
            "decode_rtf_10s": round((500 * ms_per_step / 1000) / 10.0, 4),
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": a.dump_outputs, "shapes": dumped}

    if rank == 0 and a.full:
        # ---- roofline of the dominant kernel (weight-streaming GEMV). Two HIP-event measurements on the launch stream:
        #  * per-slot: an event pair around every launch of eager steps (per-shape view; carries ~3 us event overhead each);
        #  * category: the 66 GEMV launches of a step replayed as a hipGraph between ONE event pair -> the average launch
        #    duration as the product runs it; this is what `achieved` uses and what rocprofv3's durations must agree with.
        slots = eng.time_kernels(8)
        gemv_slots = [us for kind, us in slots if kind == "gemv"]
        n_gemv = len(gemv_slots)
        w_bytes = arena.nbytes_per_step() - 4 * (arena.K + 1) * arena.D      # GEMV-streamed bytes (embedding rows excluded)
        bytes_per_launch = w_bytes / n_gemv
        gemv_us_eager = sum(gemv_slots) / n_gemv
        gemv_us, n_cat = eng.time_category("gemv", 50)
        attn_us = eng.time_category("attn", 50)[0]
        room = min(eng.max_steps - int(eng.states()[0].n_steps), eng.max_seq - int(L + T0 + eng.states()[0].n_steps)) - 8
        samp_us = eng.time_category("sample", min(50, room) - 3)[0] if room >= 10 else float("nan")   # the sampler advances the state
        assert n_cat == n_gemv
        # ---- the long half of a 10 s utterance: the same workload timed around context 700 — the driver's default
        # timed region sits at context ~300-325, where the attention launches read half as many KV pages. Same engine, same inputs.
        ctx700 = None
        n_attn = len([1 for kind, _ in slots if kind == "attn"])
        # share of the step spent in the attention launches: launches x their duration (timed alone, graph-chained, at the context the engine
        # had reached when it was timed) / the region's ms per step — an upper bound for the headline region (its average context is lower)
        attn_share = {f"headline_region(attention timed at context {L + T0 + total + 8})": round(n_attn * attn_us / (1000.0 * ms_per_step), 4)}
        pre, n_t = 700 - (L + T0) - 10, 20
        if dist is None and not a.no_ctx700 and pre > 0 and pre + n_t + 8 <= eng.max_steps and T0 + 1 + pre + n_t <= 10 * L:
            for seed_try2 in range(4):
                kns2 = [dataclasses.replace(kn, seed=777 + u + 1000 * seed_try2) for u in range(U)]
                eng.start(text_rows, [cated] * U, kns2, noise=None)
                eng.decode(pre, use_graph=not a.no_graph)
                torch.cuda.synchronize()
                q0 = time.perf_counter()
                eng.decode(n_t, use_graph=not a.no_graph)
                torch.cuda.synchronize()
                q1 = time.perf_counter()
                if all(s_.n_steps == pre + n_t for s_ in eng.states()):
                    ms700 = 1000 * (q1 - q0) / n_t
                    attn700 = eng.time_category("attn", 50)[0]
                    ctx700 = {"ms_per_step": round(ms700, 4), "codec_tokens_per_s": round(4 * U / (ms700 * 1e-3), 1), "steps": n_t,
                              "context": [L + T0 + pre, L + T0 + pre + n_t], "attn_us_per_launch": round(attn700, 3)}
                    attn_share[f"ctx700_region(attention timed at context {L + T0 + pre + n_t})"] = round(n_attn * attn700 / (1000.0 * ms700), 4)
                    break
        achieved = bytes_per_launch / (gemv_us * 1e-6) / 1e9
        # per-shape view of one layer (slots 0..4 = QKV, attention, out-proj, FFN1, FFN2 of layer 0.., averaged over layers)
        nl = arena.L
        paired = None
        if 2 * U == 2 and len(slots) == 1 + 3 * nl + 2:   # 2 rows, both pair forms (csrc/gemv.hip): QKV of layer 0, then per layer attention,
            paired = "both"                               # [merge + out-proj + LN2 + FFN1], [FFN2 + LN1 + QKV of the next layer | + head MLP]
            avg = lambda j, ls: round(sum(slots[1 + 3 * l + j][1] for l in ls) / len(ls), 3)
            per_shape = {"ln1+qkv (layer 0 only)": round(slots[0][1], 3), "attn": avg(0, range(nl)),
                         "combine+out_proj | ln2+ffn1 (one launch)": avg(1, range(nl)),
                         "ffn2 | ln1+qkv of the next layer (one launch)": avg(2, range(nl - 1)),
                         "ffn2 | lnf+head1 (one launch)": round(slots[1 + 3 * (nl - 1) + 2][1], 3),
                         "head2": round(slots[1 + 3 * nl][1], 3), "sample+embed": round(slots[1 + 3 * nl + 1][1], 3)}
        elif 2 * U == 2 and len(slots) == 1 + 4 * nl + 2:  # SSRHIP_GEMV_PAIR=1: only FFN2 is paired
            paired = "ffn2"
            avg = lambda j, ls: round(sum(slots[1 + 4 * l + j][1] for l in ls) / len(ls), 3)
            per_shape = {"ln1+qkv (layer 0 only)": round(slots[0][1], 3), "attn": avg(0, range(nl)), "combine+out_proj": avg(1, range(nl)),
                         "ln2+ffn1": avg(2, range(nl)), "ffn2 | ln1+qkv of the next layer (one launch)": avg(3, range(nl - 1)),
                         "ffn2 | lnf+head1 (one launch)": round(slots[1 + 4 * (nl - 1) + 3][1], 3),
                         "head2": round(slots[1 + 4 * nl][1], 3), "sample+embed": round(slots[1 + 4 * nl + 1][1], 3)}
        else:
            ns_slots = (len(slots) - 3) // nl                 # launches per layer as the engine enqueued them
            if 2 * U <= 4:
                shape_names = ["ln1+qkv", "attn", "combine+out_proj", "ln2+ffn1", "ffn2"]
            elif ns_slots == 5:                               # > 4 rows, fused walk over the pages (ssrhip_attn_rows): no combine launch
                shape_names = ["ln1+qkv", "attn_rows", "out_proj", "ln2+ffn1", "ffn2"]
            else:                                             # > 4 rows, split attention: the combine is its own launch
                shape_names = ["ln1+qkv", "attn", "combine", "out_proj", "ln2+ffn1", "ffn2"]
            assert ns_slots == len(shape_names), (ns_slots, shape_names)
            ns = len(shape_names)
            per_shape = {shape_names[j]: round(sum(slots[l * ns + j][1] for l in range(nl)) / nl, 3) for j in range(ns)}
            per_shape.update({"lnf+head1": round(slots[nl * ns][1], 3), "head2": round(slots[nl * ns + 1][1], 3), "sample+embed": round(slots[nl * ns + 2][1], 3)})
        S_mid = L + T0 + a.warmup + a.steps // 2
        kv_bytes = 262144 * 2 * U * S_mid * (arena.L / 16) * (arena.D / 2048)
        step_gbs = (arena.nbytes_per_step() + kv_bytes) / (ms_per_step * 1e-3) / 1e9
        out.update({
            "ms_per_step_passes": [round(ms_per_step, 4)] + [round(v, 4) for v in extra_passes],
            "ms_per_step_ctx700": (ctx700["ms_per_step"] if ctx700 else None), "ctx700": ctx700, "attention_share_of_step": attn_share,
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4),
                         # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command (profiles/r06_pmc_*.md; `--no-ctx700`), gfx950 x2 correction
                         # for wide reads applied: per step 3,330.0 MB read + 4.6 MB written vs 3,290.2 MB algorithmic (divided by the step's GEMV launch count)
                         "traffic": (round(TRAFFIC_BYTES_PER_STEP_GEMVS[2 * U] / n_gemv) if (2 * U in TRAFFIC_BYTES_PER_STEP_GEMVS and arena.D == 2048 and arena.L == 16) else None),
                         "traffic_source": TRAFFIC_SOURCE.get(2 * U, "not measured for this row count") + " (rocprofv3 --pmc passes of this command, gfx950 x2 FETCH_SIZE correction)",
                         "kernel": ((f"gemv_pair_merge_kernel (split-KV merge + out-proj + residual | LN + FFN1 + ReLU) and gemv_pair_kernel (FFN2 + residual | LN + QKV + KV append) "
                                     f"— two GEMVs per launch, the all-to-all edge inside — plus gemv_segu_kernel (QKV of layer 0, head MLP): all {n_gemv} GEMV launches of a step")
                                    if paired == "both" else
                                    f"gemv_segu_kernel<2,*> / gemv_seg_kernel<2,*> / gemv_pair_kernel (fused LN or split-KV merge + GEMV + bias/act/residual), all {n_gemv} GEMV launches of a step"
                                    if 2 * U <= 4 else
                                    f"gemv_rows_xreg_kernel / gemv_rows_stream_kernel (matrix-core GEMV, streaming-order weights), all {n_gemv} launches of a step"),
                         "bytes_per_launch": int(bytes_per_launch), "launches_per_step": n_gemv, "us_per_launch": round(gemv_us, 3),
                         "us_per_launch_eager_event_pair": round(gemv_us_eager, 3),
                         "other_kernels_us_per_launch": {k_: round(v_, 3) for k_, v_ in (("attn_decode", attn_us), ("sample+embed", samp_us)) if v_ == v_},
                         "step_level": {"bytes_per_step": int(arena.nbytes_per_step() + kv_bytes), "achieved": round(step_gbs, 1),
                                        "frac": round(step_gbs / HBM_PEAK_GBS, 4)},
                         "event_timed_us_per_launch": per_shape},
        })
        if allgather_ms is not None:
            out["allgather_ms"] = round(allgather_ms, 3)

    # ---- extras (every rank takes part: dp64 ends in a collective). None of them feeds `value`.
    extras = {}
    if a.full and not a.no_extras and U == 1:
        eng.close()                              # gives the device's pairing slot back (csrc/engine.hip): the API model's engine takes it next
        del eng
        torch.cuda.empty_cache()
        import tempfile

        def all_ok(ok: bool) -> bool:
            """Every rank reports whether its LOCAL part of a leg worked; the leg's collective only runs when all did."""
            if dist is None:
                return ok
            t = torch.tensor([1 if ok else 0], device=dev, dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(int(t.item()))

        wanted = {v for v in a.legs.split(",") if v}

        def leg(name, fn):
            if wanted and name not in wanted:
                return
            # the headline metric must not depend on an extra: a failure becomes an "error" entry. dp64's collective is guarded
            # inside dp.generate (ranks agree on success before the all-gather); codec256's only collective is a timing all-reduce
            # behind all_ok().
            try:
                extras[name] = fn()
            except Exception as e:
                extras[name] = {"error": repr(e)}

        model = None
        try:
            model = build_api_model(args_lm, sd, dev)
        except Exception as e:
            extras["rtf_10s_tts"] = extras["dp64"] = {"error": repr(e)}
        if not all_ok(model is not None):
            if model is not None:
                model._invalidate()
            model = None
            extras.setdefault("dp64", {"error": "model build failed on another rank"})
        if model is not None:
            if world == 1:
                with tempfile.TemporaryDirectory() as td:
                    leg("rtf_10s_tts", lambda: rtf_leg(model, args_lm, dev, td))
            leg("dp64", lambda: dp64_leg(model, args_lm, dev, world, rank, dist))
            if world == 1:
                leg("dp64_ragged", lambda: dp64_ragged_leg(model, args_lm, dev))
            model._invalidate()
            del model
            torch.cuda.empty_cache()
        leg("codec256", lambda: codec256_leg(dev, world, rank, dist, all_ok))
        if world == 1:
            leg("wmencodec", lambda: codec_leg(dev, with_cpu=not a.no_cpu_baseline))

    if rank == 0:
        out.update(extras)
        if world == 1 and a.full and not a.no_cpu_baseline and U == 1:
            out["cpu_baseline"] = cpu_baseline(args_lm, sd, x, y, unc)
            out["speedup_vs_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
