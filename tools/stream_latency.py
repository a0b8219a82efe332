"""When does the first audio leave, and what does handing it out early cost? The 830M shape with bench.py's `rtf_10s_tts` inputs
(the `demo_5895..._160f` prompt, 67 phonemes, top-k 40 / top-p 0.8 sampling, CFG stride 5), in one process: one untimed warm-up run of
`inference_one_sample` and of `inference_one_sample_stream`, then 3 alternating rounds of the two with the same seeds. Reports the
host time to the first yielded chunk (after a stream synchronize on it), that chunk's length, both paths' total wall time, and the
codec launches per stage-2 window. One JSON line on stdout; `--out FILE` also writes it there.
`--weight_dtype bf16` measures the bf16 weight stream (`SSR_Speech.set_weight_dtype`); the output also carries the real-time factor
(wall time / seconds of audio) of both paths.
`--utts N` measures the BATCHED stream instead (DESIGN.md Part I.16): N samples of that utterance in one lock-step group under CFG,
`inference_samples_stream` against `inference_batch(refill=False, group=N)` + `render_many` in the same process, same warm-up and
rounds; it reports the host time to the first chunk of the FIRST and of the LAST utterance (after a stream synchronize), both arms'
total wall time (median and spread of the rounds), the polls and the codec launches per run.
`--use_watermark` measures the WATERMARKED stream (DESIGN.md Part I.17): one-pass `inference_one_sample(use_watermark=True)`,
`inference_one_sample_wmstream` and, for scale, the un-watermarked stream, same warm-up and rounds; it reports the first audio at the
caller, the total wall time of the three, the chunks, the codec's library calls per 16-frame push, the hold-back in frames and whether
every round was bit-identical.
`--utts N --use_watermark` measures the BATCHED WATERMARKED stream (DESIGN.md Part I.29): `inference_samples_wmstream` against
`inference_samples(use_watermark=True)` in the same process, same warm-up and rounds; it reports the host time to the first chunk of
every utterance, both arms' total wall time, the codec's library calls per poll in which every utterance is live (and how many of them
are row-op launches) and the bytes of the stream's tap buffers.
Usage: python tools/stream_latency.py [--weight_dtype bf16] [--utts 8] [--use_watermark] [--out profiles/stream_latency_830m.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import weights as W  # noqa: E402
from ssr_speech_amd.data.tokenizer import AudioTokenizer, write_wav  # noqa: E402
from ssr_speech_amd.inference_scale import (_phoneme_ids, _prompt_codes, inference_one_sample, inference_one_sample_stream,  # noqa: E402
                                            inference_one_sample_wmstream, inference_samples, inference_samples_stream,
                                            inference_samples_wmstream, render_many)
from ssr_speech_amd.models.ssr import SSR_Speech  # noqa: E402

DEMO_PROMPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "demo_5895_34622_000026_000002_160f.wav")


class CharPhonemizer:
    def __call__(self, texts):
        return [[c for c in t if c != " "] for t in texts]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--weight_dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--codec_weight_dtype", choices=["fp32", "bf16"], default="fp32", help="the codec's weights (DESIGN.md Part I.30; SSRHIP_CODEC_W1=0: three planes)")
    ap.add_argument("--codec_act_dtype", choices=["fp32", "bf16"], default="fp32", help="bf16 (with --codec_weight_dtype bf16): bf16 activation operands (DESIGN.md Part I.32)")
    ap.add_argument("--utts", type=int, default=0, help="N > 0: the batched stream of N utterances against inference_batch + render_many")
    ap.add_argument("--use_watermark", action="store_true", help="the watermarked stream against one-pass inference_one_sample(use_watermark=True)")
    opt = ap.parse_args(argv)
    dev = torch.device("cuda")
    args_lm = W.lm_args_830m()
    sd = W.lm_state_dict(args_lm, seed=0, device=dev)
    for k in range(args_lm.n_codebooks):          # only codec ids leave the LM (bench.py build_api_model)
        b = sd[f"predict_layer.{k}.2.bias"].clone()
        b[int(args_lm.audio_vocab_size):] = -30.0
        sd[f"predict_layer.{k}.2.bias"] = b
    model = SSR_Speech(args_lm)
    model.load_state_dict({k: v.cpu() for k, v in sd.items()})
    del sd
    model = model.to(dev).eval()
    model.set_weight_dtype(opt.weight_dtype)
    ccfg = W.codec_config_full()
    tok = AudioTokenizer(device=dev, config=ccfg, state_dict=W.codec_state_dict(ccfg, seed=0), weight_dtype=opt.codec_weight_dtype,
                         act_dtype=opt.codec_act_dtype)
    g = torch.Generator().manual_seed(7)
    n_prompt = 160
    noise_prompt = torch.randn(1, n_prompt * 320, generator=g) * 0.1
    tmp = tempfile.mkdtemp()
    fn = DEMO_PROMPT
    if not os.path.exists(fn):
        fn = os.path.join(tmp, "prompt.wav")
        write_wav(fn, noise_prompt, 16000)
    symbols = [chr(ord("a") + i) for i in range(26)] + [chr(ord("A") + i) for i in range(26)]
    phn2num = {c: i for i, c in enumerate(symbols)}
    prompt_text = "".join(symbols[int(i)] for i in torch.randint(0, 52, (20,), generator=g))
    target_text = prompt_text + " " + "".join(symbols[int(i)] for i in torch.randint(0, 52, (47,), generator=g))
    decode_config = {"top_k": 40, "top_p": 0.8, "temperature": 1, "stop_repetition": 2, "kvcache": 1, "codec_audio_sr": 16000, "codec_sr": 50}
    mi = torch.LongTensor([[n_prompt, n_prompt]])
    call = (model, argparse.Namespace(**vars(args_lm)), phn2num, CharPhonemizer(), tok, fn, prompt_text, target_text, mi, 1.5, 5, True, False,
            False, True, dev, decode_config)
    codec = tok.codec
    if opt.utts > 0 and opt.use_watermark:
        return batched_watermarked(opt, model, tok, call)
    if opt.utts > 0:
        return batched(opt, model, args_lm, tok, call, phn2num, fn, target_text, mi)

    def one_pass(seed, call=call):
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = inference_one_sample(*call)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lr = model.last_run
        return wav, dict(total_ms=1000 * (t1 - t0), first_16_frames_ms=1000 * (lr["t_first_chunk"] - t0), steps=int(lr["steps"]),
                         lm_ms=1000 * (lr["t_end"] - lr["t_start"]), audio_s=wav.shape[-1] / 16000.0)

    def streamed(seed, gen=inference_one_sample_stream, call=call):
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        n0 = codec.n_launches
        t0 = time.perf_counter()
        chunks, first_ms = [], None
        for chunk in gen(*call):
            if first_ms is None:
                torch.cuda.current_stream().synchronize()
                first_ms = 1000 * (time.perf_counter() - t0)
            chunks.append(chunk)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lr = model.last_run
        wav = torch.cat(chunks, -1)
        return wav, dict(total_ms=1000 * (t1 - t0), first_chunk_ms=first_ms, first_chunk_samples=int(chunks[0].shape[-1]),
                         first_16_frames_ms=1000 * (lr["t_first_chunk"] - t0), chunks=len(chunks), steps=int(lr["steps"]),
                         lm_ms=1000 * (lr["t_end"] - lr["t_start"]), codec_launches=codec.n_launches - n0, audio_s=wav.shape[-1] / 16000.0)

    if opt.use_watermark:
        return watermarked(opt, model, codec, ccfg, call, one_pass, streamed)
    one_pass(1)
    streamed(1)
    rounds = []
    for r in range(opt.rounds):
        wa, a = one_pass(1 + r)
        wb, b = streamed(1 + r)
        b["bit_identical"] = bool(wa.shape == wb.shape and torch.equal(wa, wb))
        rounds.append({"one_pass": a, "stream": b})
    # one more streamed run with every push / finish timed on its own (call + stream synchronize): what the codec's share of the loop
    # costs when nothing overlaps it; the polls' other additions (reading the new rows, the frame release) are the rest
    from ssr_speech_amd.codec.wmencodec import DecodeStream  # noqa: E402
    spent = {"push_ms": 0.0, "calls": 0}
    real_push, real_finish = DecodeStream.push, DecodeStream.finish

    def timed(fn):
        def wrapper(self, *a, **k):
            torch.cuda.current_stream().synchronize()
            t0 = time.perf_counter()
            out = fn(self, *a, **k)
            torch.cuda.current_stream().synchronize()
            spent["push_ms"] += 1000 * (time.perf_counter() - t0)
            spent["calls"] += 1
            return out
        return wrapper

    DecodeStream.push, DecodeStream.finish = timed(real_push), timed(real_finish)
    try:
        _, timed_run = streamed(1)
    finally:
        DecodeStream.push, DecodeStream.finish = real_push, real_finish
    # launches of one interior stage-2 window and of one 16-frame stage-1 advance, counted on a stream of their own
    st = codec.decode_stream(64)
    codes = torch.zeros(1, ccfg.n_q, 64, dtype=torch.long, device=dev)
    st.push(codes[..., :24])
    n0, w0 = codec.n_launches, st.windows
    st.push(codes[..., 24:40])
    per_push = dict(launches=codec.n_launches - n0, windows=st.windows - w0)
    st.finish()
    torch.cuda.synchronize()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {
        "tool": "tools/stream_latency.py", "shape": "830M LM, full codec (8,5,4,2), 160-frame demo prompt, 67 phonemes, sampled, CFG stride 5",
        "weight_dtype": opt.weight_dtype,
        "rounds": rounds,
        "median": {
            "one_pass_rtf": round(med([r["one_pass"]["total_ms"] / 1000 / r["one_pass"]["audio_s"] for r in rounds]), 5),
            "stream_rtf": round(med([r["stream"]["total_ms"] / 1000 / r["stream"]["audio_s"] for r in rounds]), 5),
            "one_pass_total_ms": round(med([r["one_pass"]["total_ms"] for r in rounds]), 2),
            "stream_total_ms": round(med([r["stream"]["total_ms"] for r in rounds]), 2),
            "stream_first_chunk_ms": round(med([r["stream"]["first_chunk_ms"] for r in rounds]), 2),
            "one_pass_first_16_frames_ms": round(med([r["one_pass"]["first_16_frames_ms"] for r in rounds]), 2),
            "stream_first_16_frames_ms": round(med([r["stream"]["first_16_frames_ms"] for r in rounds]), 2),
        },
        "first_chunk_samples": rounds[0]["stream"]["first_chunk_samples"],
        "codec_launches_per_16_frame_push": per_push,
        "synchronized_pushes": {"summed_ms": round(spent["push_ms"], 2), "calls": spent["calls"], "run_total_ms": round(timed_run["total_ms"], 2)},
        "all_bit_identical": all(r["stream"]["bit_identical"] for r in rounds),
    }
    line = json.dumps(out)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


def watermarked(opt, model, codec, ccfg, call, one_pass, streamed):
    """--use_watermark: `inference_one_sample_wmstream` against one-pass `inference_one_sample(use_watermark=True)`, and the
    un-watermarked stream for scale; `one_pass(seed, call)` / `streamed(seed, gen, call)` are main's timed runs"""
    from ssr_speech_amd.codec.wmencodec import wm_stream_holdback
    call_wm = call[:13] + (True,) + call[14:]
    arms = (("one_pass", lambda s: one_pass(s, call_wm)), ("wmstream", lambda s: streamed(s, inference_one_sample_wmstream, call_wm)),
            ("stream", lambda s: streamed(s)))
    for _, run in arms:
        run(1)
    rounds = []
    for r in range(opt.rounds):
        got = {name: run(1 + r) for name, run in arms}
        row = {name: stats for name, (_, stats) in got.items()}
        wa, wb = got["one_pass"][0], got["wmstream"][0]
        row["wmstream"]["bit_identical"] = bool(wa.shape == wb.shape and torch.equal(wa, wb))
        rounds.append(row)
    # launches of one 16-frame push in the middle of an utterance, counted on streams of their own
    dev = codec.device
    codes = torch.zeros(1, ccfg.n_q, 64, dtype=torch.long, device=dev)
    marks, wav = torch.ones(64, dtype=torch.long, device=dev), torch.zeros(1, 1, 64 * 320, device=dev)
    per_push = {}
    for name, st, args in (("wmstream", codec.wmdecode_stream(64), lambda a, b: (codes[..., a:b], marks[a:b], wav[..., a * 320: b * 320])),
                           ("stream", codec.decode_stream(64), lambda a, b: (codes[..., a:b],))):
        st.push(*args(0, 24))
        n0, w0 = codec.n_launches, st.windows
        st.push(*args(24, 40))
        per_push[name] = dict(launches=codec.n_launches - n0, windows=st.windows - w0)
        st.finish()
    torch.cuda.synchronize()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    col = lambda arm, key: [r[arm][key] for r in rounds]
    out = {
        "tool": "tools/stream_latency.py --use_watermark", "weight_dtype": opt.weight_dtype,
        "shape": "830M LM, full codec (8,5,4,2), 160-frame demo prompt, 67 phonemes, sampled, CFG stride 5, watermarked decode",
        "rounds": rounds,
        "median": {
            "one_pass_total_ms": round(med(col("one_pass", "total_ms")), 2),
            "wmstream_total_ms": round(med(col("wmstream", "total_ms")), 2),
            "wmstream_first_chunk_ms": round(med(col("wmstream", "first_chunk_ms")), 2),
            "stream_total_ms": round(med(col("stream", "total_ms")), 2),
            "stream_first_chunk_ms": round(med(col("stream", "first_chunk_ms")), 2),
        },
        "wmstream_chunks": col("wmstream", "chunks"),
        "wmstream_first_chunk_samples": rounds[0]["wmstream"]["first_chunk_samples"],
        "codec_launches_per_16_frame_push": per_push,
        "codec_launches_per_run": {"wmstream": med(col("wmstream", "codec_launches")), "stream": med(col("stream", "codec_launches"))},
        "holdback_frames": wm_stream_holdback(ccfg),
        "all_bit_identical": all(r["wmstream"]["bit_identical"] for r in rounds),
    }
    line = json.dumps(out)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


def batched(opt, model, args_lm, tok, call, phn2num, fn, target_text, mi):
    """--utts N: `inference_samples_stream` against `inference_batch(refill=False, group=N)` + `render_many`"""
    n, codec = opt.utts, tok.codec
    decode_config, K = call[-1], int(args_lm.n_codebooks)

    def one_pass(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prompt_frames, scale = _prompt_codes(tok, fn, K)
        one = {"x": _phoneme_ids(CharPhonemizer(), phn2num, target_text), "y": prompt_frames, "mask_interval": mi.unsqueeze(0)}
        results = model.inference_batch([one] * n, top_k=decode_config["top_k"], top_p=decode_config["top_p"], temperature=decode_config["temperature"],
                                        stop_repetition=decode_config["stop_repetition"], cfg_coef=1.5, cfg_stride=5, aug_text=True, seed=seed,
                                        group=n, refill=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        waves = render_many(tok, results, scale, fn, False, True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return waves, dict(total_ms=1000 * (t2 - t0), lm_ms=1000 * (t1 - t0), render_ms=1000 * (t2 - t1),
                           frames=[int(r[0].shape[-1]) for r in results], audio_s=sum(w.shape[-1] for w in waves) / 16000.0)

    def streamed(seed):
        torch.cuda.synchronize()
        n0 = codec.n_launches
        t0 = time.perf_counter()
        parts, first = [[] for _ in range(n)], {}
        for i, chunk in inference_samples_stream(*call, seeds=list(range(seed, seed + n))):
            if i not in first and (not first or len(first) == n - 1):      # the first chunk of the first and of the last utterance
                torch.cuda.current_stream().synchronize()
            first.setdefault(i, 1000 * (time.perf_counter() - t0))
            parts[i].append(chunk)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        waves = [torch.cat(p, -1) for p in parts]
        eng = next(iter(model._engines.values()))
        return waves, dict(total_ms=1000 * (t1 - t0), first_chunk_first_utt_ms=min(first.values()), first_chunk_last_utt_ms=max(first.values()),
                           first_chunk_samples=int(parts[0][0].shape[-1]), chunks=sum(len(p) for p in parts), polls=eng._steps_enqueued // 16,
                           codec_launches=codec.n_launches - n0, audio_s=sum(w.shape[-1] for w in waves) / 16000.0)

    one_pass(1)
    streamed(1)
    rounds = []
    for r in range(opt.rounds):
        wa, a = one_pass(1 + 100 * r)
        wb, b = streamed(1 + 100 * r)
        b["max_abs_diff"] = max(float((x - y).abs().max()) if x.shape == y.shape else float("inf") for x, y in zip(wa, wb))
        rounds.append({"one_pass": a, "stream": b})
    med = lambda xs: sorted(xs)[len(xs) // 2]
    col = lambda arm, key: [r[arm][key] for r in rounds]
    out = {
        "tool": "tools/stream_latency.py --utts", "utts": n, "weight_dtype": opt.weight_dtype,
        "shape": f"830M LM, full codec (8,5,4,2), {n} samples x CFG of the 160-frame demo prompt, 67 phonemes, sampled, CFG stride 5",
        "rounds": rounds,
        "median": {k: round(med(col(arm, key)), 2) for k, arm, key in (
            ("one_pass_total_ms", "one_pass", "total_ms"), ("one_pass_lm_ms", "one_pass", "lm_ms"), ("one_pass_render_ms", "one_pass", "render_ms"),
            ("stream_total_ms", "stream", "total_ms"), ("stream_first_chunk_first_utt_ms", "stream", "first_chunk_first_utt_ms"),
            ("stream_first_chunk_last_utt_ms", "stream", "first_chunk_last_utt_ms"))},
        "spread": {"one_pass_total_ms": round(max(col("one_pass", "total_ms")) - min(col("one_pass", "total_ms")), 2),
                   "stream_total_ms": round(max(col("stream", "total_ms")) - min(col("stream", "total_ms")), 2)},
        "max_abs_diff": max(col("stream", "max_abs_diff")),
    }
    line = json.dumps(out)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


def batched_watermarked(opt, model, tok, call):
    """--utts N --use_watermark: `inference_samples_wmstream` against `inference_samples(use_watermark=True)`"""
    from ssr_speech_amd.codec.wmencodec import BatchWMDecodeStream, wm_stream_holdback
    n, codec = opt.utts, tok.codec
    call_wm = call[:13] + (True,) + call[14:]
    seen = {"polls": [], "tap_bytes": None, "rows": None}
    real_advance = BatchWMDecodeStream.advance

    def counted(self, new_frames, ended, *a, **k):
        n0, o0, live = codec.n_launches, self.ops.launches, not any(self.ended) and not any(ended)
        out = real_advance(self, new_frames, ended, *a, **k)
        seen["polls"].append((live, codec.n_launches - n0, self.ops.launches - o0))
        seen["tap_bytes"], seen["rows"] = self.tap_bytes, self.rows
        return out

    def one_pass(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        waves = inference_samples(*call_wm, seeds=list(range(seed, seed + n)))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return waves, dict(total_ms=1000 * (t1 - t0), frames=[int(w.shape[-1]) // 320 for w in waves], audio_s=sum(w.shape[-1] for w in waves) / 16000.0)

    def streamed(seed):
        torch.cuda.synchronize()
        seen["polls"] = []
        n0 = codec.n_launches
        t0 = time.perf_counter()
        parts, first = [[] for _ in range(n)], {}
        for i, chunk in inference_samples_wmstream(*call_wm, seeds=list(range(seed, seed + n))):
            if i not in first and (not first or len(first) == n - 1):      # the first chunk of the first and of the last utterance
                torch.cuda.current_stream().synchronize()
            first.setdefault(i, 1000 * (time.perf_counter() - t0))
            parts[i].append(chunk)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        waves = [torch.cat(p, -1) for p in parts]
        live = [p for p in seen["polls"] if p[0]]
        return waves, dict(total_ms=1000 * (t1 - t0), first_chunk_ms=[round(first[i], 2) for i in range(n)],
                           first_chunk_first_utt_ms=min(first.values()), first_chunk_last_utt_ms=max(first.values()),
                           first_chunk_samples=int(parts[0][0].shape[-1]), chunks=sum(len(p) for p in parts), polls=len(seen["polls"]),
                           codec_launches=codec.n_launches - n0, live_poll_calls=sorted({p[1] for p in live}),
                           live_poll_row_op_launches=sorted({p[2] for p in live}), audio_s=sum(w.shape[-1] for w in waves) / 16000.0)

    BatchWMDecodeStream.advance = counted
    try:
        one_pass(1)
        streamed(1)
        rounds = []
        for r in range(opt.rounds):
            wa, a = one_pass(1 + 100 * r)
            wb, b = streamed(1 + 100 * r)
            b["max_abs_diff"] = max(float((x - y).abs().max()) if x.shape == y.shape else float("inf") for x, y in zip(wa, wb))
            rounds.append({"one_pass": a, "wmstream": b})
    finally:
        BatchWMDecodeStream.advance = real_advance
    med = lambda xs: sorted(xs)[len(xs) // 2]
    col = lambda arm, key: [r[arm][key] for r in rounds]
    out = {
        "tool": "tools/stream_latency.py --utts --use_watermark", "utts": n, "weight_dtype": opt.weight_dtype,
        "shape": f"830M LM, full codec (8,5,4,2), {n} samples x CFG of the 160-frame demo prompt, 67 phonemes, sampled, CFG stride 5, watermarked decode",
        "rounds": rounds,
        "median": {k: round(med(col(arm, key)), 2) for k, arm, key in (
            ("one_pass_total_ms", "one_pass", "total_ms"), ("wmstream_total_ms", "wmstream", "total_ms"),
            ("wmstream_first_chunk_first_utt_ms", "wmstream", "first_chunk_first_utt_ms"),
            ("wmstream_first_chunk_last_utt_ms", "wmstream", "first_chunk_last_utt_ms"))},
        "median_first_chunk_ms_per_utt": [round(med([r["wmstream"]["first_chunk_ms"][i] for r in rounds]), 2) for i in range(n)],
        "spread": {"one_pass_total_ms": round(max(col("one_pass", "total_ms")) - min(col("one_pass", "total_ms")), 2),
                   "wmstream_total_ms": round(max(col("wmstream", "total_ms")) - min(col("wmstream", "total_ms")), 2)},
        "library_calls_per_live_poll": rounds[-1]["wmstream"]["live_poll_calls"],
        "row_op_launches_per_live_poll": rounds[-1]["wmstream"]["live_poll_row_op_launches"],
        "tap_buffer_bytes": seen["tap_bytes"], "rows_per_item": seen["rows"], "holdback_frames": wm_stream_holdback(codec.cfg),
        "max_abs_diff": max(col("wmstream", "max_abs_diff")),
    }
    line = json.dumps(out)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
