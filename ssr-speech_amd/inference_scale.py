"""`inference_one_sample` — one utterance through the whole HIP path: phonemes -> ids, prompt wav -> codec codes,
AR decode (`SSR_Speech.inference`), codes -> wav (plain or watermarked decode).

Only the positional signature and the returned tensor are the reference's (`inference_scale.py:18`, `:88`; SURVEY §8
row C1) so that `inference_v2.py`-style drivers can call it unchanged; the body is organised around three stages:

  1. `_phoneme_ids`           text -> LongTensor [1, L]                (ids missing from `phn2num` are dropped, :20-34)
  2. `_prompt_codes`          wav file -> codes [1, T, K], scale       (:36-38)
  3. `_render`                generated codes -> waveform [1, 1, n]    (:63-86), using `kept_audio_track` for the
                              watermark decoder's skip input (:67-78, pinned by tests/golden/glue_watermark.npz)
"""
from __future__ import annotations

import logging
import time
from typing import Sequence, Tuple

import torch
import torch.nn.functional as F

from .data.tokenizer import read_wav, tokenize_audio, tokenize_text

HOP = 320          # samples per codec frame at 16 kHz / 50 Hz; the reference hard-codes it (:66, :69, :76, :86)
log = logging.getLogger(__name__)


def _phoneme_ids(text_tokenizer, phn2num: dict, text: str) -> torch.Tensor:
    ids = [phn2num[p] for p in tokenize_text(text_tokenizer, text=text.strip()) if p in phn2num]
    return torch.tensor(ids, dtype=torch.long).view(1, -1)


def _prompt_codes(audio_tokenizer, audio_fn: str, n_codebooks: int) -> Tuple[torch.Tensor, object]:
    codes, scale, _emb = tokenize_audio(audio_tokenizer, audio_fn)           # [1, K, T]
    frames_first = codes.transpose(2, 1)                                     # [1, T, K] as `inference` wants it
    if frames_first.ndim != 3 or frames_first.shape[0] != 1 or frames_first.shape[2] != n_codebooks:
        raise AssertionError(tuple(frames_first.shape))
    return frames_first[..., :n_codebooks], scale


def kept_audio_track(wav: torch.Tensor, n_frames: int, kept_new: Sequence, kept_old: Sequence, hop: int = HOP) -> torch.Tensor:
    """Waveform the watermark decoder's skip-encoder sees: silence where frames were generated, the ORIGINAL audio where
    frames were kept, moved to where those frames sit in the new utterance (reference `inference_scale.py:67-78`).

    wav       [1, n] original audio, n a multiple of `hop`
    kept_new  intervals (frame units) of kept audio in the NEW frame axis   (`masks` of `SSR_Speech.inference`)
    kept_old  the same intervals in the ORIGINAL frame axis                 (`non_mask_intervals`)
    -> [1, n_frames * hop]

    Done per frame: a gather of whole hop-sized rows, so a kept interval must have the same length on both axes."""
    if wav.ndim != 2 or wav.shape[0] != 1 or wav.shape[1] % hop:
        raise ValueError(f"expected mono audio [1, k*{hop}], got {tuple(wav.shape)}")
    src = wav.reshape(-1, hop)
    track = torch.zeros(n_frames, hop, dtype=wav.dtype)
    for (new_a, new_b), (old_a, old_b) in zip(kept_new, kept_old):
        new_a, old_a = max(int(new_a), 0), max(int(old_a), 0)
        new_b, old_b = int(new_b), int(old_b)
        if new_b - new_a != old_b - old_a:
            raise ValueError(f"kept interval changed length: new [{new_a},{new_b}) vs original [{old_a},{old_b})")
        if new_b > new_a:
            track[new_a:new_b] = src[old_a:old_b]
    return track.reshape(1, n_frames * hop)


def _watermark_inputs(codes, kept_new, kept_old, audio_fn) -> torch.Tensor:
    """The skip-encoder input of `wmdecode` for one utterance (:67-78): [1, 1, frames * HOP] on the codes' device."""
    wav, _sr = read_wav(audio_fn) if isinstance(audio_fn, str) else (audio_fn, None)
    short = -wav.shape[-1] % HOP                                             # zero-extend to whole frames, like the encode side
    if short:
        wav = F.pad(wav, (0, short))
    return kept_audio_track(wav, codes.shape[-1], kept_new, kept_old).unsqueeze(0).to(codes.device)


def _render(audio_tokenizer, codes, marks, kept_new, kept_old, scale, audio_fn, use_watermark: bool) -> torch.Tensor:
    if not use_watermark:
        return audio_tokenizer.decode(codes, scale)
    return audio_tokenizer.wmdecode(codes, marks.to(codes.device), _watermark_inputs(codes, kept_new, kept_old, audio_fn), scale)


def render_many(audio_tokenizer, results: Sequence[tuple], scale, audio_fns, use_watermark: bool, tts: bool):
    """`_render` of several utterances in ONE pass of the codec per length bucket (`AudioTokenizer.decode_batch` /
    `wmdecode_batch`: items of different lengths, each with its own halo, so waveform i equals `_render` of utterance i alone).
    results[i] = the 4-tuple of `SSR_Speech.inference`; audio_fns = one path / [1, n] tensor for all, or a list with one per
    utterance (only read with `use_watermark`). For `tts` the prompt part (the first kept interval) is cut off (:85-86)."""
    if not isinstance(audio_fns, (list, tuple)):
        audio_fns = [audio_fns] * len(results)
    codes = [r[0] for r in results]
    if not use_watermark:
        waves = audio_tokenizer.decode_batch(codes, scale)
    else:
        tracks = [_watermark_inputs(c, kn, ko, fn) for (c, _m, kn, ko), fn in zip(results, audio_fns)]
        waves = audio_tokenizer.wmdecode_batch(codes, [r[1].to(r[0].device) for r in results], tracks, scale)
    if tts:
        waves = [w[..., int(r[2][0][1]) * HOP:] for w, r in zip(waves, results)]
    return waves


@torch.no_grad()
def inference_samples(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                      cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config, seeds,
                      share_prompt: bool = False, return_scores: bool = False):
    """`--sample_batch_size N` in one pass: the N samples of ONE utterance (seeds `seeds[i]`) decoded in lock-step through
    `SSR_Speech.inference_batch`, so the weights stream once per step for all of them (the reference loops them one after the
    other, `inference_v2.py:331-358`). Sample i is bit-identical to `inference_one_sample` called after
    `torch.manual_seed(seeds[i])`: the prompt is encoded once (it is the same for every sample) and every sample keeps its
    own RNG stream. `seeds` must be consecutive integers. Returns the list of waveforms [1, 1, n_i].
    `share_prompt=True` (opt-in): the samples share one prefill and the prompt's KV pages (`SSR_Speech.inference_batch`); same waveforms.
    `return_scores=True` (opt-in, DESIGN.md Part I.27): returns `(waveforms, scores)`, the same waveforms and, for sample i,
    scores[i] = dict(seed, mean_logprob, total_logprob, count, frames) — how probable the model found the tokens it drew for that sample
    (`layout.TokenLogprobs` of `inference_batch(return_logprobs=True)`; `frames` = generated frames of the sample), to rank the samples by."""
    seeds = [int(s) for s in seeds]
    assert seeds == list(range(seeds[0], seeds[0] + len(seeds))), "seeds must be consecutive (seed + sample index)"
    K = int(model_args.n_codebooks)
    target_ids = _phoneme_ids(text_tokenizer, phn2num, target_text)
    prompt_frames, scale = _prompt_codes(audio_tokenizer, audio_fn, K)
    one = {"x": target_ids, "y": prompt_frames, "mask_interval": mask_interval.unsqueeze(0)}
    t0 = time.perf_counter()
    results = model.inference_batch([one] * len(seeds), top_k=decode_config["top_k"], top_p=decode_config["top_p"],
                                    temperature=decode_config["temperature"], stop_repetition=decode_config["stop_repetition"],
                                    cfg_coef=cfg_coef, cfg_stride=cfg_stride, aug_text=aug_text, seed=seeds[0], share_prompt=share_prompt,
                                    return_logprobs=bool(return_scores))
    log.info("AR decode of %d samples in lock-step: %.3f s", len(seeds), time.perf_counter() - t0)
    # all samples through the codec in one ragged pass (they differ in length; each keeps its own halo): same waveforms as one
    # `_render` per sample, which is what the reference's loop does (inference_v2.py:331-358)
    waves = render_many(audio_tokenizer, [r[:4] for r in results], scale, audio_fn, bool(use_watermark), bool(tts))
    if not return_scores:
        return waves
    scores = [dict(seed=s_, mean_logprob=float(r[4].mean), total_logprob=float(r[4].total), count=int(r[4].count), frames=int(r[1].sum()))
              for s_, r in zip(seeds, results)]
    return waves, scores


@torch.no_grad()
def inference_one_sample(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                         cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config):
    """Positional signature of the reference (`inference_scale.py:18`). `aug_context` is accepted and — exactly as in the
    reference, which never forwards it (:42-58) — not handed to `model.inference`. Returns the waveform [1, 1, n]; for
    `tts` the prompt part (the first kept interval) is cut off (:85-86)."""
    K = int(model_args.n_codebooks)
    target_ids = _phoneme_ids(text_tokenizer, phn2num, target_text)
    prompt_ids = _phoneme_ids(text_tokenizer, phn2num, prompt_text)
    prompt_frames, scale = _prompt_codes(audio_tokenizer, audio_fn, K)
    rate = decode_config["codec_sr"]
    log.info("prompt: %d codec frames (%.2f s), %d target phonemes", prompt_frames.shape[1], prompt_frames.shape[1] / rate, target_ids.shape[1])

    t0 = time.perf_counter()
    on_dev = lambda t: t.to(device)
    result = model.inference(
        on_dev(target_ids), on_dev(torch.tensor([target_ids.shape[1]])), on_dev(prompt_ids), on_dev(torch.tensor([prompt_ids.shape[1]])),
        on_dev(prompt_frames), on_dev(prompt_frames), mask_interval=on_dev(mask_interval.unsqueeze(0)),
        top_k=decode_config["top_k"], top_p=decode_config["top_p"], temperature=decode_config["temperature"],
        stop_repetition=decode_config["stop_repetition"], kvcache=decode_config["kvcache"],
        cfg_coef=cfg_coef, cfg_stride=cfg_stride, aug_text=aug_text)
    codes, marks, kept_new, kept_old = result
    if isinstance(codes, tuple):                                             # tolerated by the reference too (:60-61)
        codes = codes[0]
    log.info("AR decode: %.3f s for %d frames (%.2f s of audio)", time.perf_counter() - t0, codes.shape[-1], codes.shape[-1] / rate)

    wave = _render(audio_tokenizer, codes, marks, kept_new, kept_old, scale, audio_fn, bool(use_watermark))
    if tts:
        wave = wave[..., int(kept_new[0][1]) * HOP:]
    return wave


@torch.no_grad()
def _stream_setup(make_codec, model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                  cfg_coef, cfg_stride, aug_text, device, decode_config):
    """What the single-utterance streams share: the codec stream `make_codec(max_frames)` — it allocates everything NOW, ahead of the
    engine's first launch — and the `SSR_Speech.inference_stream` that feeds it (nothing of it runs before its first `next()`)."""
    K = int(model_args.n_codebooks)
    target_ids = _phoneme_ids(text_tokenizer, phn2num, target_text)
    prompt_ids = _phoneme_ids(text_tokenizer, phn2num, prompt_text)
    prompt_frames, scale = _prompt_codes(audio_tokenizer, audio_fn, K)
    if scale is not None:
        raise AssertionError("renormalize=False codec: scale must be None")
    n_spans = int(mask_interval.reshape(-1, 2).shape[0])
    # the most frames the result can have: the prompt's + the decode's step cap (models/ssr.py `cap`: a span ends at the latest when the
    # audio is 10x the text, + K + 1 eog steps each)
    max_frames = int(prompt_frames.shape[1]) + 10 * int(target_ids.shape[1]) + 2 + n_spans * (K + 1)
    codec = make_codec(max_frames)
    on_dev = lambda t: t.to(device)
    frames = model.inference_stream(
        on_dev(target_ids), on_dev(torch.tensor([target_ids.shape[1]])), on_dev(prompt_ids), on_dev(torch.tensor([prompt_ids.shape[1]])),
        on_dev(prompt_frames), on_dev(prompt_frames), mask_interval=on_dev(mask_interval.unsqueeze(0)),
        top_k=decode_config["top_k"], top_p=decode_config["top_p"], temperature=decode_config["temperature"],
        stop_repetition=decode_config["stop_repetition"], kvcache=decode_config["kvcache"],
        cfg_coef=cfg_coef, cfg_stride=cfg_stride, aug_text=aug_text)
    return codec, frames


@torch.no_grad()
def inference_one_sample_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                                cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config):
    """`inference_one_sample` as a generator of waveform chunks [1, 1, n] (views of one buffer), handed out while the AR decode still
    runs: `SSR_Speech.inference_stream` releases the frames that are final after every 16-step poll, `AudioTokenizer.decode_stream`
    turns them into samples. The concatenation of the chunks is bit-identical to `inference_one_sample` with the same inputs and seed.
    For `tts` the prompt (the first kept interval) only warms the codec's LSTM state up and is never yielded. The watermarked decode is
    streamed by `inference_one_sample_wmstream`; here `use_watermark=True` raises ValueError."""
    if use_watermark:
        raise ValueError("inference_one_sample_stream: the watermarked decode (use_watermark=True) is streamed by inference_one_sample_wmstream")
    codec, frames = _stream_setup(audio_tokenizer.decode_stream, model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text,
                                  target_text, mask_interval, cfg_coef, cfg_stride, aug_text, device, decode_config)
    first = True
    for inc in frames:
        # the first increment is the first kept interval: for `tts` the prompt, which `inference_one_sample` cuts off (:85-86)
        chunk = codec.push(inc.codes.unsqueeze(0), emit=not (tts and first and inc.kept))
        first = False
        if chunk.shape[-1]:
            yield chunk
    if frames.result is None:
        raise RuntimeError("generation did not finish")
    chunk = codec.finish()
    if chunk.shape[-1]:
        yield chunk


def kept_sources(non_mask_intervals: Sequence, crop: int = 0) -> list:
    """The frames of the ORIGINAL audio under the kept `FrameIncrement`s of a stream, in their order: the i-th kept interval is
    `non_mask_intervals[i]` — the mapping of `kept_audio_track`, which reads the result's intervals: shifted by the `aug_context` crop and
    cut at 0. An empty interval releases no increment and has no entry."""
    out = []
    for s, e in non_mask_intervals:
        s, e = max(int(s) - int(crop), 0), int(e) - int(crop)
        if e > s:
            out.append((s, e))
    return out


@torch.no_grad()
def inference_one_sample_wmstream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                                  cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config):
    """`inference_one_sample(..., use_watermark=True)` as a generator of waveform chunks [1, 1, n] (views of one buffer), handed out while
    the AR decode still runs, for zero-shot TTS and for speech edits: `AudioTokenizer.wmdecode_stream` is pushed every increment's
    codes and marks and, under a kept increment, the original audio of that kept interval (`kept_sources`; silence under generated
    frames) — the rows `kept_audio_track` would put there. The concatenation of the chunks is bit-identical to `inference_one_sample`
    with the same inputs and seed. A falsy `use_watermark` is `inference_one_sample_stream`."""
    if not use_watermark:
        yield from inference_one_sample_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text,
                                               mask_interval, cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config)
        return
    codec, frames = _stream_setup(audio_tokenizer.wmdecode_stream, model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn,
                                  prompt_text, target_text, mask_interval, cfg_coef, cfg_stride, aug_text, device, decode_config)
    # the original audio, zero-extended to whole frames as `_watermark_inputs` extends it: uploaded once, ahead of the first launch
    wav, _sr = read_wav(audio_fn) if isinstance(audio_fn, str) else (audio_fn, None)
    short = -wav.shape[-1] % HOP
    if short:
        wav = F.pad(wav, (0, short))
    orig = wav.reshape(1, 1, -1).to(audio_tokenizer.device, torch.float32)
    sources, first = None, True
    for inc in frames:
        if sources is None:
            sources = iter(kept_sources(frames.non_mask_intervals, frames.crop))
        audio, n = None, int(inc.codes.shape[-1])
        if inc.kept:
            s, e = next(sources, (0, 0))
            if e - s != n:
                raise ValueError(f"kept interval changed length: {n} frames released for the original frames [{s},{e})")
            audio = orig[..., s * HOP: e * HOP]
        chunk = codec.push(inc.codes.unsqueeze(0), torch.as_tensor(inc.marks, dtype=torch.int32), audio, emit=not (tts and first and inc.kept))
        first = False
        if chunk.shape[-1]:
            yield chunk
    if frames.result is None:
        raise RuntimeError("generation did not finish")
    chunk = codec.finish()
    if chunk.shape[-1]:
        yield chunk


def _orig_audio(audio_fn, device) -> torch.Tensor:
    """The original audio under a prompt, zero-extended to whole frames as `_watermark_inputs` extends it, on the device: [n]"""
    wav, _sr = read_wav(audio_fn) if isinstance(audio_fn, str) else (audio_fn, None)
    short = -wav.shape[-1] % HOP
    if short:
        wav = F.pad(wav, (0, short))
    return wav.reshape(-1).to(device, torch.float32)


def _stream_batch(model, audio_tokenizer, utterances, cfg_coef, cfg_stride, aug_text, decode_config, seed, audio_fns=None):
    """The batched stream behind `inference_batch_stream` / `inference_samples_stream` and their watermarked twins:
    `SSR_Speech.inference_batch_stream` gathers every poll's final frames on the device into the codec stream's own block,
    `BatchDecodeStream.advance` turns them into samples. `audio_fns` (one path / [1, n] tensor per utterance): the watermarked decode —
    `SSR_Speech.inference_batch_wmstream` feeds a `BatchWMDecodeStream`, whose prompts take the original audio beside their codes."""
    held = {}
    wm = audio_fns is not None

    def before_start(info):
        # the codec stream allocates everything NOW, ahead of the engine's first launch; the gather writes straight into its block
        make = audio_tokenizer.wmdecode_stream_batch if wm else audio_tokenizer.decode_stream_batch
        held["codec"] = make(info["prompt_lens"], info["max_new_frames"])
        if wm:                                                               # the original audio: uploaded once, here; one upload per file
            up, held["audio"] = {}, []
            for fn, p in zip(audio_fns, info["prompt_lens"]):
                key = fn if isinstance(fn, str) else id(fn)
                if key not in up:
                    up[key] = _orig_audio(fn, audio_tokenizer.device)
                held["audio"].append(up[key][: p * HOP])
        return held["codec"].codes

    start = model.inference_batch_wmstream if wm else model.inference_batch_stream
    frames = start(utterances, top_k=decode_config["top_k"], top_p=decode_config["top_p"],
                   temperature=decode_config["temperature"], stop_repetition=decode_config["stop_repetition"],
                   cfg_coef=cfg_coef, cfg_stride=cfg_stride, aug_text=aug_text, seed=seed,
                   bins=int(audio_tokenizer.codec.cfg.bins), before_start=before_start)
    for inc in frames:
        codec = held["codec"]
        if inc.kept:
            # the prompts only warm the LSTM state up: never yielded
            codec.push_prompts(inc.codes, held["audio"]) if wm else codec.push_prompts(inc.codes)
            continue
        # the flag is read once per poll, after the poll's codec work is enqueued, and raises before any sample of the poll leaves
        for i, chunk in enumerate(codec.advance(inc.counts, inc.ended, flag=frames.flag)):
            if chunk.shape[-1]:
                yield i, chunk
    if frames.results is None:
        raise RuntimeError("generation did not finish")


@torch.no_grad()
def inference_batch_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, utterances, cfg_coef, cfg_stride, aug_text,
                           use_watermark, device, decode_config, seed: int = 0):
    """Zero-shot TTS of several utterances decoded in lock-step AND streamed (DESIGN.md Part I.16): a generator of
    `(index, chunk [1, 1, n])` — waveform chunks of utterance `index`, views of one buffer, handed out after every 16-step poll of the
    engine while the group still decodes. utterances[i] = {audio_fn, target_text}: the prompt is the whole file, as `--tts` passes it.
    Per utterance the concatenated chunks are `inference_one_sample(..., tts=True)` under `torch.manual_seed(seed + i)` (same tokens;
    samples within the bound that holds a batched codec pass to the batch-1 one). The prompt is never yielded. One fixed group:
    `len(utterances) x rows <= 32`, no refill; speech edits, a larger group and `use_watermark=True` are ValueErrors that name
    `inference_batch` + `render_many`, raised before any launch."""
    if use_watermark:
        raise ValueError("inference_batch_stream: the watermarked decode (use_watermark=True) is not streamed; use inference_batch + render_many")
    K = int(model_args.n_codebooks)
    jobs = []
    for u in utterances:
        prompt_frames, scale = _prompt_codes(audio_tokenizer, u["audio_fn"], K)
        if scale is not None:
            raise AssertionError("renormalize=False codec: scale must be None")
        T = int(prompt_frames.shape[1])
        jobs.append({"x": _phoneme_ids(text_tokenizer, phn2num, u["target_text"]), "y": prompt_frames,
                     "mask_interval": torch.tensor([[[T, T]]], dtype=torch.long)})
    yield from _stream_batch(model, audio_tokenizer, jobs, cfg_coef, cfg_stride, aug_text, decode_config, seed)


@torch.no_grad()
def inference_samples_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                             cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config, seeds):
    """`inference_samples` as a generator of `(sample index, chunk [1, 1, n])`: the N samples of ONE utterance decoded in lock-step and
    streamed (`inference_batch_stream`). Sample i's concatenated chunks are `inference_one_sample` after `torch.manual_seed(seeds[i])`.
    `--tts` only: a speech edit, `use_watermark=True` or more samples than one engine pass holds raise ValueError before any launch."""
    if use_watermark:
        raise ValueError("inference_samples_stream: the watermarked decode (use_watermark=True) is not streamed; use inference_samples")
    if not tts:
        raise ValueError("inference_samples_stream: only zero-shot TTS (--tts) is streamed; use inference_samples for a speech edit")
    seeds = [int(s) for s in seeds]
    assert seeds == list(range(seeds[0], seeds[0] + len(seeds))), "seeds must be consecutive (seed + sample index)"
    K = int(model_args.n_codebooks)
    prompt_frames, scale = _prompt_codes(audio_tokenizer, audio_fn, K)
    if scale is not None:
        raise AssertionError("renormalize=False codec: scale must be None")
    one = {"x": _phoneme_ids(text_tokenizer, phn2num, target_text), "y": prompt_frames, "mask_interval": mask_interval.unsqueeze(0)}
    yield from _stream_batch(model, audio_tokenizer, [one] * len(seeds), cfg_coef, cfg_stride, aug_text, decode_config, seeds[0])


@torch.no_grad()
def inference_batch_wmstream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, utterances, cfg_coef, cfg_stride, aug_text,
                             use_watermark, device, decode_config, seed: int = 0):
    """`inference_batch_stream` with the watermarked decode (DESIGN.md Part I.29): a generator of `(index, chunk [1, 1, n])` whose
    chunks, per utterance, are `inference_one_sample(..., use_watermark=True, tts=True)` under `torch.manual_seed(seed + i)` (same
    tokens; samples within the bound that holds a batched codec pass to the batch-1 one). Each utterance's original audio is uploaded
    once, ahead of the engine's first launch; `AudioTokenizer.wmdecode_stream_batch` puts it under the prompt and silence under the
    generated frames. One fixed group, zero-shot TTS only; a refusal names `inference_batch` + `render_many(use_watermark=True)`. A falsy
    `use_watermark` is `inference_batch_stream`."""
    if not use_watermark:
        yield from inference_batch_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, utterances, cfg_coef, cfg_stride, aug_text,
                                          use_watermark, device, decode_config, seed=seed)
        return
    K = int(model_args.n_codebooks)
    jobs = []
    for u in utterances:
        prompt_frames, scale = _prompt_codes(audio_tokenizer, u["audio_fn"], K)
        if scale is not None:
            raise AssertionError("renormalize=False codec: scale must be None")
        T = int(prompt_frames.shape[1])
        jobs.append({"x": _phoneme_ids(text_tokenizer, phn2num, u["target_text"]), "y": prompt_frames,
                     "mask_interval": torch.tensor([[[T, T]]], dtype=torch.long)})
    yield from _stream_batch(model, audio_tokenizer, jobs, cfg_coef, cfg_stride, aug_text, decode_config, seed,
                             audio_fns=[u["audio_fn"] for u in utterances])


@torch.no_grad()
def inference_samples_wmstream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text, mask_interval,
                               cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config, seeds):
    """`inference_samples(..., use_watermark=True)` as a generator of `(sample index, chunk [1, 1, n])`: the N samples of ONE utterance
    decoded in lock-step, watermarked and streamed (`inference_batch_wmstream`). Sample i's concatenated chunks are
    `inference_one_sample(..., use_watermark=True)` after `torch.manual_seed(seeds[i])`. `--tts` only: a speech edit or more samples
    than one engine pass holds raise ValueError before any launch. A falsy `use_watermark` is `inference_samples_stream`."""
    if not use_watermark:
        yield from inference_samples_stream(model, model_args, phn2num, text_tokenizer, audio_tokenizer, audio_fn, prompt_text, target_text,
                                            mask_interval, cfg_coef, cfg_stride, aug_text, aug_context, use_watermark, tts, device, decode_config,
                                            seeds)
        return
    if not tts:
        raise ValueError("inference_samples_wmstream: only zero-shot TTS (--tts) is streamed; use inference_samples(use_watermark=True) for a "
                         "speech edit")
    seeds = [int(s) for s in seeds]
    assert seeds == list(range(seeds[0], seeds[0] + len(seeds))), "seeds must be consecutive (seed + sample index)"
    K = int(model_args.n_codebooks)
    prompt_frames, scale = _prompt_codes(audio_tokenizer, audio_fn, K)
    if scale is not None:
        raise AssertionError("renormalize=False codec: scale must be None")
    one = {"x": _phoneme_ids(text_tokenizer, phn2num, target_text), "y": prompt_frames, "mask_interval": mask_interval.unsqueeze(0)}
    yield from _stream_batch(model, audio_tokenizer, [one] * len(seeds), cfg_coef, cfg_stride, aug_text, decode_config, seeds[0],
                             audio_fns=[audio_fn] * len(seeds))
