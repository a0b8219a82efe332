"""`SSR_Speech` — drop-in for the reference's `models.ssr.SSR_Speech` on the inference path
(reference `models/ssr.py:88-812`): same constructor (`args` Namespace or `config` dict), same
`state_dict` keys, same `inference(...)` signature and 4-tuple return.  The arithmetic runs in
libssrhip.so (hand-written HIP for gfx950); this file holds only host orchestration.

There is no CPU fallback: `inference` raises if the HIP library or a GPU is missing.
`forward(batch)` (the training loss, models/ssr.py:280-379) is outside this package's scope and raises; `score(batch)` returns the
same numbers (loss, top-10 accuracy, token counts) for evaluation, without autograd.
"""
from __future__ import annotations

import copy
import ctypes as C
import logging
import os
import time
from argparse import Namespace
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .. import layout as LY
from .. import score as SC
from ..engine import (DEFAULT_GROUP_ROWS, KV16_MAX_PAGES, KV_DTYPES, MAX_ROWS, PAIR_FORMS, SAMPLING_RNGS, STREAMS, WEIGHT_DTYPES, DecodeEngine,
                      DecodeKnobs, DecodePlan, LMWeightsArena, PhiloxNoise, TorchCpuNoiseFeed, resolve_decode_plan, resolve_sampling_rng)
from ..weights import lm_param_specs

TokenLogprobs = LY.TokenLogprobs          # the fifth element of `inference(..., return_logprobs=True)` results


class EngineKey(NamedTuple):
    """What `SSR_Speech._get_engine` files a DecodeEngine under: its plan (built as the engine builds it, so every switch the plan reads
    is part of the key), its shape and its capacities. `pool`: the KV pages the engine holds — of a request, the pages it needs;
    `exact_pool`: the pool an engine built for this request gets."""
    plan: DecodePlan
    n_utt: int
    use_cfg: bool
    debug: bool
    page_order: Optional[tuple]
    cap_seq: int
    cap_steps: int
    pool: int
    exact_pool: int

    def covers(self, want: "EngineKey") -> bool:
        """Does the engine filed under this key serve the request `want`? The same decisions and shape, and capacities that cover it.
        `max_pages` follows the capacity and `kv_dtype` may (a bf16 cache has a page cap): an engine built larger serves as it was built.
        A caller-chosen page order (tests) pins the pool size exactly."""
        same = lambda k: (k.plan._replace(max_pages=0, kv_dtype=""), k.n_utt, k.use_cfg, k.debug, k.page_order)
        return same(self) == same(want) and self.cap_seq >= want.cap_seq and self.cap_steps >= want.cap_steps \
            and (self.pool >= want.pool if want.page_order is None else self.pool == want.exact_pool)


def engine_key(weight_dtype: str, n_layers: int, kv_default: str, n_utt: int, use_cfg: bool, cap_seq: int, cap_steps: int, env,
               need_pages: Optional[int] = None, share_prompt: bool = False, logprobs: bool = False, debug: bool = False,
               page_order: Optional[Sequence[int]] = None) -> EngineKey:
    """The key of the engine `_get_engine` wants: the plan of an engine nobody asked anything of (every request None: the switches in
    `env` and the model's cache type decide) plus the caller's logprobs and, where the engine can serve it, prompt sharing — <= 4 rows, a
    bf16 cache or more than KV16_MAX_PAGES pages per row run unshared. Pure."""
    rows = n_utt * (2 if use_cfg else 1)
    plan = resolve_decode_plan(rows, weight_dtype, n_layers, cap_seq, env, logprobs=logprobs, kv_default=kv_default)
    if share_prompt and rows > 4 and plan.kv_dtype == "fp32" and plan.max_pages <= KV16_MAX_PAGES:
        plan = plan._replace(share_prompt=True)
    # KV pool: `need_pages` = sum over rows of the pages each row can reach (short and long utterances share one pool); never more
    # than rows x pages-per-row
    need = rows * plan.max_pages if need_pages is None else min(rows * plan.max_pages, int(need_pages))
    return EngineKey(plan, n_utt, bool(use_cfg), bool(debug), tuple(page_order) if page_order is not None else None, cap_seq, cap_steps, need,
                     min(rows * plan.max_pages, ((need + 7) // 8) * 8))


def _set_param(root: nn.Module, dotted: str, p: nn.Parameter):
    mod = root
    parts = dotted.split(".")
    for name in parts[:-1]:
        if not hasattr(mod, name):
            mod.add_module(name, nn.Module())
        mod = getattr(mod, name)
    mod.register_parameter(parts[-1], p)


class InferenceStream:
    """Iterator returned by `SSR_Speech.inference_stream`; `.result` is set when it is exhausted, `.steps_enqueued` is how many decode
    steps the engine has been given so far. From the first `next()` on, `.non_mask_intervals` holds the kept intervals on the ORIGINAL
    frame axis and `.crop` the frames dropped in front (`aug_context`): where a kept increment's frames come from
    (`inference_scale.kept_sources`)."""

    def __init__(self, model: "SSR_Speech", setup_args: tuple, use_graph: bool):
        self.model, self.result, self.steps_enqueued = model, None, 0
        self.non_mask_intervals, self.crop = None, 0
        self._it = self._run(setup_args, use_graph)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._it)

    def _run(self, setup_args, use_graph):
        m = self.model
        with torch.no_grad():
            K, held = m.args.n_codebooks, {}
            # every frame the run can release, on the device: ONE buffer, allocated ahead of the engine's first launch
            run = m._begin_inference(*setup_args, before_start=lambda n: held.update(buf=torch.empty(K * n, dtype=torch.int64, device=m.device)))
            eng, buf = run["eng"], held["buf"]
            asm = LY.FrameAssembler(run["y_np"], run["nmi"], m.args, run["out_len"] if run["aug_context"] else 0)
            self.non_mask_intervals, self.crop = list(asm.nmi), asm.out_len
            at = 0

            def on_device(incs):
                nonlocal at
                for inc in incs:
                    n = inc.codes.shape[1]
                    view = buf[K * at: K * (at + n)].view(K, n)      # contiguous: one plain host-to-device copy
                    view.copy_(torch.from_numpy(inc.codes))
                    at += n
                    yield LY.FrameIncrement(view, inc.marks, inc.kept)

            yield from on_device(asm.start())
            have, st = 0, None
            for states in eng.iter_chunks(chunk=16, use_graph=use_graph, max_total=run["cap"], feed=run["feed"]):
                st = states[0]
                self.steps_enqueued = eng._steps_enqueued
                n = int(st.n_steps)
                rows = eng.tokens(0, n, have)                   # through `tokens`: the pair-launch check guards every row that leaves
                have = n
                yield from on_device(asm.feed(rows, int(st.span), list(st.span_end)))
            self.result = m._end_inference(run, st, asm.rows)
            return self.result


class BatchFrames(NamedTuple):
    """One release of `SSR_Speech.inference_batch_stream`. `kept`: the prompts — `codes` is the list of the utterances' kept frames,
    [K, P_u] int64 on the device; else the generated frames that became final at one poll — `codes` is ONE int32 device block
    [n_utt][K][n] with utterance u's `counts[u]` new frames in its first columns (a view of a buffer the next poll overwrites).
    `ended[u]`: utterance u is complete with these frames."""
    kept: bool
    counts: List[int]
    ended: List[bool]
    codes: object


class BatchInferenceStream:
    """Iterator returned by `SSR_Speech.inference_batch_stream`; `.results` is set when it is exhausted, `.flag` is the device word the
    gather sets for an id outside [0, bins) (read it once per poll, after the poll's consumer work is enqueued:
    `BatchDecodeStream.advance(flag=)` does), `.polls` counts the polls so far."""

    def __init__(self, model: "SSR_Speech", utterances, kw: dict, use_graph: bool, bins: Optional[int], before_start, watermark: bool = False):
        a = model.args
        rows = 2 if kw["aug_text"] else 1
        # the refusals, before anything reaches the library (`watermark`: the same rules, with refusals that name the watermarked calls)
        check = LY.check_wmstream_batch if watermark else LY.check_stream_batch
        self.prompt_lens = check([int(u["y"].shape[1]) for u in utterances], [u["mask_interval"][0].detach().cpu().numpy() for u in utterances],
                                 rows, MAX_ROWS)
        self.model, self.results, self.polls, self.flag = model, None, 0, None
        self.bins = int(a.audio_vocab_size if bins is None else bins)
        self._it = self._run(utterances, kw, use_graph, before_start)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._it)

    def _run(self, utterances, kw, use_graph, before_start):
        m = self.model
        with torch.no_grad():
            K, dev, n = m.args.n_codebooks, m.device, len(utterances)
            setup = m._begin_batch(utterances, kw["top_k"], kw["top_p"], kw["temperature"], kw["stop_repetition"], kw["silence_tokens"],
                                   kw["cfg_coef"], kw["cfg_stride"], kw["aug_text"], kw["seed"], kw["first_index"], kw["indices"], n, False)
            eng, chunk = setup["eng"], 16
            # every buffer ahead of the engine's first launch: the poll's block, the range table, the flag
            block = before_start(dict(n_utt=n, K=K, prompt_lens=list(self.prompt_lens), max_new_frames=setup["cap_max"])) \
                if before_start is not None else None
            if block is None:
                block = torch.zeros(n * K * chunk, dtype=torch.int32, device=dev)
            if block.dtype != torch.int32 or block.numel() < n * K * chunk or not block.is_contiguous():
                raise ValueError("inference_batch_stream: the gather needs a contiguous int32 device buffer of n_utt * K * 16 ids")
            ranges_dev = torch.zeros(4 * n, dtype=torch.int32, device=dev)
            self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
            lib = _lib.lib()
            yield BatchFrames(True, list(self.prompt_lens), [False] * n,
                              [u["y"][0, :p].transpose(1, 0).to(dev) for u, p in zip(utterances, self.prompt_lens)])
            released, over = [0] * n, [False] * n
            it = eng.iter_queue(setup["jobs"], chunk=chunk, use_graph=use_graph, sampling=kw["top_k"] != 1)
            while True:
                try:
                    states, slot_job = next(it)
                except StopIteration as fin:
                    outs = fin.value
                    break
                self.polls += 1
                # the first fill puts job u into slot u, and a fixed group is never refilled: slot u IS utterance u until it ends
                # (a slot the queue has parked — its utterance ran into its step cap — releases nothing more and ends: `results` raises)
                parked = [not over[u] and slot_job[u] != u for u in range(n)]
                sts = [(int(states[u].n_steps), bool(states[u].span >= 1), int(states[u].span_end[0])) if not (over[u] or parked[u])
                       else (0, True, released[u] + K) for u in range(n)]
                table = LY.stream_gather_ranges(released, sts, K)
                counts = [int(table[2, u] - table[1, u]) for u in range(n)]
                ended = [bool(not over[u] and (parked[u] or states[u].done)) for u in range(n)]
                width = max(counts)
                if width:
                    ranges_dev.copy_(torch.from_numpy(table.reshape(-1)))       # pushed the way the page table is
                    _lib.check(lib.ssrhip_stream_gather(eng.generated.data_ptr(), n, int(eng.generated.shape[1]), K, table.ctypes.data,
                                                        ranges_dev.data_ptr(), block.data_ptr(), n, width, self.bins, self.flag.data_ptr(),
                                                        _lib.stream_ptr()), "ssrhip_stream_gather")
                for u in range(n):
                    released[u] += counts[u]
                    over[u] = over[u] or ended[u]
                if width or any(ended):
                    yield BatchFrames(False, counts, ended, block[: n * K * width].view(n, K, width) if width else None)
            self.results = m._batch_results(setup, outs)
            return self.results


class SSR_Speech(nn.Module):
    def __init__(self, args: Optional[Namespace] = None, config: Optional[Dict] = None):
        super().__init__()
        if args is not None and config is not None:
            raise ValueError("Cannot provide both `args` and `config`.")          # ssr.py:99-100
        if args is None:
            if config is None:
                raise ValueError("Either `args` or `config` must be provided.")  # ssr.py:109-110
            args = Namespace(**config)
        self.args = copy.copy(args)
        if not getattr(self.args, "n_special", False):                            # ssr.py:114-116
            self.args.n_special = 3
        self.args.eos = getattr(self.args, "eos", -1)
        if isinstance(self.args.audio_vocab_size, str):                           # ssr.py:118-119
            self.args.audio_vocab_size = eval(self.args.audio_vocab_size)
        a = self.args
        self.n_text_tokens = a.text_vocab_size + 1
        assert a.text_pad_token == a.text_vocab_size, f"self.args.text_vocab_size: {a.text_vocab_size}, self.args.text_pad_token: {a.text_pad_token}"
        self.n_audio_tokens = [int(a.audio_vocab_size) + a.n_special + a.max_n_spans] * a.n_codebooks
        assert a.audio_vocab_size == a.empty_token, a.empty_token                 # ssr.py:125-130
        assert a.eog == a.audio_vocab_size + 1, a.eog
        assert a.audio_pad_token == a.audio_vocab_size + 2, a.audio_pad_token
        assert a.eos == a.audio_vocab_size + 3, a.eos
        assert a.sos == a.audio_vocab_size + 4, a.sos
        assert a.mts == a.audio_vocab_size + 5, a.mts
        # parameters under the reference's names (values are placeholders until load_state_dict)
        for name, (shape, _kind) in lm_param_specs(a).items():
            _set_param(self, name, nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=False))
        self._arena: Optional[LMWeightsArena] = None
        self._engines: Dict[tuple, DecodeEngine] = {}
        self._weight_dtype = "fp32"
        self._kv_dtype = "fp32"
        self._sampling_rng = "torch_cpu"
        self.debug_logits = False          # tests: keep the per-step post-edit logits
        self.page_order = None             # tests: permutation deciding which physical KV pages the allocator hands out first
        self.last_run: dict = {}

    # ------------------------------------------------------------------ nn.Module plumbing
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        # tolerate the training-only torchmetrics states a checkpoint may carry
        sd = {k: v for k, v in state_dict.items() if not k.startswith("accuracy_metrics.")}
        out = super().load_state_dict(sd, strict=strict, **kw)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._invalidate()
        return out

    def _invalidate(self):
        for e in getattr(self, "_engines", {}).values():
            e.close()
        self._engines = {}
        self._arena = None

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def weight_dtype(self) -> str:
        return self._weight_dtype

    def set_weight_dtype(self, weight_dtype: str) -> None:
        """"bf16": the decode step's six matrix families are rounded once to bf16 (engine.LMWeightsArena) and every path — `inference`,
        `inference_stream`, `inference_batch`, `score`, `dp.*` — computes with the rounded values; engines of <= 4 rows stream them as
        2-byte weights. "e4m3": the same families are quantised once to OCP e4m3 codes with one power-of-two scale per output row
        (engine.quantize_e4m3; a COARSE format: 2.6 % relative rms rounding error of the weights against 0.17 % for bf16); every path computes
        with codes * scale, engines of <= 4 rows stream the 1-byte codes (`SSRHIP_GEMV_W8=0`: their fp32 masters), engines of 5..16 rows
        stream them when `SSRHIP_GEMVM_W8=1` opts in (engine.DecodeEngine stream_wt8; off by default, same tokens), and whatever serves a
        bf16 model's rounded weights (one-plane prefill / score, the 5..32-row streaming copies) serves these too. "fp32" (the default)
        restores today's numbers bit for bit: the arena is rebuilt from `state_dict()`. Drops the arena and the cached engines."""
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype {weight_dtype!r} not in {WEIGHT_DTYPES}")
        if weight_dtype != self._weight_dtype:
            self._weight_dtype = weight_dtype
            self._invalidate()

    @property
    def kv_dtype(self) -> str:
        return self._kv_dtype

    def set_kv_dtype(self, kv_dtype: str) -> None:
        """"bf16": decode engines of 5..32 rows — `inference_batch`, `dp.generate`, `dp.synthesize`, `run_queue` with 3 or more utterances
        under CFG — keep their KV cache in 2-byte bf16 entries (engine.DecodeEngine kv_dtype): half the cache memory and half the bytes the
        attention reads; K / V are rounded once when written, everything else stays fp32. The 2-row paths (`inference`,
        `inference_stream`) keep fp32 K / V unless `SSRHIP_ATTN_KV16_SMALL=1` opts engines of 1, 2 or 4 rows in (engine.resolve_kv16_small,
        DESIGN.md Part I.23); `score` keeps fp32 K / V. "fp32" (the default) restores today's numbers bit for bit. Independent of
        `set_weight_dtype`. Drops the cached engines."""
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype {kv_dtype!r} not in {KV_DTYPES}")
        if kv_dtype != self._kv_dtype:
            self._kv_dtype = kv_dtype
            for e in self._engines.values():
                e.close()
            self._engines = {}

    @property
    def sampling_rng(self) -> str:
        return self._sampling_rng

    def set_sampling_rng(self, sampling_rng: str) -> None:
        """Where the multinomial noise of SAMPLED runs (`top_k != 1`) comes from (DESIGN.md Part I.21). "torch_cpu" (the default): the host
        draws torch's CPU stream and uploads it beside the decode — the reference's tokens from the seed alone. "philox": a counter-based
        generator on the device (engine.PhiloxNoise, csrc/noise.hip) writes it on the decode stream from the utterance's seed — no host
        draw, no pinned staging, no copy stream; other tokens than "torch_cpu", and the batch contract by construction: result i of
        `inference_batch(seed=s)` equals `inference()` of utterance i alone after `torch.manual_seed(s + i)`, for any `group`, with and
        without refill, at any DP world size. Every path honours it — `inference`, `inference_stream`, `inference_batch`,
        `inference_batch_stream`, `inference_samples*`, `dp.generate`, `dp.synthesize`; an explicit `noise=` argument still wins; greedy runs
        ignore it. Under "philox" the CPU generator is consumed by the `aug_text` draw of the unconditional text only, so after a run it
        is NOT where the reference leaves it. A property of a run, not of an engine: nothing is dropped or rebuilt."""
        if sampling_rng not in SAMPLING_RNGS:
            raise ValueError(f"sampling_rng {sampling_rng!r} not in {SAMPLING_RNGS}")
        self._sampling_rng = sampling_rng

    def forward(self, batch):
        raise NotImplementedError("SSR_Speech.forward (training loss, reference models/ssr.py:280-379) is outside the "
                                  "scope of ssr_speech_amd: only the inference hot path is implemented. SSR_Speech.score(batch) "
                                  "returns its loss, top-10 accuracy and token counts without autograd.")

    # ------------------------------------------------------------------ engine management
    def _get_engine(self, n_utt: int, use_cfg: bool, need_seq: int, need_steps: int, need_pages: Optional[int] = None,
                    share_prompt: bool = False, logprobs: bool = False) -> DecodeEngine:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("ssr_speech_amd.SSR_Speech.inference needs the model on a ROCm GPU (model.to('cuda')); "
                               "there is no CPU path in this package.")
        if self._arena is None:
            self._arena = LMWeightsArena(self.args, self.state_dict(), dev, weight_dtype=self._weight_dtype)
        cap_seq = ((need_seq + 1023) // 1024) * 1024
        cap_steps = ((need_steps + 255) // 256) * 256
        if self._arena.ensure_positions(cap_seq):      # long text / long utterances: grow the position table (reference: extend_pe)
            for e in self._engines.values():
                e.close()
            self._engines = {}
        want = engine_key(self._arena.weight_dtype, self._arena.L, self._kv_dtype, n_utt, use_cfg, cap_seq, cap_steps, os.environ, need_pages=need_pages,
                          share_prompt=share_prompt, logprobs=logprobs, debug=self.debug_logits, page_order=self.page_order)
        # reuse: any resident engine of the same shape whose capacities cover the request (a batch of other lengths must not re-allocate
        # the pool, the noise buffer and re-capture the graph)
        for key, e in self._engines.items():
            if key.covers(want):
                return e
        for e in self._engines.values():         # one engine (KV pool) resident at a time
            e.close()
        self._engines = {}
        key, plan = want._replace(pool=want.exact_pool), want.plan
        order = None
        if self.page_order is not None:          # tests: a caller-chosen hand-out order of the physical pages
            order = [p for p in self.page_order if p < key.pool] if len(self.page_order) >= key.pool else None
        eng = DecodeEngine(self._arena, n_utt, use_cfg, cap_seq, cap_steps, debug_logits=self.debug_logits, pool_pages=key.pool, page_order=order,
                           kv_dtype=plan.kv_dtype, share_prompt=plan.share_prompt, kv16_small=plan.kv16_small, logprobs=plan.logprobs,
                           **{"stream_" + st.name: plan.stream is st for st in STREAMS}, **{pf.name: plan.pair is pf for pf in PAIR_FORMS})
        self._engines[key] = eng
        return eng

    # ------------------------------------------------------------------ teacher-forced scoring
    @torch.no_grad()
    def score(self, batch: dict, max_rows: int = 16384) -> Optional[dict]:
        """What the reference's `forward(batch)` returns (models/ssr.py:280-379), computed for evaluation: `loss`, `top10acc`,
        `top10acc_by_codebook`, `effective_ntoken` with the reference's types, on the model's device; plus `nll_by_item` [B] (cross entropy
        summed over every codebook's loss positions, unweighted) and `ntoken_by_item` [B] (their count) for rescoring.

        batch: the collated batch of data/gigaspeech.py:298-321 — x [B,S], x_lens [B], y [B,K,T] (rearranged / shifted / mask-inserted,
        padded with audio_pad_token), y_lens [B]. An empty batch returns None. The items are packed without padding rows into launches of
        at most `max_rows` rows (an item longer than that is a launch of its own); scratch memory grows with `max_rows` (DESIGN I.7).
        Top-10 hits count targets with fewer than 10 strictly larger logits: exact ties at the 10th place count as hits."""
        items = SC.validate(batch, self.args)          # ValueError before anything reaches the device
        if items is None:
            return None
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("ssr_speech_amd.SSR_Speech.score needs the model on a ROCm GPU (model.to('cuda')); "
                               "there is no CPU path in this package.")
        if self._arena is None:
            self._arena = LMWeightsArena(self.args, self.state_dict(), dev, weight_dtype=self._weight_dtype)
        a = self._arena
        B, K = len(items), a.K
        work = [it for it in items if it.n_scored > 0]                      # an item with y_len < 2 has no scored position
        longest = max([max(it.text.shape[0], it.audio.shape[1]) for it in work], default=0)
        if a.ensure_positions(longest + 1):            # long items: grow the position table, and drop the engines built on the old one
            for e in self._engines.values():
                e.close()
            self._engines = {}
        a.ensure_split_planes()
        a.ensure_head_split_planes()
        lib = _lib.lib()
        dims = a.dims()
        w = a.c_struct()
        keep = dict(a._arrays)
        chunks = SC.plan_chunks([it.rows for it in work], max_rows)
        nlls, ranks, tgts = [], [], []
        f32 = dict(dtype=torch.float32, device=dev)
        ldc = (a.card + 3) // 4 * 4
        hd = a.D // a.H
        ws = None
        for ch in chunks:
            pk = SC.pack_items([work[i] for i in ch], K)
            R, M, S = int(pk["tok"].shape[0]), int(pk["target"].shape[1]), len(ch)
            Rc = max(R, ws["R"] if ws is not None else 0)
            if ws is None or ws["R"] < R:
                ws = dict(R=Rc, x=torch.empty(Rc, a.D, **f32), xn=torch.empty(Rc, a.D, **f32), qkv=torch.empty(Rc, 3 * a.D, **f32),
                          o=torch.empty(Rc, a.D, **f32), h=torch.empty(Rc, a.F, **f32))
            hc = min(M, 4096)
            if ws.get("hc", 0) < hc:
                ws.update(hc=hc, head_h=torch.empty(hc, K * a.Hh, **f32), logits=torch.empty(hc, ldc, **f32))
            npg = int(pk["n_pages"])
            if ws.get("pages", 0) < npg:
                ws.update(pages=npg, pool=torch.empty(npg * 2 * a.H * _lib.PAGE * hd, **f32))
            # every integer array of the chunk in ONE host -> device copy, addressed by views
            parts = [pk[k].reshape(-1).astype(np.int32) for k in ("tok", "pos", "kind", "row_seq", "row_pos", "row_len", "seq_start", "target", "table")]
            offs = np.concatenate([[0], np.cumsum([p_.size for p_ in parts])])
            ints = torch.from_numpy(np.concatenate(parts)).pin_memory().to(dev, non_blocking=True)
            view = lambda i: ints[int(offs[i]): int(offs[i + 1])]
            nll = torch.empty(K, M, **f32)
            rank = torch.empty(K, M, dtype=torch.int32, device=dev)
            sa = _lib.ScoreArgs()
            for i, name in enumerate(("tok", "pos", "kind", "row_seq", "row_pos", "row_len", "seq_start")):
                setattr(sa, name, view(i).data_ptr())
            sa.R, sa.n_seq, sa.max_len = R, S, int(pk["max_len"])
            sa.x, sa.xn, sa.qkv, sa.o, sa.h = (ws[k].data_ptr() for k in ("x", "xn", "qkv", "o", "h"))
            sa.kv = _lib.KV(ws["pool"].data_ptr(), view(8).data_ptr(), int(pk["table"].shape[1]), 1, a.H, hd)
            first, count = np.ascontiguousarray(pk["score_first"]), np.ascontiguousarray(pk["score_count"])
            sa.score_first, sa.score_count, sa.M = first.ctypes.data, count.ctypes.data, M
            sa.target, sa.nll, sa.rank = view(7).data_ptr(), nll.data_ptr(), rank.data_ptr()
            sa.hs = ws["xn"].data_ptr()                # the final LayerNorm's output of the scored rows: xn is free after the layer loop
            sa.head_h, sa.logits, sa.head_chunk = ws["head_h"].data_ptr(), ws["logits"].data_ptr(), hc
            if getattr(a, "_hs_ready", False):
                sa.head1_ws, sa.head2_ws = a.head1_ws.data_ptr(), a.head2_ws.data_ptr()
            # the plane count of the arena's buffers picks the entry: a one-plane buffer must never reach the three-plane one
            entry = "ssrhip_lm_score_w1" if a.split_planes == 1 else "ssrhip_lm_score"
            _lib.check(getattr(lib, entry)(C.byref(dims), C.byref(w), C.byref(sa), _lib.stream_ptr()), entry)
            nlls.append(nll)
            ranks.append(rank)
            tgts.append(view(7).view(K, M))
        del keep
        idx = SC.scored_index(work)
        if nlls:
            nll, rank, tgt = torch.cat(nlls, 1), torch.cat(ranks, 1), torch.cat(tgts, 1)
        else:
            nll, rank, tgt = torch.zeros(K, 0, **f32), torch.zeros(K, 0, dtype=torch.int32, device=dev), torch.zeros(K, 0, dtype=torch.int32, device=dev)
        out = SC.reduce(nll, rank, tgt, torch.from_numpy(idx["item"]).to(dev), torch.from_numpy(idx["pos"]).to(dev), B, self.args)
        self.last_score = dict(chunks=len(chunks), rows=sum(it.rows for it in work), scored_rows=int(nll.shape[1]), nll=nll, rank=rank)
        return out

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def inference(
        self,
        x: torch.Tensor,
        x_lens: torch.Tensor,
        prompt_x: torch.Tensor,
        prompt_x_lens: torch.Tensor,
        y: torch.Tensor,
        prompt: torch.Tensor,
        mask_interval: List[torch.Tensor],
        top_k: int = -100,
        top_p: float = 1.0,
        temperature: float = 1.0,
        stop_repetition: int = -1,
        kvcache: int = 1,
        silence_tokens: List[int] = [1388, 1898, 131],
        cfg_coef: float = 1.5,
        cfg_stride: int = 1,
        aug_text: bool = False,
        aug_context: bool = False,
        cfg_pretrained: bool = False,
        *,
        noise: Optional[torch.Tensor] = None,
        uncond_x: Optional[torch.Tensor] = None,
        max_new_steps: Optional[int] = None,
        use_graph: bool = True,
        return_logprobs: bool = False,
    ):
        """Same contract as the reference's `SSR_Speech.inference` (models/ssr.py:504-812).

        `kvcache` is accepted and ignored (the engine always keeps a paged KV cache; the reference
        produces identical tokens for kvcache 0/1).  Keyword-only extras (not in the reference):
        `noise` [steps,K,card] Exp(1) draws replacing the multinomial generator draw, `uncond_x`
        overriding the random CFG text (ssr.py:574), `max_new_steps` (tests), `use_graph`, and
        `return_logprobs` (DESIGN.md Part I.27): the result is the same 4-tuple plus a fifth element,
        `layout.TokenLogprobs` — the log-probability of every generated token, per step and aligned
        with `res`, NaN where the state machine decided the token. Same tokens, bit for bit; the
        decode engine of such a call is built with `logprobs=True` (a model that never asks never
        builds one). The streaming iterators and `dp.generate` do not take the keyword."""
        run = self._begin_inference(x, x_lens, prompt_x, prompt, y, mask_interval, top_k, top_p, temperature, stop_repetition, silence_tokens,
                                    cfg_coef, cfg_stride, aug_text, aug_context, cfg_pretrained, noise, uncond_x, max_new_steps,
                                    logprobs=return_logprobs)
        eng = run["eng"]
        states = eng.run_to_completion(chunk=16, use_graph=use_graph, max_total=run["cap"], feed=run["feed"])
        st = states[0]
        n = int(st.n_steps)
        out = self._end_inference(run, st, eng.tokens(0, n))
        if not return_logprobs or out is None:
            return out
        return out + (LY.assemble_logprobs(eng.logprobs(0, n), [st.span_end[i] for i in range(run["num_task"])], run["y_np"].shape[1], run["nmi"],
                                           run["out_len"] if run["aug_context"] else 0),)

    def _begin_inference(self, x, x_lens, prompt_x, prompt, y, mask_interval, top_k, top_p, temperature, stop_repetition, silence_tokens,
                         cfg_coef, cfg_stride, aug_text, aug_context, cfg_pretrained, noise, uncond_x, max_new_steps, before_start=None,
                         logprobs: bool = False) -> dict:
        """Everything `inference` does before the decode loop (shared with `inference_stream`): argument checks, prompt layout, engine,
        prefill. `before_start(n)` is called ahead of the engine's first launch with the most frames the result can have. Returns what
        the loop and `_end_inference` need."""
        t_call = time.perf_counter()
        K = self.args.n_codebooks
        assert cfg_coef >= 1.0, cfg_coef
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3, y.shape
        y = y.transpose(2, 1)
        assert prompt.ndim == 3, prompt.shape
        prompt = prompt.transpose(2, 1)
        assert y.shape[0] == 1 and y.shape[1] == K, y.shape
        assert prompt.shape[0] == 1 and prompt.shape[1] == K, prompt.shape
        assert mask_interval.shape == torch.Size((1, mask_interval.shape[1], 2)), mask_interval
        # ssr.py:563-568: the context is prepended only when the masked spans are short (< 2 s at 50 Hz)
        context_len = int(sum(int(item[1] - item[0]) for item in mask_interval[0]))
        aug_context = bool(aug_context and context_len < 2 * 50)

        x_np = x.detach().cpu().numpy().astype(np.int64)
        y_np = y[0].detach().cpu().numpy().astype(np.int64)
        mi = mask_interval[0].detach().cpu().numpy().astype(np.int64)
        out_len = 0
        if aug_context:
            # ssr.py:578-594, 607-608: [prompt text ‖ text], [prompt codes ‖ codes], spans shifted by the prompt length
            assert prompt_x.ndim == 2, prompt_x.shape
            out_len = int(prompt.shape[2])
            x_np = np.concatenate([prompt_x.detach().cpu().numpy().astype(np.int64), x_np], axis=1)
            y_np = np.concatenate([prompt[0].detach().cpu().numpy().astype(np.int64), y_np], axis=1)
            mi = mi + out_len
        L = x_np.shape[1]
        text_rows = [x_np[0]]
        if aug_text:
            if cfg_pretrained:
                # ssr.py:576/587 + :631-634: the unconditional row is `text_vocab_size-1` repeated L times with text keys 1..L-1
                # padded out for every query. Those positions are then attended by nothing and their own outputs are dropped
                # (:275-276), and text / audio positions are embedded independently (:599-600, :662), so the row is exactly
                # the length-1 text [text_vocab_size-1] — the engine's rows carry their own text length.
                text_rows.append(np.asarray([int(self.args.text_vocab_size) - 1], dtype=np.int64))
            else:
                if uncond_x is None:
                    # drawn from the global CPU generator, before any sampling draw — exactly ssr.py:574/585
                    uncond_x = torch.randint(0, self.n_text_tokens, (1, L))
                text_rows.append(uncond_x.detach().cpu().numpy().astype(np.int64)[0])
        cated, mask_position, num_task, nmi = LY.build_layout(y_np, mi, self.args)
        T0 = cated.shape[1]
        # upper bound on steps: every span stops at the latest when y_len > 10*L (ssr.py:739) + K eog steps
        cap = max(10 * L + 2 - T0, 1) + num_task * (K + 1)
        if max_new_steps is not None:
            cap = min(cap, max_new_steps)
        eng = self._get_engine(1, bool(aug_text), L + T0 + cap + 8, cap, logprobs=logprobs)
        knobs = DecodeKnobs(top_k=top_k, top_p=top_p, temperature=temperature, stop_repetition=stop_repetition,
                            silence_tokens=tuple(int(s) for s in silence_tokens), cfg_coef=cfg_coef, cfg_stride=cfg_stride,
                            use_cfg=bool(aug_text), text_len=L, n_spans=num_task, seed=int(torch.initial_seed()))
        if before_start is not None:
            before_start(y_np.shape[1] + cap)
        greedy = top_k == 1
        feed = None
        if noise is not None:
            eng.start(text_rows, [cated], [knobs], noise=noise.to(torch.float32).unsqueeze(0))
        elif not greedy:
            # reproduce the reference's CPU sampling stream: torch.multinomial(probs[K,card], 1) draws one Exp(1) tensor of that
            # shape per step from the global generator (after the uncond_x draw above) — streamed in 16 steps at a time beside the decode
            # ... or, under sampling_rng "philox", written on the device from knobs.seed, 16 steps at a time on the decode stream
            feed = PhiloxNoise([knobs.seed]) if resolve_sampling_rng(None, self._sampling_rng) == "philox" else TorchCpuNoiseFeed([None], K, eng.a.card)
            eng.start(text_rows, [cated], [knobs], host_noise=True)
        else:
            eng.start(text_rows, [cated], [knobs])
        return dict(eng=eng, feed=feed, cap=cap, y_np=y_np, nmi=nmi, num_task=num_task, out_len=out_len, aug_context=aug_context,
                    prefill_rows=(L + T0) * (2 if aug_text else 1), t_call=t_call, max_new_steps=max_new_steps)

    def _end_inference(self, run: dict, st, gen: np.ndarray):
        """What `inference` does after the decode loop: `last_run`, the not-finished cases, span re-assembly, the 4-tuple."""
        eng, cap, num_task, out_len = run["eng"], run["cap"], run["num_task"], run["out_len"]
        self.last_run = dict(steps=st.n_steps, done=st.done, span_end=list(st.span_end), prefill_rows=run["prefill_rows"],
                             t_start=run["t_call"], t_first_chunk=eng.t_first_chunk, t_end=time.perf_counter())
        if st.done != 1:
            if run["max_new_steps"] is not None:
                return None
            raise RuntimeError(f"generation did not finish within {cap} steps (done={st.done})")
        ends = [0] + [st.span_end[i] for i in range(num_task)]
        spans = [gen[ends[i]:ends[i + 1]] for i in range(num_task)]
        res, marks, masks, nmi_out = LY.assemble(run["y_np"], spans, run["nmi"], self.args)
        if run["aug_context"]:                                  # ssr.py:806-810
            res, marks = res[:, out_len:], marks[out_len:]
            masks = [(a - out_len, b - out_len) for a, b in masks]
            nmi_out = [(a - out_len, b - out_len) for a, b in nmi_out]
        res_t = torch.from_numpy(np.ascontiguousarray(res)).unsqueeze(0).to(self.device)
        marks_t = torch.from_numpy(np.ascontiguousarray(marks)).unsqueeze(0)          # CPU tensor, as the reference (ssr.py:805)
        logging.info(f"ssr_speech_amd: generated {st.n_steps} steps")
        return res_t, marks_t, masks, nmi_out

    @torch.no_grad()
    def inference_stream(self, x, x_lens, prompt_x, prompt_x_lens, y, prompt, mask_interval, top_k: int = -100, top_p: float = 1.0,
                         temperature: float = 1.0, stop_repetition: int = -1, kvcache: int = 1, silence_tokens: List[int] = [1388, 1898, 131],
                         cfg_coef: float = 1.5, cfg_stride: int = 1, aug_text: bool = False, aug_context: bool = False,
                         cfg_pretrained: bool = False, *, noise: Optional[torch.Tensor] = None, uncond_x: Optional[torch.Tensor] = None,
                         max_new_steps: Optional[int] = None, use_graph: bool = True) -> "InferenceStream":
        """`inference` that hands the result out while the decode loop still runs: an iterator of `layout.FrameIncrement`s — the frames
        of the final `res` that can no longer change, in final time order, `codes` [K, n] int64 on the model's device (views of one buffer
        allocated before the first launch) — released after every 16-step poll of the engine. Same arguments, same tokens, same use of
        the CPU generator as `inference`; after exhaustion `.result` holds the 4-tuple `inference` would have returned (it is also the
        generator's `StopIteration.value`) and `last_run` is filled the same way. Nothing runs before the first `next()`."""
        return InferenceStream(self, (x, x_lens, prompt_x, prompt, y, mask_interval, top_k, top_p, temperature, stop_repetition, silence_tokens,
                                      cfg_coef, cfg_stride, aug_text, aug_context, cfg_pretrained, noise, uncond_x, max_new_steps), use_graph)

    # ------------------------------------------------------------------ batched decode (new capability)
    @torch.no_grad()
    def inference_batch(self, utterances, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0, stop_repetition: int = -1,
                        silence_tokens=(1388, 1898, 131), cfg_coef: float = 1.5, cfg_stride: int = 1, aug_text: bool = False,
                        seed: int = 0, first_index: int = 0, group: Optional[int] = None, use_graph: bool = True, refill: bool = True,
                        indices: Optional[Sequence[int]] = None, share_prompt: bool = False, *, return_logprobs: bool = False):
        """Several independent utterances decoded in lock-step so that one pass over the weights serves all of them
        (the reference is strictly batch-1: `assert y.shape[0] == 1`, ssr.py:559, and loops `--sample_batch_size`
        sequentially, inference_v2.py:331-333).

        utterances: list of dicts {x: LongTensor[1,L], y: LongTensor[1,T,K], mask_interval: LongTensor[1,M,2]}.
        Parity contract: result i == `inference()` of utterance i alone after `torch.manual_seed(seed + first_index + i)`
        (per-utterance RNG streams, independent of grouping and of the DP world size); `indices[i]` replaces `first_index + i`
        when the list is a cost-balanced (non-contiguous) shard of a larger job (`dp.generate`).
        `refill=False` (A/B knob, bench): fixed groups of `group` utterances, each decoded until its longest member ends (round 2).
        `share_prompt=True` (opt-in, DESIGN.md Part I.15): utterances of the FIRST fill with equal text and prompt audio — the samples of
        one utterance — are prefilled once and share the prompt's KV pages (engine.DecodeEngine share_prompt); same results, bit for bit.
        Engines of <= 4 rows, or with a bf16 KV cache, run unshared without error.
        `return_logprobs=True` (keyword-only, DESIGN.md Part I.27): every result gets a fifth element, the `layout.TokenLogprobs` of that
        utterance, as in `inference`; same tokens. `inference_batch_stream` and `dp.generate` do not take the keyword.
        Returns a list of the same 4-tuples `inference` returns."""
        setup = self._begin_batch(utterances, top_k, top_p, temperature, stop_repetition, silence_tokens, cfg_coef, cfg_stride, aug_text,
                                  seed, first_index, indices, group, share_prompt, logprobs=return_logprobs)
        if setup is None:
            return []
        jobs, eng, n_slots = setup["jobs"], setup["eng"], setup["n_slots"]
        greedy = top_k == 1
        if refill:
            outs = eng.run_queue(jobs, chunk=16, use_graph=use_graph, sampling=not greedy)
            lps = list(eng.queue_logprobs)
        else:
            outs, lps = [], []
            for g0 in range(0, len(jobs), n_slots):
                outs += eng.run_queue(jobs[g0: g0 + n_slots], chunk=16, use_graph=use_graph, sampling=not greedy)
                lps += list(eng.queue_logprobs)
        return self._batch_results(setup, outs, lps if return_logprobs else None)

    def _begin_batch(self, utterances, top_k, top_p, temperature, stop_repetition, silence_tokens, cfg_coef, cfg_stride, aug_text,
                     seed, first_index, indices, group, share_prompt, logprobs: bool = False) -> Optional[dict]:
        """What `inference_batch` and `inference_batch_stream` do before the decode loop: the job list (per-utterance RNG stream, text rows,
        prompt layout, step cap), the KV page demand and the engine lookup. None for an empty list."""
        K = self.args.n_codebooks
        assert cfg_coef >= 1.0, cfg_coef
        rows = 2 if aug_text else 1
        if group is None:
            group = DEFAULT_GROUP_ROWS // rows     # 16 rows per engine pass: 8 utterances with CFG; up to 32 on request
        assert 1 <= group * rows <= MAX_ROWS, (group, rows)
        if not utterances:
            return None
        jobs, metas, page_need = [], [], []
        cap_max, seq_max = 1, 1
        for j, u in enumerate(utterances):
            gi = int(indices[j]) if indices is not None else first_index + j
            rng = torch.Generator().manual_seed(seed + gi)      # same stream as `torch.manual_seed(seed + gi)` + a batch-1 run
            x_np = u["x"].detach().cpu().numpy().astype(np.int64)
            L = x_np.shape[1]
            text_rows = [x_np[0]]
            if aug_text:
                text_rows.append(torch.randint(0, self.n_text_tokens, (1, L), generator=rng).numpy().astype(np.int64)[0])     # ssr.py:574
            y_np = u["y"][0].transpose(1, 0).detach().cpu().numpy().astype(np.int64)
            mi = u["mask_interval"][0].detach().cpu().numpy().astype(np.int64)
            cated, mask_position, num_task, nmi = LY.build_layout(y_np, mi, self.args)
            T0 = cated.shape[1]
            cap = max(10 * L + 2 - T0, 1) + num_task * (K + 1)
            cap_max, seq_max = max(cap_max, cap), max(seq_max, L + T0 + cap + 8)
            page_need.append(rows * ((L + T0 + cap + 16) // 128 + 1))      # + the 16-step chunk the allocator provisions ahead
            kn = DecodeKnobs(top_k=top_k, top_p=top_p, temperature=temperature, stop_repetition=stop_repetition,
                             silence_tokens=tuple(int(s) for s in silence_tokens), cfg_coef=cfg_coef, cfg_stride=cfg_stride,
                             use_cfg=bool(aug_text), text_len=L, n_spans=num_task, seed=seed + gi)
            jobs.append(dict(text_rows=text_rows, audio_cols=cated, knobs=kn, gen=rng, cap=cap, rng=self._sampling_rng))
            metas.append((y_np, nmi, num_task))
        # Utterance slots of ONE engine, refilled as utterances finish (continuous batching): a finished utterance's rows take the next
        # pending utterance at the following 16-step poll instead of idling until the longest member of a fixed group ends.
        n_slots = min(group, len(jobs))
        while n_slots * rows == 3:                 # 3 rows is the one unsupported count: one more slot (it stays idle when there is no job for it)
            n_slots += 1
        # KV pool: at most n_slots utterances are resident at a time -> the n_slots largest page demands bound the concurrent need
        pages_sum = sum(sorted(page_need, reverse=True)[:n_slots])
        eng = self._get_engine(n_slots, bool(aug_text), seq_max, cap_max + 16, need_pages=pages_sum, share_prompt=share_prompt, logprobs=logprobs)
        return dict(jobs=jobs, metas=metas, n_slots=n_slots, eng=eng, cap_max=cap_max)

    def _batch_results(self, setup: dict, outs, lps=None) -> list:
        """The 4-tuples `inference_batch` returns, from what `DecodeEngine.run_queue` returns; with `lps` (the engine's `queue_logprobs`,
        one array per job) each gets its `TokenLogprobs` as a fifth element."""
        jobs, metas, dev = setup["jobs"], setup["metas"], self.device
        results = []
        for j, (st, gen) in enumerate(outs):
            if st.done != 1:
                raise RuntimeError(f"utterance {j} did not finish within {jobs[j]['cap']} steps (done={st.done})")
            y_np, nmi, num_task = metas[j]
            ends = [0] + [st.span_end[i] for i in range(num_task)]
            spans = [gen[ends[i]:ends[i + 1]] for i in range(num_task)]
            res, marks, masks, nmi_out = LY.assemble(y_np, spans, nmi, self.args)
            out = (torch.from_numpy(res).unsqueeze(0).to(dev), torch.from_numpy(marks).unsqueeze(0), masks, nmi_out)
            if lps is not None:
                out += (LY.assemble_logprobs(lps[j], ends[1:], y_np.shape[1], nmi),)
            results.append(out)
        return results

    @torch.no_grad()
    def inference_batch_stream(self, utterances, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0, stop_repetition: int = -1,
                               silence_tokens=(1388, 1898, 131), cfg_coef: float = 1.5, cfg_stride: int = 1, aug_text: bool = False,
                               seed: int = 0, first_index: int = 0, use_graph: bool = True, indices: Optional[Sequence[int]] = None,
                               *, bins: Optional[int] = None, before_start=None, return_logprobs: bool = False) -> "BatchInferenceStream":
        """`inference_batch` of ONE fixed lock-step group that hands the frames out while the decode loop still runs (DESIGN.md Part I.16).
        Zero-shot TTS utterances only (one generated span that ends the utterance, behind one kept interval), `n_utt x rows <= MAX_ROWS`,
        no refill; anything else is a ValueError raised before any launch. Same parity contract as `inference_batch`.

        Returns an iterator of `BatchFrames`: first the prompts (`kept`), then after every 16-step poll the generated frames of every
        utterance that can no longer change (`layout.FrameAssembler`'s rule per utterance), gathered on the device by ONE
        `ssrhip_stream_gather` launch into a [n_utt][K][n] int32 block — the tokens never visit the host. When exhausted, `.results` is
        exactly the list `inference_batch` returns. Nothing runs before the first `next()`.
        `bins`: ids outside [0, bins) are an error (default: `audio_vocab_size`). `before_start(info)` is called ahead of the engine's first
        launch with dict(n_utt, K, prompt_lens, max_new_frames); it may return the int32 device buffer to gather into
        (`BatchDecodeStream.codes`), else the stream allocates its own.
        `return_logprobs` is `inference_batch`'s keyword, here for signature parity only (this signature follows `inference_batch`'s) and
        not served: True is a ValueError naming the call to use instead. Serve it whole or not at all."""
        if return_logprobs:
            raise ValueError("the batched stream hands out frames, not log-probabilities: use inference_batch(..., return_logprobs=True)")
        return BatchInferenceStream(self, utterances, dict(top_k=top_k, top_p=top_p, temperature=temperature, stop_repetition=stop_repetition,
                                                           silence_tokens=silence_tokens, cfg_coef=cfg_coef, cfg_stride=cfg_stride,
                                                           aug_text=aug_text, seed=seed, first_index=first_index, indices=indices),
                                    use_graph, bins, before_start)

    def inference_batch_wmstream(self, utterances, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0, stop_repetition: int = -1,
                                 silence_tokens=(1388, 1898, 131), cfg_coef: float = 1.5, cfg_stride: int = 1, aug_text: bool = False,
                                 seed: int = 0, first_index: int = 0, use_graph: bool = True, indices: Optional[Sequence[int]] = None,
                                 *, bins: Optional[int] = None, before_start=None) -> "BatchInferenceStream":
        """`inference_batch_stream` for a consumer that decodes WITH the watermark (DESIGN.md Part I.29): the same iterator of
        `BatchFrames`, the same tokens and `.results`; the rules are `layout.check_wmstream_batch`'s — zero-shot TTS only, one engine
        pass, no refill — and a refusal names `inference_batch` + `render_many(use_watermark=True)`. `before_start(info)` is where
        `BatchWMDecodeStream` is created (`inference_scale.inference_batch_wmstream`)."""
        return BatchInferenceStream(self, utterances, dict(top_k=top_k, top_p=top_p, temperature=temperature, stop_repetition=stop_repetition,
                                                           silence_tokens=silence_tokens, cfg_coef=cfg_coef, cfg_stride=cfg_stride,
                                                           aug_text=aug_text, seed=seed, first_index=first_index, indices=indices),
                                    use_graph, bins, before_start, watermark=True)
