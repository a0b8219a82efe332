"""Host-side integer code of the decode path: prompt layout before generation and span
re-assembly after it.  Pure NumPy (index arithmetic, no loops over time steps).

Restates, vectorised:
  build_layout  <- SSR_Speech.rearrange / get_pattern_sequence / shift / insert_mask / cat_y and the
                   interval arithmetic in inference()   (reference models/ssr.py:381-436, 466-502, 604-625)
  undelay       <- revert_pattern_sequence              (models/ssr.py:438-464)
  assemble      <- the tail of inference()              (models/ssr.py:776-812)
  FrameAssembler   `assemble` in increments: the frames of the result that are already final while the decode loop still runs
and `pack_prefill_rows`, the flattened [text || audio] rows every prefill launch of the library reads; `assemble_logprobs` / `TokenLogprobs`:
`assemble` for the per-token log-probabilities of an engine built with logprobs=True.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from ._lib import MAX_CODEBOOKS


def delay_pattern(seg: np.ndarray, fill: int) -> np.ndarray:
    """[K,T] -> [K,T+K-1]: codebook q delayed by q columns, gaps = `fill` (delays=[0..K-1])."""
    K, T = seg.shape
    out = np.full((K, T + K - 1), fill, dtype=np.int64)
    for q in range(K):
        out[q, q:q + T] = seg[q]
    return out


def undelay(pattern: np.ndarray, fill: int) -> np.ndarray:
    """[K,S] -> [K,S-K+1]: inverse of delay_pattern."""
    K, S = pattern.shape
    T = S - (K - 1)
    out = np.full((K, max(T, 0)), fill, dtype=np.int64)
    for q in range(K):
        out[q] = pattern[q, q:q + T]
    return out


def intervals(y_len: int, mask_interval: np.ndarray) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """(non_mask_intervals, mask_intervals) exactly as models/ssr.py:609-616."""
    mi = [(int(a), int(b)) for a, b in np.asarray(mask_interval).reshape(-1, 2)]
    starts = [a for a, _ in mi] + [y_len]
    ends = [0] + [b for _, b in mi]
    return list(zip(ends, starts)), mi


def build_layout(y: np.ndarray, mask_interval: np.ndarray, args):
    """y [K,T] int, mask_interval [M,2] -> (cated [K,T0], mask_position, num_task, non_mask_intervals).

    Column order: kept segments (first gets <sos> in front, last gets <eos> behind) each delayed
    separately and separated by their <mts+i> token, then for every masked span <mts+i> followed by
    its delayed content + <eog>; the result is cut right before the first generation-side <mts>."""
    y = np.asarray(y, dtype=np.int64)
    K, T = y.shape
    nmi, mi = intervals(T, mask_interval)
    col = lambda v: np.full((K, 1), v, dtype=np.int64)
    segs = []
    for i, (s, e) in enumerate(nmi):
        body = y[:, s:e]
        if i == 0:
            segs.append(np.concatenate([col(args.sos), body], 1))
        elif i == len(nmi) - 1:
            segs.append(np.concatenate([body, col(args.eos)], 1))
        else:
            segs.append(body)
    for s, e in mi:
        segs.append(np.concatenate([y[:, s:e], col(args.eog)], 1))
    shifted = [delay_pattern(s, args.empty_token) for s in segs]
    n_masks = (len(shifted) - 1) // 2
    assert 2 * n_masks == len(shifted) - 1 and n_masks <= args.max_n_spans, (len(shifted), args.max_n_spans)
    mask_value = list(range(args.mts, args.mts + n_masks)) * 2
    pieces, mask_position, run = [], [], 0
    for j in range(len(shifted) - 1):
        pieces.append(shifted[j])
        run += shifted[j].shape[1]
        mask_position.append(run)
        pieces.append(col(mask_value[j]))
        run += 1
    pieces.append(shifted[-1])
    cated = np.concatenate(pieces, 1)
    num_task = len(mask_position) // 2
    return cated[:, : mask_position[num_task]], mask_position, num_task, nmi


def pack_prefill_rows(seqs, K: int) -> dict:
    """The flattened [text || audio] rows one prefill launch reads (include/ssrhip.h ssrhip_prefill_args / ssrhip_score_args), written
    ONCE for the engine's admissions and `score`. seqs: (seq_id, text ids [L], audio ids [K, T]) per sequence; a sequence's rows are
    contiguous and in position order. Returns int32 arrays: tok [R][4] (text id in column 0, the K codebooks of an audio position in
    columns 0..K-1, the rest 0), pos / kind (text 0 / audio 1, each part's sine position from 0: models/ssr.py:305-307, :205-206),
    row_seq (the row's seq_id: which page-table row its K/V go to), row_pos / row_len (position in its sequence, and how many keys it
    attends to), seq_start [n+1] (row index where each sequence starts) and lens [n]."""
    toks, poss, kinds, ids, rposs, lens = [], [], [], [], [], []
    for sid, text, audio in seqs:
        tx = np.asarray(text, dtype=np.int64).reshape(-1)
        au = np.asarray(audio, dtype=np.int64)
        L, T = tx.shape[0], au.shape[1]
        t = np.zeros((L + T, MAX_CODEBOOKS), dtype=np.int32)
        t[:L, 0] = tx
        t[L:, :K] = au.T
        toks.append(t)
        poss.append(np.concatenate([np.arange(L), np.arange(T)]).astype(np.int32))
        kinds.append(np.concatenate([np.zeros(L), np.ones(T)]).astype(np.int32))
        ids.append(np.full(L + T, sid, dtype=np.int32))
        rposs.append(np.arange(L + T, dtype=np.int32))
        lens.append(L + T)
    rpos = np.concatenate(rposs)
    return dict(tok=np.concatenate(toks), pos=np.concatenate(poss), kind=np.concatenate(kinds), row_seq=np.concatenate(ids),
                row_pos=rpos, row_len=rpos + 1, seq_start=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                lens=np.asarray(lens, dtype=np.int32))


def assemble(y: np.ndarray, spans: Sequence[np.ndarray], non_mask_intervals, args):
    """y [K,T] original codes; spans[i] [S_i,K] generated rows of span i (incl. the eog cascade).
    -> (res [K,T'], marks [T'], masks, non_mask_intervals) as models/ssr.py:776-805."""
    K = y.shape[0]
    res, marks, masks, tmp = [], [], [], 0
    for (s, e), sp in zip(non_mask_intervals, spans):
        gen = undelay(np.asarray(sp, dtype=np.int64).T, args.empty_token)[:, :-1]   # drop the eog column
        res.append(y[:, s:e])
        masks.append((tmp, tmp + e - s))
        marks += [0] * (e - s)
        res.append(gen)
        tmp += (e - s) + gen.shape[1]
        marks += [1] * gen.shape[1]
    ls, le = non_mask_intervals[-1]
    if y.shape[1] != le + 1:            # reference quirk kept verbatim (ssr.py:799)
        res.append(y[:, ls:le])
        masks.append((tmp, tmp + le - ls))
        marks += [0] * (le - ls)
    return np.concatenate(res, 1), np.asarray(marks, dtype=np.int64), masks, list(non_mask_intervals)


class TokenLogprobs(NamedTuple):
    """Per-token log-probabilities of one generated utterance (DESIGN.md Part I.27), NumPy arrays on the host. A value is the natural-log
    probability of the generated token under the softmax of the logits the sampler drew from — after the CFG combine, the special-token
    edits, the silence penalty and the temperature, before top-k / top-p — and NaN where the state machine, not the draw, decided the
    token (start-of-span delay, eog cascade, stop rule).
      steps  float32 [n_steps, K]: step order, delay pattern in place;
      frames float32 [1, K, T]: aligned with the `res` of the same result (delay pattern undone, every span where `assemble` puts it,
             the `aug_context` crop applied); NaN at kept frames. Every finite entry of `steps` is in `frames` with one exception per
             span: an eog that codebook 0 DREW (no stop rule fired) has a value in `steps`, and sits in the eog column `assemble` drops;
      count / total / mean: how many entries of `steps` are not NaN, their sum (accumulated in fp64), total / count (NaN when count == 0)
             — over `steps`, so a drawn eog is counted."""
    steps: np.ndarray
    frames: np.ndarray
    count: int
    total: float
    mean: float


def assemble_logprobs(steps: np.ndarray, span_end: Sequence[int], y_len: int, non_mask_intervals, out_len: int = 0) -> TokenLogprobs:
    """`assemble` for the per-step log-probabilities: steps [n_steps, K] in step order, span_end[i] = the step count at which span i
    ended, y_len = T of the `y` that `assemble` gets. What `assemble` does to the tokens of a span (delay pattern undone, eog column
    dropped) is done to their values; kept frames are NaN; `out_len` frames are dropped in front (the `aug_context` crop)."""
    steps = np.ascontiguousarray(np.asarray(steps, dtype=np.float32))
    K = steps.shape[1]
    nan = lambda n: np.full((K, n), np.nan, dtype=np.float32)
    ends = [0] + [int(e) for e in span_end]
    parts = []
    for i, (s, e) in enumerate(non_mask_intervals[: len(ends) - 1]):
        pat = steps[ends[i]:ends[i + 1]].T                  # [K, S]
        T = max(pat.shape[1] - (K - 1), 0)
        gen = np.stack([pat[q, q:q + T] for q in range(K)])[:, :-1] if T else nan(0)
        parts += [nan(e - s), gen]
    ls, le = non_mask_intervals[-1]
    if y_len != le + 1:                 # `assemble`'s closing segment, quirk included
        parts.append(nan(le - ls))
    frames = np.concatenate(parts, 1)[None, :, int(out_len):]
    ok = ~np.isnan(steps)
    count = int(ok.sum())
    total = float(steps[ok].astype(np.float64).sum())
    return TokenLogprobs(steps, np.ascontiguousarray(frames), count, total, total / count if count else float("nan"))


class FrameIncrement(NamedTuple):
    """Consecutive frames of the final `res`, in final time order: codes [K, n], marks [n] (0 kept / 1 generated), and whether they
    are kept (original) frames or generated ones (one increment never mixes the two)."""
    codes: np.ndarray
    marks: np.ndarray
    kept: bool


class FrameAssembler:
    """`assemble` while the spans are still being generated: fed the generated rows as they arrive, it hands out the frames of the
    final `res` that can no longer change, in final time order, and never takes one back.

      * the first kept segment is final at once (`start()`);
      * generated frame t of a span is final once the span's local rows 0 .. t+K-1 exist (codebook q of frame t sits in row t+q:
        `undelay` applied to a partial pattern) and row t's codebook 0 is not `eog` — the `eog` column is never released;
      * the kept segment behind span i is final when span i has ended;
      * the closing segment follows `assemble`'s last lines (the reference quirk included), and `out_len` frames are dropped in front
        (the `aug_context` crop of models/ssr.py:806-810).

    After the last span has ended the concatenation of everything handed out equals `assemble(...)[0]` / `[1]` (cropped by `out_len`),
    and `result()` returns the 4-tuple with `masks` / `non_mask_intervals` shifted the same way."""

    def __init__(self, y: np.ndarray, non_mask_intervals, args, out_len: int = 0):
        self.y = np.asarray(y, dtype=np.int64)
        self.K = int(self.y.shape[0])
        self.nmi = [(int(s), int(e)) for s, e in non_mask_intervals]
        self.n_spans = len(self.nmi) - 1              # `assemble` zips the intervals with the spans: one span behind each but the last
        self.eog, self.empty = int(args.eog), int(args.empty_token)
        self.out_len = int(out_len)
        self._skip = self.out_len                     # frames still to drop in front
        self._rows = np.zeros((0, self.K), dtype=np.int64)
        self._cur = 0                                 # span whose frames are being released
        self._starts = [0]                            # first row of span i
        self._rel = 0                                 # generated frames of span `_cur` released so far
        self._kept_out = False                        # the kept segment in front of span `_cur` has been released
        self._tail_out = False
        self._codes: List[np.ndarray] = []
        self._marks: List[np.ndarray] = []
        self._masks: List[Tuple[int, int]] = []
        self._tmp = 0
        self.n_released = 0                           # frames handed out (after the crop)

    @property
    def finished(self) -> bool:
        return self._tail_out

    @property
    def rows(self) -> np.ndarray:
        """every generated row fed so far, [n, K]"""
        return self._rows

    def _emit(self, out: List[FrameIncrement], codes: np.ndarray, kept: bool):
        n = codes.shape[1]
        marks = np.full(n, 0 if kept else 1, dtype=np.int64)
        self._codes.append(codes)
        self._marks.append(marks)
        drop = min(self._skip, n)
        self._skip -= drop
        if n - drop > 0:
            out.append(FrameIncrement(np.ascontiguousarray(codes[:, drop:]), marks[drop:], kept))
            self.n_released += n - drop

    def _kept(self, out, s: int, e: int):
        self._masks.append((self._tmp, self._tmp + e - s))
        self._tmp += e - s
        self._emit(out, self.y[:, s:e], True)

    def start(self) -> List[FrameIncrement]:
        """What is final before any row exists (the first kept segment; everything when there is no span)."""
        return self.feed(np.zeros((0, self.K), dtype=np.int64), 0, ())

    def feed(self, rows: np.ndarray, span: int, span_end: Sequence[int]) -> List[FrameIncrement]:
        """rows [n, K]: the generated rows that follow the ones already fed; `span`: how many spans have ended (the sampler state's
        `span`); span_end[i]: the row count at which span i ended (valid for i < span). Returns the new increments, in order."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, self.K)
        if rows.shape[0]:
            self._rows = np.concatenate([self._rows, rows], 0)
        n_rows, K = self._rows.shape[0], self.K
        out: List[FrameIncrement] = []
        while self._cur < self.n_spans:
            i = self._cur
            if not self._kept_out:
                self._kept(out, *self.nmi[i])
                self._kept_out = True
            ended = i < int(span)
            r0 = self._starts[i]
            r1 = int(span_end[i]) if ended else n_rows
            if r1 > n_rows:
                raise ValueError(f"span {i} ended at row {r1}, only {n_rows} rows were fed")
            t = self._rel
            while t + K - 1 < r1 - r0 and self._rows[r0 + t, 0] != self.eog:
                t += 1
            if t > self._rel:
                loc = self._rows[r0:r1]
                self._emit(out, np.stack([loc[q + self._rel: q + t, q] for q in range(K)]), False)
                self._tmp += t - self._rel
                self._rel = t
            if not ended:
                return out
            if self._rel != max(r1 - r0 - K, 0):
                raise ValueError(f"span {i}: {r1 - r0} rows hold {max(r1 - r0 - K, 0)} frames, {self._rel} were released")
            self._starts.append(r1)
            self._cur, self._rel, self._kept_out = i + 1, 0, False
        if not self._tail_out:
            ls, le = self.nmi[-1]
            if self.y.shape[1] != le + 1:            # reference quirk kept verbatim (ssr.py:799)
                self._kept(out, ls, le)
            self._tail_out = True
        return out

    def result(self):
        """-> (res [K, T'], marks [T'], masks, non_mask_intervals) of the finished utterance: `assemble`'s, cropped by `out_len`."""
        if not self._tail_out:
            raise RuntimeError("FrameAssembler.result() before the last span has ended")
        o = self.out_len
        res, marks = np.concatenate(self._codes, 1)[:, o:], np.concatenate(self._marks)[o:]
        return res, marks, [(a - o, b - o) for a, b in self._masks], [(a - o, b - o) for a, b in self.nmi]


# ----------------------------------------------------------------------------- the batched stream (DESIGN.md Part I.16): host arithmetic only
def check_stream_batch(y_lens: Sequence[int], mask_intervals: Sequence[np.ndarray], rows_per_utt: int, max_rows: int,
                       use_watermark: bool = False) -> List[int]:
    """Which calls `SSR_Speech.inference_batch_stream` serves: zero-shot TTS utterances — ONE generated span that ends the utterance,
    behind ONE kept interval — that fit one engine pass, decoded without the watermark. Anything else is a ValueError naming the call to
    use instead, raised before any library call. Returns the prompt lengths (frames of the kept interval)."""
    if use_watermark:
        raise ValueError("the batched stream does not run the watermarked decode (use_watermark=True): use inference_batch + render_many")
    n = len(y_lens)
    if n < 1 or n * int(rows_per_utt) > int(max_rows):
        raise ValueError(f"the batched stream decodes one fixed lock-step group: {n} utterances x {rows_per_utt} rows do not fit one engine "
                         f"pass of {max_rows} rows; use inference_batch (it refills)")
    prompts = []
    for i, (T, mi) in enumerate(zip(y_lens, mask_intervals)):
        mi = np.asarray(mi, dtype=np.int64).reshape(-1, 2)
        if mi.shape[0] != 1:
            raise ValueError(f"utterance {i}: the batched stream takes one generated span, got {mi.shape[0]} (a speech edit): use inference_batch")
        a, b = int(mi[0, 0]), int(mi[0, 1])
        if b != int(T) or not 0 <= a <= b:
            raise ValueError(f"utterance {i}: the span [{a}, {b}) does not end the utterance of {int(T)} frames (a speech edit leaves a second "
                             f"kept interval): use inference_batch")
        prompts.append(a)
    return prompts


def check_wmstream_batch(y_lens: Sequence[int], mask_intervals: Sequence[np.ndarray], rows_per_utt: int, max_rows: int) -> List[int]:
    """Which calls `SSR_Speech.inference_batch_wmstream` serves: what `check_stream_batch` accepts, decoded WITH the watermark (the
    batched watermarked stream puts silence under generated frames and labels the prompt 0, the rest 1: zero-shot TTS). The other rules
    hold — TTS only, one engine pass, no refill — and a refusal names the watermarked call to use instead. Returns the prompt lengths."""
    try:
        return check_stream_batch(y_lens, mask_intervals, rows_per_utt, max_rows)
    except ValueError as e:
        msg = str(e).replace("the batched stream", "the batched watermarked stream")
        if "watermarked" not in msg:
            msg = "the batched watermarked stream: " + msg
        raise ValueError(msg.replace("use inference_batch", "use inference_batch + render_many(use_watermark=True)")) from None


def final_generated_frames(n_rows: int, ended: bool, end_row: int, K: int) -> int:
    """How many generated frames of a ONE-span utterance are final when `n_rows` generated rows exist — `FrameAssembler`'s rule without
    the rows themselves: frame t needs the rows 0 .. t + K - 1, and the first `eog` of codebook 0 sits exactly K rows before the span's
    end (the cascade), so it can only be met once the span has ended at row `end_row` — then the frames are the end_row - K in front of it."""
    return max(int(end_row) - K, 0) if ended else max(int(n_rows) - K + 1, 0)


def stream_gather_ranges(released: Sequence[int], states: Sequence[Tuple[int, bool, int]], K: int) -> np.ndarray:
    """The table `ssrhip_stream_gather` reads at one poll, int32 [4][n] = step0 | f0 | f1 | col0: utterance u has `released[u]` frames
    out already, states[u] = (n_steps, span ended, span_end[0]); its new frames [f0, f1) go to the columns [0, f1 - f0) of the poll's block."""
    n = len(released)
    t = np.zeros((4, n), dtype=np.int32)
    for u, (rel, (n_rows, ended, end_row)) in enumerate(zip(released, states)):
        f1 = max(final_generated_frames(n_rows, ended, end_row, K), int(rel))
        t[:, u] = (0, int(rel), f1, -int(rel))
    return t

