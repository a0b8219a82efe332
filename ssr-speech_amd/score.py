"""Host planning and reduction of `SSR_Speech.score`: the teacher-forced loss and top-10 accuracy the reference's training forward
returns (models/ssr.py:280-379), computed without autograd.

Pure functions on numpy / torch:
  * `validate` checks a collated batch (data/gigaspeech.py:298-321) before anything reaches the device;
  * `pack_items` lays the items out as the prefill's flattened [text || audio] rows (the format of `DecodeEngine.admit`), one sequence
    per item, no padding rows: attention with the reference's causal + key-padding mask equals each item run unpadded;
  * `plan_chunks` splits the items into launches of at most `max_rows` rows;
  * `reduce` turns the per-position cross entropy and rank (ssrhip_xent_rank) into the reference's dict with its masks.
The arithmetic of the rows (layers, heads, cross entropy) runs in libssrhip.so (`ssrhip_lm_score`).
"""
from __future__ import annotations

import ast
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._lib import PAGE
from .layout import pack_prefill_rows


@dataclass
class Item:
    """One batch item, unpadded: text ids [L], audio ids [K, T] (T = y_len)."""
    index: int
    text: np.ndarray
    audio: np.ndarray

    @property
    def rows(self) -> int:
        return int(self.text.shape[0] + self.audio.shape[1])

    @property
    def n_scored(self) -> int:
        """Audio position t predicts y[t + 1]: T - 1 scored rows (models/ssr.py:350-351)."""
        return max(int(self.audio.shape[1]) - 1, 0)


def _np(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def validate(batch: dict, args) -> Optional[List[Item]]:
    """The collated batch -> its items, or None for an empty batch (ssr.py:296-297). Raises ValueError on anything the device must not
    see: wrong dims, lengths out of range, text ids outside [0, n_text), audio ids outside [0, card), and padded `y` positions
    (>= y_len) that are not `audio_pad_token` — the reference would score those, rows of padding predicting them."""
    for key in ("x", "x_lens", "y", "y_lens"):
        if key not in batch:
            raise ValueError(f"score: the batch has no '{key}'")
    x, x_lens, y, y_lens = (_np(batch[k]) for k in ("x", "x_lens", "y", "y_lens"))
    if len(x) == 0:
        return None
    K = int(args.n_codebooks)
    n_text = int(args.text_vocab_size) + 1
    card = int(args.audio_vocab_size) + int(args.n_special) + int(args.max_n_spans)
    if x.ndim != 2 or x_lens.ndim != 1 or y.ndim != 3 or y_lens.ndim != 1:
        raise ValueError(f"score: expected x [B,S], x_lens [B], y [B,K,T], y_lens [B]; got {x.shape}, {x_lens.shape}, {y.shape}, {y_lens.shape}")
    B = x.shape[0]
    if y.shape[0] != B or y.shape[1] != K or x_lens.shape[0] != B or y_lens.shape[0] != B:
        raise ValueError(f"score: batch sizes / codebooks disagree: x {x.shape}, x_lens {x_lens.shape}, y {y.shape} (K={K}), y_lens {y_lens.shape}")
    for name, a in (("x", x), ("x_lens", x_lens), ("y", y), ("y_lens", y_lens)):
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"score: {name} must hold integers, not {a.dtype}")
    x_lens, y_lens = x_lens.astype(np.int64), y_lens.astype(np.int64)
    if (x_lens < 0).any() or (x_lens > x.shape[1]).any():
        raise ValueError(f"score: x_lens {x_lens.tolist()} outside [0, {x.shape[1]}]")
    if (y_lens < 0).any() or (y_lens > y.shape[2]).any():
        raise ValueError(f"score: y_lens {y_lens.tolist()} outside [0, {y.shape[2]}]")
    ymax = int(y_lens.max())
    items = []
    for b in range(B):
        L, T = int(x_lens[b]), int(y_lens[b])
        tx = x[b, :L].astype(np.int64)
        au = y[b, :, :T].astype(np.int64)
        if tx.size and (tx.min() < 0 or tx.max() >= n_text):
            raise ValueError(f"score: item {b} has text ids outside [0, {n_text})")
        if au.size and (au.min() < 0 or au.max() >= card):
            raise ValueError(f"score: item {b} has audio ids outside [0, {card})")
        pad = y[b, :, T:ymax]
        if pad.size and (pad != int(args.audio_pad_token)).any():
            raise ValueError(f"score: item {b} has positions at or past y_len={T} that are not audio_pad_token={args.audio_pad_token}")
        items.append(Item(b, tx, au))
    return items


def plan_chunks(row_counts: Sequence[int], max_rows: int) -> List[List[int]]:
    """Indices of items grouped, in order, into chunks of at most `max_rows` rows; an item longer than that is a chunk of its own."""
    if max_rows < 1:
        raise ValueError(f"max_rows must be >= 1, not {max_rows}")
    chunks: List[List[int]] = []
    cur: List[int] = []
    n = 0
    for i, r in enumerate(row_counts):
        if cur and n + r > max_rows:
            chunks.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += int(r)
    if cur:
        chunks.append(cur)
    return chunks


def pack_items(items: Sequence[Item], K: int) -> Dict[str, np.ndarray]:
    """The prefill's rows (`layout.pack_prefill_rows`) for the items of one chunk, sequence s = items[s]: tok [R][4], pos / kind, row_seq /
    row_pos / row_len, seq_start [n+1]; the scored rows (score_first / score_count: audio positions 0 .. T-2 of each item) and their
    targets [K][M] = y[:, t + 1]; the KV page table of a scratch pool that holds every item's positions once (one layer)."""
    pk = pack_prefill_rows([(s, it.text, it.audio) for s, it in enumerate(items)], K)
    lens = [int(n) for n in pk.pop("lens")]
    max_len = max(lens)
    max_pages = (max_len + PAGE - 1) // PAGE
    table = np.zeros((len(items), max_pages), dtype=np.int32)
    nxt = 0
    for s, n in enumerate(lens):
        npg = (n + PAGE - 1) // PAGE
        table[s, :npg] = np.arange(nxt, nxt + npg)
        table[s, npg:] = nxt                       # never read (positions >= n are masked out); a valid page all the same
        nxt += npg
    tgts = [it.audio[:, 1:].astype(np.int32) for it in items]
    return dict(pk, score_first=np.asarray([s + it.text.shape[0] for s, it in zip(pk["seq_start"], items)], dtype=np.int32),
                score_count=np.asarray([it.n_scored for it in items], dtype=np.int32),
                target=np.concatenate(tgts, axis=1) if tgts else np.zeros((K, 0), dtype=np.int32),
                table=table, n_pages=np.asarray(nxt), max_len=np.asarray(max_len))


def scored_index(items: Sequence[Item]) -> Dict[str, np.ndarray]:
    """For the concatenation of the chunks' scored rows (chunk order = item order): batch index and position t (target y[t + 1]) of each."""
    b = [np.full(it.n_scored, it.index, dtype=np.int64) for it in items]
    t = [np.arange(it.n_scored, dtype=np.int64) for it in items]
    return dict(item=np.concatenate(b) if b else np.zeros(0, np.int64), pos=np.concatenate(t) if t else np.zeros(0, np.int64))


def codebook_weights(args) -> List[float]:
    cw = getattr(args, "codebook_weight", None)
    if cw is None:
        return [1.0] * int(args.n_codebooks)
    return list(ast.literal_eval(cw) if isinstance(cw, str) else cw)          # ssr.py:369-372 (eval of a list literal)


def reduce(nll: torch.Tensor, rank: torch.Tensor, target: torch.Tensor, item: torch.Tensor, pos: torch.Tensor, B: int, args) -> dict:
    """The reference's bookkeeping (ssr.py:353-379) over the scored rows of the whole batch, on their device.
    nll / rank / target: [K][M]; item / pos: [M] (batch index, position within the item). Returns the reference's four keys with its
    types, plus nll_by_item [B] (CE summed over every codebook's tmp_mask positions, unweighted) and ntoken_by_item [B] (their count)."""
    dev = nll.device
    K = int(args.n_codebooks)
    tg = target.to(torch.int64)
    mask = (tg != int(args.audio_pad_token)) & (tg != int(args.empty_token))
    if not args.predict_mask_token:
        mask &= tg < int(args.mts)
    tmp = mask.clone()
    if not args.predict_all:
        # positions before the LAST mask token of each (codebook, item) leave the loss (the loop at ssr.py:358-360)
        key = torch.arange(K, device=dev).unsqueeze(1) * B + item.unsqueeze(0)
        cand = torch.where(tg == int(args.mts), pos.unsqueeze(0).expand(K, -1), torch.full_like(tg, -1))
        last = torch.full((K * B,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, key.reshape(-1), cand.reshape(-1), "amax")
        tmp &= pos.unsqueeze(0) >= last[key]
    nll64 = nll.to(torch.float64)
    n_tmp = tmp.sum(1)
    ce_sum = torch.where(tmp, nll64, torch.zeros_like(nll64)).sum(1)
    hits = (tmp & (rank < 10)).sum(1)
    losses = (ce_sum / n_tmp.to(torch.float64)).to(torch.float32)                       # 0 / 0 = NaN, as F.cross_entropy of nothing
    accs = torch.where(n_tmp > 0, hits.to(torch.float64) / n_tmp.clamp(min=1).to(torch.float64), torch.zeros_like(ce_sum)).to(torch.float32)
    ntok = [int(v) for v in mask.sum(1).tolist()]                                        # `mask`, not `tmp_mask` (ssr.py:367)
    cw = codebook_weights(args)
    loss = sum(losses[k] * ntok[k] * cw[k] for k in range(K))
    by_cb = [accs[k] * ntok[k] for k in range(K)]
    nll_item = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, item, torch.where(tmp, nll64, torch.zeros_like(nll64)).sum(0))
    ntok_item = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, item, tmp.sum(0))
    return {"loss": loss, "top10acc": sum(by_cb), "top10acc_by_codebook": by_cb,
            "effective_ntoken": torch.tensor(sum(ntok)).to(dev),
            "nll_by_item": nll_item.to(torch.float32), "ntoken_by_item": ntok_item}
