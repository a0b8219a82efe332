"""Host-side driver of the HIP decode engine (libssrhip.so): weight arena, paged KV cache, prefill
rows, hipGraph decode loop, read-back.  PyTorch is used for device memory and streams only.

The arithmetic replaced is the device part of `SSR_Speech.inference` (reference `models/ssr.py:597-754`);
integer layout code lives in `layout.py`.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
from collections import namedtuple
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import PAGE, MAX_CODEBOOKS
from .layout import pack_prefill_rows


def sine_pe_table(n: int, dim: int) -> torch.Tensor:
    """Sinusoidal table built on the CPU in fp32 exactly like the reference does
    (models/modules/embedding.py:67-92: built on CPU, then moved to the device)."""
    pe = torch.zeros(n, dim)
    position = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


@dataclass
class DecodeKnobs:
    """Per-utterance decode parameters (the `inference()` keyword surface, models/ssr.py:513-523)."""
    top_k: int = -100
    top_p: float = 1.0
    temperature: float = 1.0
    stop_repetition: int = -1
    silence_tokens: Sequence[int] = (1388, 1898, 131)
    cfg_coef: float = 1.5
    cfg_stride: int = 1
    use_cfg: bool = False
    text_len: int = 0
    n_spans: int = 1
    seed: int = 0


def to_streaming_order(W: torch.Tensor) -> torch.Tensor:
    """[.., N, K] row-major -> the matrix-core GEMV's streaming order (include/ssrhip.h SSRHIP_WTILED_INDEX): rows in 8-row
    units (zero-padded), K in 16-float steps, each (unit, k-step) a 512-byte block indexed [k-slot 0..3][row 0..7][4 floats]."""
    *lead, N, K = W.shape
    assert K % 16 == 0, K
    U = (N + 7) // 8
    if U * 8 != N:
        W = torch.cat([W, W.new_zeros(*lead, U * 8 - N, K)], dim=-2)
    return W.reshape(*lead, U, 8, K // 16, 4, 4).permute(*range(len(lead)), -5, -3, -2, -4, -1).contiguous()


def to_w16_order(W: torch.Tensor) -> torch.Tensor:
    """[.., N, K] (K % 1024 == 0) -> the packed bf16 order of the <= 4-row bf16 weight stream (include/ssrhip.h SSRHIP_W16_INDEX) as an
    int16 tensor of the same shape: per (row, 1024-element segment) two KiB-sized wave loads, lane l's 16 bytes of load j holding the fp32
    kernel's float4 #2j and #2j+1 of that lane. Values are rounded to bf16 (nearest even); already rounded masters pack exactly."""
    *lead, N, K = W.shape
    assert K % 1024 == 0, K
    Wb = W.to(torch.bfloat16).reshape(*lead, N, K // 1024, 2, 2, 64, 4)          # [n][segment][i / 2][i % 2][lane][k % 4]
    n = len(lead)
    return Wb.permute(*range(n), n, n + 1, n + 2, n + 4, n + 3, n + 5).contiguous().view(torch.int16).reshape(*lead, N, K)


def to_wt16_order(W: torch.Tensor) -> torch.Tensor:
    """[.., N, K] (K % 64 == 0) -> the packed bf16 streaming order of the 5..16-row bf16 weight stream (include/ssrhip.h SSRHIP_WT16_INDEX)
    as an int16 tensor [.., ceil(N/8)*8, K]: rows in 8-row units (zero-padded), K in quads of four k-steps; the 512-byte block (unit, quad,
    h) holds at 16-byte piece ks*8 + c the four weights of k-step 4q + h followed by the four of k-step 4q + h + 2. Values are rounded to
    bf16 (nearest even); already rounded masters pack exactly."""
    *lead, N, K = W.shape
    assert K % 64 == 0, K
    U = (N + 7) // 8
    if U * 8 != N:
        W = torch.cat([W, W.new_zeros(*lead, U * 8 - N, K)], dim=-2)
    Wb = W.to(torch.bfloat16).reshape(*lead, U, 8, K // 64, 2, 2, 4, 4)          # [u][c][q][g][h][ks][e]
    n = len(lead)
    return Wb.permute(*range(n), n, n + 2, n + 4, n + 5, n + 1, n + 3, n + 6).contiguous().view(torch.int16).reshape(*lead, U * 8, K)


def from_wt16_order(P: torch.Tensor, N: int) -> torch.Tensor:
    """Inverse of `to_wt16_order`: the packed int16 tensor [.., ceil(N/8)*8, K] -> the fp32 values [.., N, K] it stores (exact: << 16)."""
    *lead, NP, K = P.shape
    U = NP // 8
    n = len(lead)
    Wb = P.view(torch.bfloat16).reshape(*lead, U, K // 64, 2, 4, 8, 2, 4)         # [u][q][h][ks][c][g][e]
    Wb = Wb.permute(*range(n), n, n + 4, n + 1, n + 5, n + 2, n + 3, n + 6).reshape(*lead, NP, K)
    return Wb[..., :N, :].to(torch.float32).contiguous()


def to_w8_order(Q: torch.Tensor) -> torch.Tensor:
    """[.., N, K] 1-byte codes (K % 1024 == 0) -> the packed order of the <= 4-row e4m3 weight stream (include/ssrhip.h SSRHIP_W8_INDEX), same
    shape and dtype: per (row, 1024-element segment) ONE KiB-sized wave load, lane l's 16 bytes holding the fp32 kernel's four float4 of
    that lane in order. One permute; nothing is rounded here (the codes come from `quantize_e4m3` / `e4m3_codes`)."""
    *lead, N, K = Q.shape
    assert K % 1024 == 0 and Q.element_size() == 1, (K, Q.dtype)
    n = len(lead)
    return Q.reshape(*lead, N, K // 1024, 4, 64, 4).permute(*range(n), n, n + 1, n + 3, n + 2, n + 4).contiguous().reshape(*lead, N, K)   # [n][segment][i][lane][k % 4] -> [..][lane][i][..]


def from_w8_order(P: torch.Tensor) -> torch.Tensor:
    """Inverse of `to_w8_order`: the packed codes [.., N, K] -> the codes in [n][k] order."""
    *lead, N, K = P.shape
    n = len(lead)
    return P.reshape(*lead, N, K // 1024, 64, 4, 4).permute(*range(n), n, n + 1, n + 3, n + 2, n + 4).contiguous().reshape(*lead, N, K)


def to_wt8_order(Q: torch.Tensor) -> torch.Tensor:
    """[.., N, K] 1-byte codes (K % 128 == 0) -> the packed order of the 5..16-row e4m3 weight stream (include/ssrhip.h SSRHIP_WT8_INDEX),
    [.., ceil(N/8)*8, K] of the same dtype: rows in 8-row units (padded with code 0), K in octets of eight k-steps; the 512-byte block
    (unit, octet, h) holds at 16-byte piece ks*8 + c, as dword g, the four codes of k-step 8o + 2g + h. One permute; nothing is rounded."""
    *lead, N, K = Q.shape
    assert K % 128 == 0 and Q.element_size() == 1, (K, Q.dtype)
    U = (N + 7) // 8
    if U * 8 != N:
        Q = torch.cat([Q, Q.new_zeros(*lead, U * 8 - N, K)], dim=-2)
    n = len(lead)
    Qr = Q.reshape(*lead, U, 8, K // 128, 4, 2, 4, 4)                            # [u][c][o][g][h][ks][e]
    return Qr.permute(*range(n), n, n + 2, n + 4, n + 5, n + 1, n + 3, n + 6).contiguous().reshape(*lead, U * 8, K)


def from_wt8_order(P: torch.Tensor, N: int) -> torch.Tensor:
    """Inverse of `to_wt8_order`: the packed codes [.., ceil(N/8)*8, K] -> the codes [.., N, K] in [n][k] order."""
    *lead, NP, K = P.shape
    U = NP // 8
    n = len(lead)
    Qr = P.reshape(*lead, U, K // 128, 2, 4, 8, 4, 4)                            # [u][o][h][ks][c][g][e]
    return Qr.permute(*range(n), n, n + 4, n + 1, n + 5, n + 2, n + 3, n + 6).reshape(*lead, NP, K)[..., :N, :].contiguous()


E4M3_MAX = 448.0              # the largest finite OCP e4m3 value (torch.float8_e4m3fn): 0.875 * 2^9


def quantize_e4m3(W: torch.Tensor):
    """[.., N, K] fp32 -> (codes uint8 [.., N, K], scale fp32 [.., N]): per output row the smallest integer e with amax <= 448 * 2^e (exactly,
    from `torch.frexp`: amax = m * 2^x, m in [0.5, 1): e = x - 9 if m <= 0.875 else x - 8; a row of zeros takes e = 0; clamped to
    [-100, 100]), scale = 2^e, codes = ldexp(W, -e) rounded to OCP e4m3 (nearest, ties to even). |ldexp(W, -e)| <= 448 by construction, so
    the NaN codes 0x7f / 0xff never occur. A non-finite weight or one with |w| >= 2^100 raises ValueError. The weight the model then
    computes with is codes.view(float8_e4m3fn).float() * scale, exactly (`e4m3_master`)."""
    W = W.to(torch.float32)
    if not bool(torch.isfinite(W).all()):
        raise ValueError("quantize_e4m3: non-finite weight")
    amax = W.abs().amax(dim=-1)
    if bool((amax >= 2.0 ** 100).any()):
        raise ValueError("quantize_e4m3: |weight| >= 2^100")
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-100, 100)
    scale = torch.ldexp(torch.ones_like(amax), e)
    return e4m3_codes(W, scale), scale


def e4m3_codes(W: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The codes of `quantize_e4m3` for given power-of-two scales [.., N]: W / scale (exact) rounded to e4m3. On a master it is the exact inverse
    of `e4m3_master`."""
    return (W * (1.0 / scale).unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_master(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """codes * scale as fp32 [.., N, K]: exact (an e4m3 value has 4 significant bits, the scale is a power of two), and bf16-representable."""
    return (codes.view(torch.float8_e4m3fn).to(torch.float32) * scale.unsqueeze(-1)).contiguous()


W16_FAMILIES = ("in_proj", "out_proj", "ffn1", "ffn2")      # per layer; plus head1 and head2
WEIGHT_DTYPES = ("fp32", "bf16", "e4m3")
BF16_VALUED = ("bf16", "e4m3")      # arenas whose masters are bf16-representable (an e4m3 value times a power of two is)
# What an unset SSRHIP_GEMVM_W16 means for a 5..16-row engine of a bf16 arena (DecodeEngine stream_wt16=None): "1" = stream the
# SSRHIP_WT16_INDEX copies, "0" = stream the fp32 streaming-order masters. Decided by the measurement in DESIGN.md Part I.11.
WT16_DEFAULT = "0"
# The same switch for a 17..32-row engine of a bf16 arena (DecodeEngine stream_wt32=None): "1" = the two-panel step streams the same
# SSRHIP_WT16_INDEX copies. Decided by the measurement in DESIGN.md Part I.12.
WT32_DEFAULT = "0"
# What an unset SSRHIP_PREFILL_W1 means for a bf16 arena: "1" = the prefill / score GEMMs get ONE bf16 plane per matrix (the weight itself,
# csrc/gemm_split.hip ssrhip_gemm_w1), "0" = the three planes of the exact split (two of them zeros). Decided by the measurement in
# DESIGN.md Part I.13 (one plane: prefill 10.65 -> 6.69 ms at 598 rows, 42.5 -> 29.5 ms at 4,784 rows, same bits).
PREFILL_W1_DEFAULT = "1"


def w16_streamable(K: int) -> bool:
    """Can a matrix with this inner dimension have a packed copy (the shapes ssrhip_gemv_w16 takes)?"""
    return K % 1024 == 0 and K // 1024 in (1, 2, 4, 8)


def wt16_streamable(K: int) -> bool:
    """Can a matrix with this inner dimension have a SSRHIP_WT16_INDEX copy (whole quads of four k-steps)?"""
    return K > 0 and K % 64 == 0


def wt8_streamable(K: int) -> bool:
    """Can a matrix with this inner dimension have a SSRHIP_WT8_INDEX copy (whole octets of eight k-steps)?"""
    return K > 0 and K % 128 == 0


# What an unset SSRHIP_GEMVM_W8 means for a 5..16-row engine of an e4m3 arena (DecodeEngine stream_wt8=None): "1" = stream the
# SSRHIP_WT8_INDEX codes and the scales, "0" = stream what such an engine streams without them (the fp32 streaming-order masters, or the
# 2-byte copies under SSRHIP_GEMVM_W16). Decided by the measurement in DESIGN.md Part I.22.
WT8_DEFAULT = "0"


# The packed orders an arena can hold: (pack routine, which inner dimensions get a copy). A matrix's copy of order `o` lives in
# lay[name + "_" + o] / arena.head{1,2}_<o>, under the flag arena._<o>_ready. PACKED_ORDERS: 2-byte copies of the masters of a bf16-valued
# arena; CODE_ORDERS: the 1-byte codes of an e4m3 arena (`e4m3_codes(master, scale)`, exact), read beside the arena's scales.
PACKED_ORDERS = {"w16": (to_w16_order, w16_streamable), "wt16": (to_wt16_order, wt16_streamable)}
CODE_ORDERS = {"w8": (to_w8_order, w16_streamable), "wt8": (to_wt8_order, wt8_streamable)}


# One weight stream of the decode step per format and row range. `name` is the suffix of DecodeEngine's `stream_<name>` keyword and
# attribute, of the C setter `ssrhip_lm_set_<name>` and of the counter `ssrhip_lm_<name>_launches`; [lo, hi] its rows (`rows`: as messages
# spell them); `switch` the environment variable an engine built with `stream_<name>=None` reads and `default` what it means when unset;
# `order` the packed order (PACKED_ORDERS / CODE_ORDERS) its kernels read; `only` what a refusal of more rows says; `fmt` the format word
# of its messages, which is the arena dtype `resolve_stream` asks for; `arenas` the arena dtypes that can serve it — the 2-byte copies of
# the matrix-core step serve every bf16-valued arena, the <= 4-row bf16 stream is the bf16 arena's own. Same tokens, bit for bit, as the
# same arena's masters, for every entry. An engine takes one: the row ranges of one format are disjoint, a w8 and a w16 (wt8 and wt16)
# request together are a ValueError, and a stream_wt8 that resolves on turns an unrequested wt16 off (the 1-byte stream takes the step).
Stream = namedtuple("Stream", "name lo hi rows switch default order only fmt arenas")
STREAMS = (
    Stream("w16", 1, 4, "<= 4", "SSRHIP_GEMV_W16", "1", "w16", "the bf16 weight stream exists for the <= 4-row decode step only", "bf16", ("bf16",)),
    Stream("wt16", 5, 16, "5..16", "SSRHIP_GEMVM_W16", WT16_DEFAULT, "wt16", "the bf16 weight stream of the matrix-core step exists for 5..16 rows only", "bf16", BF16_VALUED),
    Stream("wt32", 17, 32, "17..32", "SSRHIP_GEMVM_W16", WT32_DEFAULT, "wt16", "the bf16 weight stream of the two-panel step exists for 17..32 rows only", "bf16", BF16_VALUED),
    Stream("w8", 1, 4, "<= 4", "SSRHIP_GEMV_W8", "1", "w8", "the e4m3 weight stream exists for the <= 4-row decode step only", "e4m3", ("e4m3",)),
    Stream("wt8", 5, 16, "5..16", "SSRHIP_GEMVM_W8", WT8_DEFAULT, "wt8", "the e4m3 weight stream of the matrix-core step exists for 5..16 rows only", "e4m3", ("e4m3",)),
)
W16Stream, W16_STREAMS = Stream, STREAMS[:3]      # the bf16 entries, under the names they had before the e4m3 ones joined the table
STREAM_OF = {st.name: st for st in STREAMS}


def resolve_stream(st: Stream, rows: int, weight_dtype: str, requested: Optional[bool], env) -> bool:
    """Does an engine of `rows` rows on an arena of `weight_dtype` run stream `st`? requested None: on iff the arena is of the stream's
    format, the rows are the stream's and `env[st.switch]` (unset: st.default) does not start with '0'. requested True: ValueError for rows
    outside the range (named before the dtype is looked at; below it, the message names the stream of the same format that takes these
    rows), then for another arena. `env` is a mapping like os.environ; nothing else is read."""
    if requested is None:
        return weight_dtype == st.fmt and st.lo <= rows <= st.hi and env.get(st.switch, st.default)[:1] != "0"
    if not requested:
        return False
    if rows < st.lo:
        owner = next(o for o in STREAMS if o.fmt == st.fmt and rows <= o.hi)
        raise ValueError(f"stream_{st.name} is the {st.fmt} weight stream of the {st.rows}-row step; an engine of {rows} rows takes stream_{owner.name}")
    if rows > st.hi:
        raise ValueError(f"stream_{st.name}: {st.only} (this engine has {rows} rows)")
    if weight_dtype != st.fmt:
        raise ValueError(f"stream_{st.name} needs an arena built with weight_dtype='{st.fmt}'")
    return True


def resolve_w16_stream(st: Stream, rows: int, weight_dtype: str, requested: Optional[bool], env) -> bool:
    """`resolve_stream` under the name it had when the table held the bf16 streams only (DecodeEngine stream_w16 / stream_wt16 / stream_wt32)."""
    return resolve_stream(st, rows, weight_dtype, requested, env)


def resolve_w8_stream(rows: int, weight_dtype: str, requested: Optional[bool], env) -> bool:
    """`resolve_stream` for the e4m3 stream of the <= 4-row step (DecodeEngine stream_w8)."""
    return resolve_stream(STREAM_OF["w8"], rows, weight_dtype, requested, env)


def resolve_wt8_stream(rows: int, weight_dtype: str, requested: Optional[bool], env) -> bool:
    """`resolve_stream` for the e4m3 stream of the 5..16-row matrix-core step (DecodeEngine stream_wt8)."""
    return resolve_stream(STREAM_OF["wt8"], rows, weight_dtype, requested, env)


# What an unset switch of a pair form means (DecodeEngine pair_w16 / pair_w8 / pair4 / pair4_pk = None): "1" = the step runs that form's
# pair launches, "0" = it steps with its single launches. DESIGN.md Parts I.19, I.20, I.24, I.26.
W16_PAIR_DEFAULT = "0"
W8_PAIR_DEFAULT = "0"
PAIR4_DEFAULT = "0"
PAIR4_PK_DEFAULT = "0"
PAIR4_WS_BYTES = 3 * 8192 * 8 + 64      # include/ssrhip.h SSRHIP_PAIR4_WS_BYTES: three buffers of 4 x 2048 granules + the give-up flag

# One opt-in pair-launch form of the decode step per row count and weight stream. `name` is DecodeEngine's keyword and attribute; `c_name` the
# suffix of the C setter `ssrhip_lm_set_<c_name>` and of the counter `ssrhip_lm_<c_name>_launches`; `rows` the one row count it exists for; `switch`
# the environment variable an engine built with `<name>=None` reads and `default` what it means when unset; `fits(stream)` whether the
# form pairs an engine whose stream is `stream` (a Stream, None: the fp32 masters); `only` what a refusal of another row count says and
# `needs(stream)` what a refusal of the stream says. Whether an engine that asks then GETS to pair (device, pairing slot) is the library's
# decision (`DecodeEngine.pairing`, `pairing_why`). Same tokens, bit for bit, either way.
PairForm = namedtuple("PairForm", "name c_name rows switch default fits only needs")
PAIR_FORMS = (
    PairForm("pair_w16", "w16_pair", 2, "SSRHIP_GEMV_W16_PAIR", W16_PAIR_DEFAULT, lambda st: st is STREAM_OF["w16"],
             "pair launches exist for the 2-row decode step only",
             lambda st: "pair_w16 needs an engine that streams bf16 weights (stream_w16)"),
    PairForm("pair_w8", "w8_pair", 2, "SSRHIP_GEMV_W8_PAIR", W8_PAIR_DEFAULT, lambda st: st is STREAM_OF["w8"],
             "pair launches exist for the 2-row decode step only",
             lambda st: "pair_w8 needs an engine that streams e4m3 weights (stream_w8)"),
    PairForm("pair4", "pair4", 4, "SSRHIP_GEMV_PAIR4", PAIR4_DEFAULT, lambda st: st is None,
             "the 4-row pair launches exist for the 4-row decode step only",
             lambda st: f"pair4: the 4-row pair launches read fp32 weights (this engine streams {st.fmt} weights: stream_{st.name})"),
    PairForm("pair4_pk", "pair4_pk", 4, "SSRHIP_GEMV_PAIR4_PK", PAIR4_PK_DEFAULT, lambda st: st is not None,
             "the 4-row pair launches exist for the 4-row decode step only",
             lambda st: "pair4_pk needs an engine that streams packed weights (stream_w16 or stream_w8); pair4 pairs the fp32 masters"),
)
PAIR_OF = {pf.name: pf for pf in PAIR_FORMS}


def resolve_pair(pf: PairForm, rows: int, stream: Optional[Stream], pair_mode: int, requested: Optional[bool], env) -> bool:
    """Does an engine of `rows` rows whose weight stream is `stream` ask for pair form `pf`? requested None: on iff the rows are the
    form's, the stream fits, pair_mode is not 1 and `env[pf.switch]` (unset: pf.default) does not start with '0'. requested True: ValueError
    at another row count (named first), then for a stream that does not fit, then with pair_mode 1. `env` is a mapping like os.environ;
    nothing else is read."""
    if requested is None:
        return rows == pf.rows and pf.fits(stream) and pair_mode != 1 and env.get(pf.switch, pf.default)[:1] != "0"
    if not requested:
        return False
    if rows != pf.rows:
        raise ValueError(f"{pf.name}: {pf.only} (this engine has {rows} rows)")
    if not pf.fits(stream):
        raise ValueError(pf.needs(stream))
    if pair_mode == 1:
        raise ValueError(f"{pf.name} with pair_mode=1: the caller switched pair launches off")
    return True


def _small_stream(stream_w16: bool, stream_w8: bool = False) -> Optional[Stream]:
    """The stream of a <= 4-row engine from the two flags the four functions below take; each of them is `resolve_pair` for one form."""
    return STREAM_OF["w16"] if stream_w16 else STREAM_OF["w8"] if stream_w8 else None


def resolve_w16_pair(rows: int, stream_w16: bool, pair_mode: int, requested: Optional[bool], env) -> bool:
    return resolve_pair(PAIR_OF["pair_w16"], rows, _small_stream(stream_w16), pair_mode, requested, env)


def resolve_w8_pair(rows: int, stream_w8: bool, pair_mode: int, requested: Optional[bool], env) -> bool:
    return resolve_pair(PAIR_OF["pair_w8"], rows, _small_stream(False, stream_w8), pair_mode, requested, env)


def resolve_pair4(rows: int, stream_w16: bool, stream_w8: bool, pair_mode: int, requested: Optional[bool], env) -> bool:
    return resolve_pair(PAIR_OF["pair4"], rows, _small_stream(stream_w16, stream_w8), pair_mode, requested, env)


def resolve_pair4_pk(rows: int, stream_w16: bool, stream_w8: bool, pair_mode: int, requested: Optional[bool], env) -> bool:
    return resolve_pair(PAIR_OF["pair4_pk"], rows, _small_stream(stream_w16, stream_w8), pair_mode, requested, env)


KV_DTYPES = ("fp32", "bf16")
KV16_MAX_PAGES = 256          # pages per row the fused attention walk takes (csrc/attn.hip ATTN_ROWS_MAX_PAGES)


def resolve_kv_dtype(rows: int, requested: Optional[str], model_default: str = "fp32", max_pages: Optional[int] = None) -> str:
    """The entry type of the KV cache of an engine of `rows` rows. The bf16 cache exists for the 5..32-row step with at most
    KV16_MAX_PAGES pages per row. requested "bf16" outside that: ValueError. requested None: `model_default`
    (SSR_Speech.set_kv_dtype) where the engine can hold it, "fp32" otherwise — the 2-row paths keep fp32 K/V. Nothing else is read."""
    for what, v in (("kv_dtype", requested), ("model default kv_dtype", model_default)):
        if v is not None and v not in KV_DTYPES:
            raise ValueError(f"{what} {v!r} not in {KV_DTYPES}")
    fits = 5 <= rows <= MAX_ROWS and (max_pages is None or max_pages <= KV16_MAX_PAGES)
    if requested is None:
        return model_default if fits else "fp32"
    if requested == "bf16" and not fits:
        if not 5 <= rows <= MAX_ROWS:
            raise ValueError(f"kv_dtype='bf16' exists for engines of 5..{MAX_ROWS} rows (this engine has {rows} rows)")
        raise ValueError(f"kv_dtype='bf16' takes at most {KV16_MAX_PAGES} pages per row (this engine has {max_pages})")
    return requested


# What an unset SSRHIP_ATTN_KV16_SMALL means for an engine of <= 4 rows whose wanted cache type is "bf16" (DecodeEngine kv16_small=None):
# "1" = it holds the 2-byte cache through the landing cache (include/ssrhip.h ssrhip_lm_set_kv16_small), "0" = the rule of
# `resolve_kv_dtype` stands: its K / V stay fp32. DESIGN.md Part I.23.
KV16_SMALL_DEFAULT = "0"
KV16_SMALL_MAX_LAYERS = 128   # layer l lands at position l of a row's landing page (SSRHIP_PAGE positions)


def resolve_kv16_small(rows: int, kv_requested: Optional[str], model_default: str, requested: Optional[bool], env) -> bool:
    """Does an engine of `rows` rows hold a bf16 KV cache through the landing cache of the 1/2/4-row step (DecodeEngine kv16_small)? The
    wanted cache type is `kv_requested`, or `model_default` (SSR_Speech.set_kv_dtype) when that is None. requested None: on iff the engine
    has <= 4 rows, the wanted type is "bf16" and `env["SSRHIP_ATTN_KV16_SMALL"]` (unset: KV16_SMALL_DEFAULT) does not start with '0'.
    requested True: ValueError at more than 4 rows (named first), then when the wanted type is "fp32". When the answer is yes the engine's
    kv_dtype is "bf16" and `resolve_kv_dtype` is not asked. `env` is a mapping like os.environ; nothing else is read."""
    wanted = model_default if kv_requested is None else kv_requested
    if requested is None:
        return rows <= 4 and wanted == "bf16" and env.get("SSRHIP_ATTN_KV16_SMALL", KV16_SMALL_DEFAULT)[:1] != "0"
    if not requested:
        return False
    if rows > 4:
        raise ValueError(f"kv16_small: the landing cache exists for the 1/2/4-row decode step only (this engine has {rows} rows; "
                         f"engines of 5..{MAX_ROWS} rows take kv_dtype='bf16')")
    if wanted != "bf16":
        raise ValueError(f"kv16_small needs the bf16 cache type (kv_dtype='bf16' or SSR_Speech.set_kv_dtype('bf16')), not {wanted!r}")
    return True


SAMPLING_RNGS = ("torch_cpu", "philox")


def resolve_sampling_rng(requested: Optional[str], model_default: str = "torch_cpu") -> str:
    """Where a sampled run's multinomial noise comes from (DESIGN.md Part I.21). "torch_cpu": the host draws torch's CPU stream
    (`TorchCpuNoiseFeed`, `NoiseUploader`) — the reference's tokens from the seed alone; "philox": a counter-based generator on the device
    writes it (`PhiloxNoise`) — seed -> same tokens whatever the batch, no host draw. requested None: `model_default`
    (SSR_Speech.set_sampling_rng). A name outside SAMPLING_RNGS is a ValueError. Nothing else is read."""
    for what, v in (("sampling_rng", requested), ("model default sampling_rng", model_default)):
        if v is not None and v not in SAMPLING_RNGS:
            raise ValueError(f"{what} {v!r} not in {SAMPLING_RNGS}")
    return model_default if requested is None else requested


def resolve_share_prompt(rows: int, requested: Optional[bool], kv_dtype: str = "fp32") -> bool:
    """Does an engine of `rows` rows share the prompt's KV pages among equal rows (DESIGN.md Part I.15)? Pure. An explicit True where the
    grouped attention walk does not exist is a ValueError: at <= 4 rows (the split kernels), and with a bf16 KV cache (the grouped walk
    reads fp32 entries). None = off: nothing turns it on but the caller."""
    if not requested:
        return False
    if rows <= 4:
        raise ValueError(f"share_prompt exists for engines of 5..{MAX_ROWS} rows (this engine has {rows} rows)")
    if kv_dtype == "bf16":
        raise ValueError("share_prompt does not combine with kv_dtype='bf16' (the grouped attention walk reads fp32 entries)")
    return True


# Everything an engine decides before it allocates. `stream`: the one weight stream that is on (a STREAMS entry; None: the fp32 masters);
# `pair`: the one pair form asked for (a PAIR_FORMS entry; None: none); `max_pages`: pages per row.
DecodePlan = namedtuple("DecodePlan", "rows stream pair pair_mode kv_dtype kv16_small share_prompt logprobs max_pages")
STREAM_KEYWORDS = tuple("stream_" + st.name for st in STREAMS)
PAIR_KEYWORDS = tuple(pf.name for pf in PAIR_FORMS)


def resolve_decode_plan(rows: int, weight_dtype: str, n_layers: int, max_seq: int, env, pair_mode: int = 0, kv_dtype: Optional[str] = None,
                        share_prompt: Optional[bool] = None, kv16_small: Optional[bool] = None, logprobs: bool = False,
                        kv_default: str = "fp32", **requested) -> DecodePlan:
    """The plan of an engine of `rows` rows and `max_seq` positions per row on an arena of `weight_dtype` with `n_layers` layers.
    `requested`: the stream_* and pair* keywords of DecodeEngine.__init__ (STREAM_KEYWORDS, PAIR_KEYWORDS; absent = None); `kv_default`: the
    model's cache type (SSR_Speech.set_kv_dtype), which stands where `kv_dtype` is None. The cross rules, in the order they refuse: the rows;
    two streams of one step asked for together; each stream's own rule (`resolve_stream`; a wt8 that resolves on turns an unrequested wt16
    off, and refuses a requested one); `resolve_kv16_small` and its layer cap — when it says yes the cache is "bf16" and `resolve_kv_dtype`
    is not asked; `resolve_share_prompt` and its page cap; each pair form's rule (`resolve_pair`). Pure: reads its arguments and `env`
    (a mapping like os.environ), nothing else."""
    unknown = set(requested) - set(STREAM_KEYWORDS + PAIR_KEYWORDS)
    if unknown:
        raise TypeError(f"resolve_decode_plan: unknown request {sorted(unknown)}")
    if rows not in (1, 2, 4) and not (5 <= rows <= MAX_ROWS):
        raise ValueError(f"rows B={rows} not supported by this build (1, 2, 4 or 5..{MAX_ROWS})")
    ask = {st.name: requested.get("stream_" + st.name) for st in STREAMS}
    two = "stream_{0.name} and stream_{1.name} are two weight streams of the {0.rows}-row step; an engine takes one"
    on = []
    for st in STREAMS[3:] + STREAMS[:3]:      # the e4m3 streams first: wt8's answer decides an unrequested wt16
        twin = next((o for o in STREAMS[:3] if st.fmt == "e4m3" and (o.lo, o.hi) == (st.lo, st.hi)), None)      # the bf16 stream of its rows
        if twin and ask[st.name] and ask[twin.name]:
            raise ValueError(two.format(st, twin))
        if st.name == "wt16" and STREAM_OF["wt8"] in on and ask["wt16"] is None:
            continue                          # the 1-byte stream takes the step; the 2-byte copies are not built
        if resolve_stream(st, rows, st.fmt if weight_dtype in st.arenas else weight_dtype, ask[st.name], env):
            on.append(st)
    if len(on) > 1:                           # stream_wt16=True against a switched-on wt8: the library takes one packed stream
        raise ValueError(two.format(*on))
    stream = on[0] if on else None
    max_pages = (max_seq + PAGE - 1) // PAGE
    small = resolve_kv16_small(rows, kv_dtype, kv_default, kv16_small, env)
    if small and n_layers > KV16_SMALL_MAX_LAYERS:
        raise ValueError(f"kv16_small takes at most {KV16_SMALL_MAX_LAYERS} layers (this model has {n_layers})")
    kv = "bf16" if small else resolve_kv_dtype(rows, kv_dtype, kv_default, max_pages)
    share = resolve_share_prompt(rows, share_prompt, kv)
    if share and max_pages > KV16_MAX_PAGES:
        raise ValueError(f"share_prompt takes at most {KV16_MAX_PAGES} pages per row (this engine has {max_pages})")
    pair_mode = int(pair_mode)
    pairs = [pf for pf in PAIR_FORMS if resolve_pair(pf, rows, stream, pair_mode, requested.get(pf.name), env)]      # at most one fits
    return DecodePlan(rows, stream, pairs[0] if pairs else None, pair_mode, kv, small, share, bool(logprobs), max_pages)


def plan_prompt_sharing(seqs, members: int):
    """Which rows of ONE admission have the same prompt, and the attention chunks they form. Pure. seqs: (row, text ids, audio columns)
    triples. Returns (leader, chunks): leader[row] = the lowest row with an equal text AND equal audio columns (the row itself when there
    is none), chunks = lists of at most `members` rows with one leader, rows ascending, the chunks ordered by their first row; a row
    without company is a chunk of one. Under CFG the conditional rows of N samples of one utterance are rows 0, 2, 4, ... of one group;
    their unconditional rows are a second group when their texts are equal and unshared rows when `aug_text` drew each its own."""
    if members < 1:
        raise ValueError("members must be >= 1")
    first, leader, groups = {}, {}, {}
    for row, text, au in sorted(seqs, key=lambda t: t[0]):
        t, a = np.ascontiguousarray(np.asarray(text, dtype=np.int64)), np.ascontiguousarray(np.asarray(au, dtype=np.int64))
        key = (t.shape, t.tobytes(), a.shape, a.tobytes())
        lead = first.setdefault(key, row)
        leader[row] = lead
        groups.setdefault(lead, []).append(row)
    chunks = [g[i:i + members] for g in groups.values() for i in range(0, len(g), members)]
    return leader, sorted(chunks, key=lambda c: c[0])


def resolve_prefill_planes(weight_dtype: str, requested: Optional[int], env) -> int:
    """How many bf16 planes per matrix does an arena of `weight_dtype` build for the prefill / score GEMMs? 0 = none (`env` has
    SSRHIP_PREFILL_SPLIT starting with '0': the fp32 chain, whatever else is asked), 3 = the exact split of an fp32 value, 1 = the value
    itself, which only a bf16-valued arena's masters are ("bf16", "e4m3"). requested None: 1 iff the arena is bf16-valued and `env["SSRHIP_PREFILL_W1"]` (unset:
    PREFILL_W1_DEFAULT) does not start with '0'. requested 1 on an fp32 arena: ValueError. `env` is a mapping like os.environ; nothing else
    is read."""
    if requested not in (None, 1, 3):
        raise ValueError(f"split planes come as 1 or 3 per matrix, not {requested!r}")
    if requested == 1 and weight_dtype not in BF16_VALUED:
        raise ValueError("one plane per matrix needs an arena built with weight_dtype='bf16' (an fp32 weight is the sum of three bf16 planes)")
    if env.get("SSRHIP_PREFILL_SPLIT", "1")[:1] == "0":      # the C side's rule (engine.hip): a value that starts with '0'
        return 0
    if requested is not None:
        return requested
    return 1 if weight_dtype in BF16_VALUED and env.get("SSRHIP_PREFILL_W1", PREFILL_W1_DEFAULT)[:1] != "0" else 3


class LMWeightsArena:
    """Device-resident fp32 weights in the layout the kernels want (one-time repack at load).

    weight_dtype="bf16": the six matrix families of the decode step (in_proj / out_proj / ffn1 / ffn2 per layer, head1, head2) are rounded
    ONCE to bf16 (nearest even) as the arena holds them, i.e. after the LayerNorm fold, and kept as fp32 "masters" in the usual fields:
    prefill, score, the streaming-order copies and the split planes all read the same rounded values. `ensure_w16_copies` adds the
    packed 2-byte copies the <= 4-row decode step streams. Biases, embeddings and the position table stay fp32.

    weight_dtype="e4m3": the same six families are quantised ONCE (`quantize_e4m3`: OCP e4m3 codes and one power-of-two scale per output
    row, per group for head2), after the LayerNorm fold; the masters hold codes * scale, which is bf16-representable, so the arena is
    `bf16_valued` and every rule made for bf16 masters applies to it. The scales stay with the arena (lay[name + "_w8s"], head{1,2}_w8s);
    `ensure_w8_copies` adds the packed 1-byte codes the <= 4-row decode step streams. The rounding is coarse: 2.6 % relative rms of the
    weights against 0.17 % for bf16. Biases carry W beta from the UNROUNDED weights."""

    def __init__(self, args, sd: dict, device, max_pos: int = 8192, weight_dtype: str = "fp32"):
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype {weight_dtype!r} not in {WEIGHT_DTYPES}")
        self.weight_dtype = weight_dtype
        f32 = dict(dtype=torch.float32, device=device)
        self.args = args
        self.device = device
        self.D = int(args.d_model)
        self.H = int(args.nhead)
        self.L = int(args.num_decoder_layers)
        self.K = int(args.n_codebooks)
        V = int(args.audio_vocab_size)
        self.card = V + int(args.n_special) + int(args.max_n_spans)
        self.Hh = V // 2
        self.F = 4 * self.D
        self.n_text = int(args.text_vocab_size) + 1
        self.max_pos = max_pos
        g = lambda k: sd[k].detach().to(**f32).contiguous()
        self.text_emb = g("text_embedding.word_embeddings.weight")
        self.audio_emb = torch.stack([g(f"audio_embedding.{k}.word_embeddings.weight") for k in range(self.K)]).contiguous()
        self.alpha_text = float(sd["text_positional_embedding.alpha"].reshape(-1)[0])
        self.alpha_audio = float(sd["audio_positional_embedding.alpha"].reshape(-1)[0])
        self.pe = sine_pe_table(max_pos, self.D).to(**f32).contiguous()
        self.generation = 0     # bumped whenever a device pointer handed to an engine changes (engines re-create their ctx)
        # LayerNorm's affine part is folded into the Linear that follows it (one-time repack at load):
        #   Linear(LN(x)) = W (gamma * xhat + beta) + b = (W diag(gamma)) xhat + (b + W beta),  xhat = (x - mean) * rstd
        # so the decode GEMV only standardises x (in registers, no gamma/beta traffic); ln*_w / ln*_b become ones / zeros.
        self.ln_folded = True
        ones, zeros = torch.ones(self.D, **f32), torch.zeros(self.D, **f32)

        def fold(wk, bk, gk, bek):
            Wm, bm, gam, bet = g(wk), g(bk), g(gk), g(bek)
            return (Wm * gam.unsqueeze(0)).contiguous(), (bm.double() + Wm.double() @ bet.double()).to(torch.float32).contiguous()

        self.layers = []
        for l in range(self.L):
            p = f"decoder.layers.{l}."
            in_w, in_b = fold(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias", p + "norm1.weight", p + "norm1.bias")
            f1_w, f1_b = fold(p + "linear1.weight", p + "linear1.bias", p + "norm2.weight", p + "norm2.bias")
            self.layers.append(dict(
                ln1_w=ones, ln1_b=zeros, in_proj_w=in_w, in_proj_b=in_b,
                out_proj_w=g(p + "self_attn.out_proj.weight"), out_proj_b=g(p + "self_attn.out_proj.bias"),
                ln2_w=ones, ln2_b=zeros, ffn1_w=f1_w, ffn1_b=f1_b,
                ffn2_w=g(p + "linear2.weight"), ffn2_b=g(p + "linear2.bias")))
        self.lnf_w, self.lnf_b = ones, zeros
        gam, bet = g("decoder.norm.weight"), g("decoder.norm.bias")
        h1w = torch.cat([g(f"predict_layer.{k}.0.weight") for k in range(self.K)], 0)
        h1b = torch.cat([g(f"predict_layer.{k}.0.bias") for k in range(self.K)], 0)
        self.head1_w = (h1w * gam.unsqueeze(0)).contiguous()
        self.head1_b = (h1b.double() + h1w.double() @ bet.double()).to(torch.float32).contiguous()
        self.head2_w = torch.stack([g(f"predict_layer.{k}.2.weight") for k in range(self.K)]).contiguous()
        self.head2_b = torch.stack([g(f"predict_layer.{k}.2.bias") for k in range(self.K)]).contiguous()
        if weight_dtype == "e4m3":
            def quant(t):
                q, sc = quantize_e4m3(t)
                return e4m3_master(q, sc), sc.contiguous()
            for lay in self.layers:
                for name in W16_FAMILIES:
                    lay[name + "_w"], lay[name + "_w8s"] = quant(lay[name + "_w"])
            self.head1_w, self.head1_w8s = quant(self.head1_w)
            self.head2_w, self.head2_w8s = quant(self.head2_w)
        if weight_dtype == "bf16":
            rnd = lambda t: t.to(torch.bfloat16).to(torch.float32).contiguous()
            for lay in self.layers:
                for name in W16_FAMILIES:
                    lay[name + "_w"] = rnd(lay[name + "_w"])
            self.head1_w, self.head2_w = rnd(self.head1_w), rnd(self.head2_w)
        # planes per matrix in every `*_ws` buffer of this arena (3 or 1). It travels WITH the buffers: engines and `score` take it from
        # here when they hand the buffers to the library, never from the environment — a one-plane buffer read as three runs 2x its
        # size past its end. Decided once, by whichever of ensure_split_planes / ensure_head_split_planes runs first.
        self.split_planes = 3
        self._planes_decided = False

    @property
    def bf16_valued(self) -> bool:
        """Is every master of the six matrix families bf16-representable ("bf16": rounded to it; "e4m3": 4 significant bits times 2^e)?
        The one-plane prefill / score GEMM, the packed 2-byte streaming copies and their switches ask this, not the dtype's name."""
        return self.weight_dtype in BF16_VALUED

    def _ensure_packed(self, order: str) -> bool:
        if not self.bf16_valued:
            raise ValueError("packed bf16 copies need an arena built with weight_dtype='bf16' (the masters must hold the rounded values)")
        if getattr(self, f"_{order}_ready", False):
            return False
        to_order, streamable = PACKED_ORDERS[order]
        pack = lambda Wm: to_order(Wm) if streamable(Wm.shape[-1]) else None
        for lay in self.layers:
            for name in W16_FAMILIES:
                lay[f"{name}_{order}"] = pack(lay[name + "_w"])
        setattr(self, "head1_" + order, pack(self.head1_w))
        setattr(self, "head2_" + order, pack(self.head2_w))
        setattr(self, f"_{order}_ready", True)
        self.generation += 1
        return True

    def _packed_struct(self, order: str):
        w = _lib.LMW16()
        arrays = {}
        setattr(self, f"_{order}_arrays", arrays)       # the record points into them
        for name in W16_FAMILIES:
            if all(lay[f"{name}_{order}"] is not None for lay in self.layers):
                arrays[name] = (C.c_void_p * self.L)(*[lay[f"{name}_{order}"].data_ptr() for lay in self.layers])
                setattr(w, name + "_w16", C.cast(arrays[name], C.POINTER(C.c_void_p)))
        w.head1_w16, w.head2_w16 = _lib.ptr(getattr(self, "head1_" + order)), _lib.ptr(getattr(self, "head2_" + order))
        return w

    def ensure_w16_copies(self) -> bool:
        """Packed bf16 copies (`to_w16_order`) of the six matrix families for the <= 4-row decode step of a bf16 arena (+2 bytes per
        weight = +1.65 GB at 830M, built once on first use). A family whose inner dimension the kernels do not take (`w16_streamable`,
        e.g. d_model 128) gets none and streams its master. Returns True when the copies were created now."""
        return self._ensure_packed("w16")

    def w16_struct(self):
        """ssrhip_lm_w16 of the packed copies (NULL where a family has none)."""
        return self._packed_struct("w16")

    def _ensure_codes(self, order: str) -> bool:
        if self.weight_dtype != "e4m3":
            raise ValueError("packed e4m3 codes need an arena built with weight_dtype='e4m3' (the masters must hold codes * scale)")
        if getattr(self, f"_{order}_ready", False):
            return False
        to_order, streamable = CODE_ORDERS[order]
        pack = lambda Wm, sc: to_order(e4m3_codes(Wm, sc)) if streamable(Wm.shape[-1]) else None
        for lay in self.layers:
            for name in W16_FAMILIES:
                lay[f"{name}_{order}"] = pack(lay[name + "_w"], lay[name + "_w8s"])
        setattr(self, "head1_" + order, pack(self.head1_w, self.head1_w8s))
        setattr(self, "head2_" + order, pack(self.head2_w, self.head2_w8s))
        setattr(self, f"_{order}_ready", True)
        self.generation += 1
        return True

    def _codes_struct(self, order: str):
        """ssrhip_lm_w8 whose code pointers are the arena's `<family>_<order>` tensors ("w8": SSRHIP_W8_INDEX order, "wt8": SSRHIP_WT8_INDEX)"""
        w = _lib.LMW8()
        arrays = {}
        setattr(self, f"_{order}_arrays", arrays)       # the record points into them
        for name in W16_FAMILIES:
            if all(lay[f"{name}_{order}"] is not None for lay in self.layers):
                for suffix, field in (("_" + order, name + "_w8"), ("_w8s", name + "_s")):
                    arrays[field] = (C.c_void_p * self.L)(*[lay[name + suffix].data_ptr() for lay in self.layers])
                    setattr(w, field, C.cast(arrays[field], C.POINTER(C.c_void_p)))
        for h in ("head1", "head2"):
            if getattr(self, f"{h}_{order}") is not None:
                setattr(w, h + "_w8", getattr(self, f"{h}_{order}").data_ptr())
                setattr(w, h + "_s", getattr(self, h + "_w8s").data_ptr())
        return w

    def ensure_order(self, order: str) -> bool:
        """Build the copies of a Stream's `order` (PACKED_ORDERS / CODE_ORDERS) once; True when they were created now."""
        return (self._ensure_packed if order in PACKED_ORDERS else self._ensure_codes)(order)

    def order_struct(self, order: str):
        """The C record of that order's copies: ssrhip_lm_w16 (PACKED_ORDERS) or ssrhip_lm_w8 (CODE_ORDERS)."""
        return (self._packed_struct if order in PACKED_ORDERS else self._codes_struct)(order)

    def ensure_w8_copies(self) -> bool:
        """Packed e4m3 codes (`to_w8_order` of `e4m3_codes(master, scale)`, exact) of the six matrix families for the <= 4-row decode step of
        an e4m3 arena (+1 byte per weight = +0.82 GB at 830M beside the scales, built once on first use). A family whose inner dimension
        the kernels do not take (`w16_streamable`, e.g. d_model 128) gets none and streams its master. Returns True when created now."""
        return self._ensure_codes("w8")

    def w8_struct(self):
        """ssrhip_lm_w8 of the packed codes and their scales (NULL pairs where a family has no packed copy)."""
        return self._codes_struct("w8")

    def ensure_wt8_copies(self) -> bool:
        """The same in streaming order (`to_wt8_order`) for the 5..16-row decode step (+0.82 GB at 830M beside the scales and the fp32
        streaming copies). A family whose inner dimension is no multiple of 128 (`wt8_streamable`) gets none and streams its fp32
        streaming-order copy. Returns True when created now."""
        return self._ensure_codes("wt8")

    def wt8_struct(self):
        """ssrhip_lm_w8 of the SSRHIP_WT8_INDEX codes and their scales for ssrhip_lm_set_wt8 (NULL pairs where a family has no packed copy)."""
        return self._codes_struct("wt8")

    def ensure_wt16_copies(self) -> bool:
        """Packed bf16 streaming-order copies (`to_wt16_order`) of the six matrix families for the 5..32-row decode step of a bf16 arena
        (+2 bytes per weight = +1.65 GB at 830M beside the fp32 streaming copies, built once on first use). A family whose inner dimension
        is no multiple of 64 (`wt16_streamable`) gets none and streams its fp32 streaming-order copy. Returns True when created now."""
        return self._ensure_packed("wt16")

    def wt16_struct(self):
        """ssrhip_lm_w16 record of the SSRHIP_WT16_INDEX copies for ssrhip_lm_set_wt16 / _wt32 (NULL where a family has none)."""
        return self._packed_struct("wt16")

    def ensure_streaming_copies(self) -> bool:
        """Second copy of the six matrices of a decode step in the streaming order of the 5..16-row GEMV (one-time repack; used
        only by engines with more than 4 rows, +3.3 GB at 830M). Returns True when the copies were created now."""
        if getattr(self, "_wt_ready", False):
            return False
        for lay in self.layers:
            for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
                lay[name + "_wt"] = to_streaming_order(lay[name + "_w"])
        self.head1_wt = to_streaming_order(self.head1_w)
        self.head2_wt = to_streaming_order(self.head2_w)
        self._wt_ready = True
        self.generation += 1
        return True

    def _decide_planes(self, planes: Optional[int]) -> int:
        """The plane count of this arena's `*_ws` buffers: resolved once (SSRHIP_PREFILL_SPLIT / SSRHIP_PREFILL_W1 are read HERE and nowhere
        else), then fixed. 0 = none are built (now); a later call may still build them."""
        if self._planes_decided:
            if planes is not None and planes != self.split_planes:
                raise ValueError(f"this arena's split planes already come {self.split_planes} per matrix; {planes} asked for")
            resolve_prefill_planes(self.weight_dtype, planes, {})              # the argument's own checks
            return 0 if os.environ.get("SSRHIP_PREFILL_SPLIT", "1")[:1] == "0" else self.split_planes
        n = resolve_prefill_planes(self.weight_dtype, planes, os.environ)
        if n:
            self.split_planes, self._planes_decided = n, True
        return n

    def _planes_of(self, Wm: torch.Tensor) -> torch.Tensor:
        """int16 [split_planes * numel]: the three planes of the exact split (`ssrhip_split_weights`), or the one plane a bf16-valued
        master is — `to(bfloat16)` is exact there, no kernel needed."""
        if self.split_planes == 1:
            return Wm.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1)
        planes = torch.empty(3 * Wm.numel(), dtype=torch.int16, device=Wm.device)
        _lib.check(_lib.lib().ssrhip_split_weights(Wm.data_ptr(), planes.data_ptr(), Wm.numel(), _lib.stream_ptr()), "ssrhip_split_weights")
        return planes

    def ensure_split_planes(self, planes: Optional[int] = None) -> bool:
        """The four matrices of every layer as bf16 planes ([3][N][K], `ssrhip_split_weights`) for the PREFILL GEMMs: fp32 operands split
        exactly, six cross products on the bf16 matrix cores (csrc/gemm_split.hip; +6 bytes per weight = +4.8 GB at 830M, built once on
        first use). A bf16 arena with `SSRHIP_PREFILL_W1` on (unset: PREFILL_W1_DEFAULT; `planes=1` asks explicitly, `planes=3` for the
        split) builds ONE plane [N][K] instead — the weight itself, +2 bytes per weight, three products (ssrhip_gemm_w1), the same
        results bit for bit; `split_planes` says which. `planes=1` on an fp32 arena raises ValueError. `SSRHIP_PREFILL_SPLIT=0` keeps the
        prefill on the fp32 FMA chain: no planes at all. Returns True when created now."""
        if not self._decide_planes(planes) or getattr(self, "_ws_ready", False):
            return False
        for lay in self.layers:
            for name in ("in_proj", "out_proj", "ffn1", "ffn2"):
                lay[name + "_ws"] = self._planes_of(lay[name + "_w"])
        self._ws_ready = True
        self.generation += 1
        return True

    def ensure_head_split_planes(self, planes: Optional[int] = None) -> bool:
        """The two head matrices as `split_planes` bf16 planes each for the many-row head GEMMs of `ssrhip_lm_score` / `_score_w1`
        (ssrhip_score_args.head1_ws / head2_ws): head1_w [K*Hh][D] as one [planes][K*Hh][D], each codebook's head2_w[k] separately,
        [K][planes][card][Hh] (three planes: +6 bytes per head weight = +~100 MB at 830M). Same plane count as the layer planes (see
        `ensure_split_planes`); not built under `SSRHIP_PREFILL_SPLIT=0`. Returns True when created now. The decode step never reads
        them, so the engines' pointers do not change."""
        if not self._decide_planes(planes) or getattr(self, "_hs_ready", False):
            return False
        self.head1_ws = self._planes_of(self.head1_w)
        self.head2_ws = torch.cat([self._planes_of(self.head2_w[k]) for k in range(self.K)])
        self._hs_ready = True
        return True

    def split_plane_bytes(self) -> int:
        """Bytes this arena holds in split planes (layer and head buffers built so far)."""
        n = 0
        if getattr(self, "_ws_ready", False):
            n += sum(lay[name + "_ws"].numel() for lay in self.layers for name in ("in_proj", "out_proj", "ffn1", "ffn2"))
        if getattr(self, "_hs_ready", False):
            n += self.head1_ws.numel() + self.head2_ws.numel()
        return 2 * n

    def ensure_positions(self, n: int) -> bool:
        """Grow the sinusoidal table so that positions [0, n) exist, like `SinePositionalEmbedding.extend_pe` does on demand
        (models/modules/embedding.py:66-92: no length limit in the reference). Returns True when the table was rebuilt
        (its device pointer changed: engines built on the old one must be discarded)."""
        if n <= self.max_pos:
            return False
        self.max_pos = ((int(n) + 4095) // 4096) * 4096
        self.pe = sine_pe_table(self.max_pos, self.D).to(dtype=torch.float32, device=self.device).contiguous()
        self.generation += 1
        return True

    def nbytes_per_step(self) -> int:
        """Algorithmic weight bytes one decode step must stream."""
        n = 0
        for lay in self.layers:
            n += sum(t.numel() for k, t in lay.items() if not k.endswith(("_wt", "_ws", "_w16", "_wt16", "_w8", "_w8s", "_wt8")))     # incl. the (now constant) LayerNorm vectors, as SURVEY §8d counts them
        n += self.lnf_w.numel() + self.lnf_b.numel()
        n += self.head1_w.numel() + self.head1_b.numel() + self.head2_w.numel() + self.head2_b.numel()
        n += (self.K + 1) * self.D  # K embedding rows + one pe row
        half = 0                    # weights that have a packed bf16 copy stream 2 bytes each (the copy's zero-padded rows are not weights)
        order = next((o for o in PACKED_ORDERS if getattr(self, f"_{o}_ready", False)), None)
        if order is not None:
            half = sum(lay[name + "_w"].numel() for lay in self.layers for name in W16_FAMILIES if lay[f"{name}_{order}"] is not None)
            half += sum(m.numel() for m, h in ((self.head1_w, "head1_"), (self.head2_w, "head2_")) if getattr(self, h + order) is not None)
        codes = next((o for o in ("_w8", "_wt8") if getattr(self, o + "_ready", False)), None)
        if codes is not None:                       # a family with packed e4m3 codes streams 1 byte per weight and one fp32 scale per output row
            fams = [(lay[name + "_w"], lay[name + codes], lay[name + "_w8s"]) for lay in self.layers for name in W16_FAMILIES]
            fams += [(self.head1_w, getattr(self, "head1" + codes), self.head1_w8s), (self.head2_w, getattr(self, "head2" + codes), self.head2_w8s)]
            return 4 * n - sum(3 * m.numel() - 4 * sc.numel() for m, q, sc in fams if q is not None)
        return 4 * n - 2 * half

    def c_struct(self):
        w = _lib.LMWeights()
        w.text_emb, w.audio_emb, w.pe = self.text_emb.data_ptr(), self.audio_emb.data_ptr(), self.pe.data_ptr()
        w.alpha_text, w.alpha_audio = self.alpha_text, self.alpha_audio
        self._arrays = {}
        for name in ("ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln2_w", "ln2_b",
                     "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b"):
            arr = (C.c_void_p * self.L)(*[lay[name].data_ptr() for lay in self.layers])
            self._arrays[name] = arr
            setattr(w, name, C.cast(arr, C.POINTER(C.c_void_p)))
        w.lnf_w, w.lnf_b = self.lnf_w.data_ptr(), self.lnf_b.data_ptr()
        w.head1_w, w.head1_b = self.head1_w.data_ptr(), self.head1_b.data_ptr()
        w.head2_w, w.head2_b = self.head2_w.data_ptr(), self.head2_b.data_ptr()
        if getattr(self, "_wt_ready", False):
            for name in ("in_proj_wt", "out_proj_wt", "ffn1_wt", "ffn2_wt"):
                arr = (C.c_void_p * self.L)(*[lay[name].data_ptr() for lay in self.layers])
                self._arrays[name] = arr
                setattr(w, name, C.cast(arr, C.POINTER(C.c_void_p)))
            w.head1_wt, w.head2_wt = self.head1_wt.data_ptr(), self.head2_wt.data_ptr()
        if getattr(self, "_ws_ready", False):
            for name in ("in_proj_ws", "out_proj_ws", "ffn1_ws", "ffn2_ws"):
                arr = (C.c_void_p * self.L)(*[lay[name].data_ptr() for lay in self.layers])
                self._arrays[name] = arr
                setattr(w, name, C.cast(arr, C.POINTER(C.c_void_p)))
        return w

    def dims(self):
        return _lib.LMDims(self.D, self.H, self.L, self.F, self.K, self.card, self.Hh, self.n_text, self.max_pos, int(self.ln_folded))


MAX_ROWS = 32             # rows of one lock-step engine: two 16-column MFMA panels (gemv_mfma32.hip)
DEFAULT_GROUP_ROWS = 16   # rows per engine pass that inference_batch / dp.* use unless `group` says otherwise (8 utterances with CFG)


class PagePool:
    """Host-side allocator of the paged KV cache's physical pages (replaces the dense `past` tensor the reference re-concatenates
    every step, models/ssr.py:685-686 / modules/activation.py:626-631). A free list; pages are handed to a row when its
    sequence is about to cross into a new 128-position page and go back when its utterance is done. `order` fixes the order
    in which an untouched pool hands pages out (tests pass a shuffled one; the kernels only ever see the table). A page may have more
    than one holder (`share`: the prompt pages of rows with the same prompt); it is free again when the last holder gives it back."""

    def __init__(self, n_pages: int, order: Optional[Sequence[int]] = None):
        self.n_pages = int(n_pages)
        order = list(range(self.n_pages)) if order is None else [int(p) for p in order]
        if sorted(order) != list(range(self.n_pages)):
            raise ValueError("page order must be a permutation of range(n_pages)")
        self._order = order
        self.reset()

    def reset(self):
        self._free = self._order[::-1]          # pop() hands out order[0] first
        self._owner = {}
        self._holders = {}                      # page -> how many rows hold it (take: 1, share: + 1)
        self.handed_out = []                    # (page, owner) in hand-out order since the last reset (tests / debugging)

    @property
    def n_free(self) -> int:
        return len(self._free)

    def take(self, owner) -> int:
        if not self._free:
            raise RuntimeError(f"KV page pool exhausted ({self.n_pages} pages of {PAGE} positions): raise pool_pages")
        p = self._free.pop()
        self._owner[p] = owner
        self._holders[p] = 1
        self.handed_out.append((p, owner))
        return p

    def share(self, page: int, owner) -> int:
        """One more holder of a page somebody holds already (its first taker stays its `owner`; the new holder is entered in
        `handed_out` like a taker)."""
        if page not in self._owner:
            raise RuntimeError(f"page {page} shared while nobody holds it")
        self._holders[page] += 1
        self.handed_out.append((page, owner))
        return page

    def holders(self, page: int) -> int:
        return self._holders.get(page, 0)

    def give_back(self, pages: Sequence[int]):
        for p in pages:
            if p not in self._owner:
                raise RuntimeError(f"page {p} returned twice (or never taken)")
            self._holders[p] -= 1
            if self._holders[p] == 0:
                del self._owner[p], self._holders[p]
                self._free.append(p)


class IntStaging:
    """One-copy staging of an admission's integer arrays: packed back to back into a pinned int32 buffer, sent asynchronously into its
    persistent device twin, addressed there by views (ten small synchronous pageable copies per admit stalled the rows that
    were still decoding). When the buffers may be reused, and what must be idle before larger ones replace them, differs between the
    blocking and the two-phase admission and stays with them."""

    def __init__(self):
        self.pinned = self.dev = None
        self.capacity = 0

    @staticmethod
    def offsets(sizes: Sequence[int]):
        """(where each part starts, total) for parts of these sizes packed back to back"""
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + int(n))
        return offs[:-1], offs[-1]

    @staticmethod
    def grown(total: int, old: int) -> int:
        return max(int(total), 2 * int(old), 4096)

    def grow(self, total: int, device):
        self.capacity = self.grown(total, self.capacity)
        self.pinned = torch.empty(self.capacity, dtype=torch.int32).pin_memory()
        self.dev = torch.empty(self.capacity, dtype=torch.int32, device=device)

    def pack(self, parts: Sequence[np.ndarray]):
        """Write the parts, flattened, into the host buffer; returns `offsets` of their sizes."""
        offs, total = self.offsets([p.size for p in parts])
        host = self.pinned.numpy()
        for o, p in zip(offs, parts):
            host[o:o + p.size] = p.astype(np.int32, copy=False).reshape(-1)
        return offs, total

    def send(self, parts: Sequence[np.ndarray], stream=None) -> List[torch.Tensor]:
        """Pack the parts (the capacity must suffice) and issue the ONE host-to-device copy on `stream` (None: the current one);
        returns the device view of each part."""
        offs, total = self.pack(parts)
        with torch.cuda.stream(stream):
            self.dev[:total].copy_(self.pinned[:total], non_blocking=True)
        return [self.dev[o:o + p.size] for o, p in zip(offs, parts)]


def noise_segments(drawn: Sequence[int], slots: Sequence[int], chunk: int, limit: int):
    """Which steps' noise to draw next: per slot u of `slots`, in order, (u, off, n) = its next `chunk` steps from off = drawn[u], cut
    at `limit`; slots that have reached the limit are left out."""
    segs = [(u, drawn[u], min(chunk, limit - drawn[u])) for u in slots]
    return [s for s in segs if s[2] > 0]


class NoiseUploader:
    """The host-noise pipeline of a sampled run: draw a chunk of steps through a `TorchCpuNoiseFeed` into pinned staging memory and send it
    to `noise[u, off:off + n]` on a copy stream while the GPU decodes the chunk before (a 16-step chunk is ~14 ms of GPU time at 830M, its
    draws ~3 ms of host time). Three staging buffers [n_utt, chunk, K, card]: the chunk's index & 1 is the steady-state ring, 2 holds the
    first chunk of newly admitted slots. A buffer's `free` event (its last upload has finished) outlives the run, as the buffer does: the
    next run's first `send` into it waits for the previous run's last look-ahead."""

    def __init__(self, noise: torch.Tensor, chunk: int):
        self.noise, self.chunk = noise, chunk
        self.bufs = [torch.empty(noise.shape[0], chunk, *noise.shape[2:], dtype=torch.float32).pin_memory() for _ in range(3)]
        self.stream = torch.cuda.Stream(noise.device)
        self.free: List[Optional[torch.cuda.Event]] = [None] * 3
        self.feed, self.pending = None, []                      # pending: the uploads the next decode has to wait for

    def begin(self, feed: "TorchCpuNoiseFeed"):
        self.feed, self.pending = feed, []

    @staticmethod
    def fill(feed: "TorchCpuNoiseFeed", buf: torch.Tensor, slots: Sequence[int], chunk: int, limit: int):
        """The host half: draw the segments `noise_segments` names into buf[u, :n] (CPU, pinned or not); returns them."""
        segs = noise_segments(feed.drawn, slots, chunk, limit)
        for u, _, n in segs:
            feed.draw(u, buf[u, :n])
        return segs

    def send(self, buf_i: int, slots: Sequence[int], limit: int):
        """Draw the next chunk of `slots` (steps below `limit`) into staging buffer buf_i and send it; `wait` orders a stream after it."""
        if self.free[buf_i] is not None:
            self.free[buf_i].synchronize()                      # the upload that last used this staging buffer has finished
        segs = self.fill(self.feed, self.bufs[buf_i], slots, self.chunk, limit)
        with torch.cuda.stream(self.stream):
            for u, off, n in segs:
                self.noise[u, off:off + n].copy_(self.bufs[buf_i][u, :n], non_blocking=True)
        self.free[buf_i] = self.stream.record_event()
        self.pending.append(self.free[buf_i])

    def wait(self, stream):
        for ev in self.pending:
            stream.wait_event(ev)
        self.pending = []


class TorchCpuNoiseFeed:
    """The Exp(1) tensors `torch.multinomial(probs[K, card], 1)` draws on the CPU — one `exponential_` of the logits' shape per
    decode step (reference models/ssr.py:85 via :713/:732; checked in oracle/make_golden.py::make_sampler) — produced a chunk of
    steps at a time so that the host draws for steps [s, s+n) while the GPU decodes the previous chunk. One contiguous
    `[n, K, card].exponential_()` consumes the generator exactly like n successive per-step draws (tests/test_noise_feed.py).

    generators[u] is utterance u's `torch.Generator`, or None for the global CPU generator (what the reference uses).
    `finish(u, n_taken)` puts that generator in the state it has after exactly `n_taken` per-step draws, i.e. where the
    reference leaves it — chunks drawn ahead of the stop are un-drawn."""

    _chunk_ok: dict = {}             # (K, card) -> does ONE [n, K, card] draw consume the generator like n [K, card] draws on this build?

    @classmethod
    def chunked_draws_match(cls, K: int, card: int) -> bool:
        """Self-check of the assumption above, once per shape and process: torch builds whose CPU `exponential_` seeds a per-call
        stream (some MKL/VSL configurations) would give a chunked draw other numbers than per-step draws — sampled runs would then
        silently stop reproducing `torch.multinomial`. On a mismatch the feed draws step by step into the same staging buffer."""
        key = (int(K), int(card))
        if key not in cls._chunk_ok:
            g1, g2 = torch.Generator().manual_seed(987654321), torch.Generator().manual_seed(987654321)
            a = torch.empty(3, K, card).exponential_(1, generator=g1)
            b = torch.stack([torch.empty(K, card).exponential_(1, generator=g2) for _ in range(3)])
            cls._chunk_ok[key] = bool(torch.equal(a, b)) and bool(torch.equal(g1.get_state(), g2.get_state()))
        return cls._chunk_ok[key]

    def __init__(self, generators, K: int, card: int):
        self.gens = list(generators)
        self.K, self.card = K, card
        self.chunked = self.chunked_draws_match(K, card)
        self.marks = [[] for _ in self.gens]      # per utterance: (first step of the chunk, generator state before drawing it)
        self.drawn = [0] * len(self.gens)

    def _get(self, u):
        g = self.gens[u]
        return torch.get_rng_state() if g is None else g.get_state()

    def _set(self, u, st):
        g = self.gens[u]
        if g is None:
            torch.set_rng_state(st)
        else:
            g.set_state(st)

    def draw(self, u: int, out: torch.Tensor):
        """Fill `out` [n, K, card] (CPU, may be pinned) with the draws of the next n steps of utterance u."""
        self.marks[u].append((self.drawn[u], self._get(u)))
        if self.chunked:
            out.exponential_(1, generator=self.gens[u])
        else:
            for i in range(out.shape[0]):
                out[i].exponential_(1, generator=self.gens[u])
        self.drawn[u] += out.shape[0]

    def reset_slot(self, u: int, generator, seed: int = 0):
        """Slot u now serves another utterance with its own generator (continuous batching): forget the old stream's bookkeeping.
        (`seed` is what `PhiloxNoise` takes from the same call; this stream IS the generator.)"""
        self.gens[u] = generator
        self.marks[u] = []
        self.drawn[u] = 0

    def finish(self, u: int, n_taken: int):
        if n_taken >= self.drawn[u]:
            return
        s0, st = [m for m in self.marks[u] if m[0] <= n_taken][-1]
        self._set(u, st)
        if n_taken > s0:
            if self.chunked:
                torch.empty(n_taken - s0, self.K, self.card).exponential_(1, generator=self.gens[u])
            else:
                for _ in range(n_taken - s0):
                    torch.empty(self.K, self.card).exponential_(1, generator=self.gens[u])
        self.drawn[u] = n_taken


def philox_fill(noise: torch.Tensor, segs: Sequence[tuple], words: Optional[torch.Tensor] = None):
    """Enqueue, on the current stream, the device-side draws of `segs` = (slot, first_step, n_steps, seed) into `noise`
    [n_utt, max_steps, K, card] (include/ssrhip.h ssrhip_noise_philox; one launch per _lib.NOISE_MAX_SEGMENTS segments). `words`
    (tests): an int32 tensor of the same shape that receives the raw Philox words."""
    n_utt, max_steps, K, card = noise.shape
    assert noise.dtype == torch.float32 and noise.is_contiguous(), (noise.dtype, noise.stride())
    assert words is None or (words.dtype == torch.int32 and words.is_contiguous() and words.shape == noise.shape)
    for i in range(0, len(segs), _lib.NOISE_MAX_SEGMENTS):
        part = segs[i:i + _lib.NOISE_MAX_SEGMENTS]
        a = _lib.NoiseArgs()
        a.noise, a.words = noise.data_ptr(), _lib.ptr(words)
        a.n_utt, a.max_steps, a.K, a.card, a.n_seg = int(n_utt), int(max_steps), int(K), int(card), len(part)
        for s, (u, off, n, seed) in zip(a.seg, part):
            s.slot, s.first_step, s.n_steps = int(u), int(off), int(n)
            s.seed_lo, s.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        _lib.check(_lib.lib().ssrhip_noise_philox(C.byref(a), _lib.stream_ptr()), "ssrhip_noise_philox")


class PhiloxNoise:
    """The device-side noise source of a sampled run (sampling_rng "philox", DESIGN.md Part I.21): feed and uploader in one object, with the
    interface the decode loops use for `TorchCpuNoiseFeed` and `NoiseUploader` — `begin`, `send`, `wait`, `reset_slot`, `finish`, `drawn`.
    `send` enqueues ONE kernel on the current (decode) stream that writes the Exp(1) draws of the next chunk of steps into
    `noise[u, off:off + n]`; stream order does the rest, so `wait` and the staging-buffer index mean nothing here. No host draw, no pinned
    staging, no copy stream, no generator to rewind: `finish` only takes back the count of steps drawn ahead of the stop.
    seeds[u] is slot u's utterance seed (`DecodeKnobs.seed`); a value depends on (seed, step, element) only — not on the slot, the batch,
    the chunking or a refill. `launch(segments)` (tests: a fake) receives the list of (slot, first_step, n_steps, seed)."""

    on_device = True

    def __init__(self, seeds: Sequence[int], launch=None):
        self.seeds = [int(s) for s in seeds]
        self.drawn = [0] * len(self.seeds)
        self.noise, self.chunk, self.launch = None, 16, launch

    def bind(self, noise: Optional[torch.Tensor], chunk: int) -> "PhiloxNoise":
        """A decode loop starts (`DecodeEngine._begin_run`): the buffer to write and the chunk of steps per `send`"""
        self.noise, self.chunk = noise, chunk
        if self.launch is None:
            self.launch = lambda segs: philox_fill(self.noise, segs)
        return self

    def begin(self, feed=None):
        pass

    def send(self, buf_i: int, slots: Sequence[int], limit: int):
        """Enqueue the draws of the next chunk of `slots` (steps below `limit`); `buf_i` is ignored: nothing is staged."""
        segs = noise_segments(self.drawn, slots, self.chunk, limit)
        if segs:
            self.launch([(u, off, n, self.seeds[u]) for u, off, n in segs])
        for u, _, n in segs:
            self.drawn[u] += n

    def wait(self, stream):
        pass

    def reset_slot(self, u: int, generator=None, seed: int = 0):
        """Slot u now serves another utterance: its seed, and its steps count from 0 again."""
        self.seeds[u] = int(seed)
        self.drawn[u] = 0

    def finish(self, u: int, n_taken: int):
        if n_taken < self.drawn[u]:
            self.drawn[u] = n_taken


def make_noise_feed(sampling_rng: str, n_slots: int, K: int, card: int):
    """The noise source of a sampled queue run over `n_slots` utterance slots whose jobs arrive later (`reset_slot`)"""
    if resolve_sampling_rng(sampling_rng) == "philox":
        return PhiloxNoise([0] * n_slots)
    return TorchCpuNoiseFeed([None] * n_slots, K, card)


class DecodeEngine:
    """B rows (= n_utt x (2 if CFG else 1)) decoded in lock-step; one captured hipGraph per engine."""

    def __init__(self, arena: LMWeightsArena, n_utt: int, use_cfg: bool, max_seq: int, max_steps: int, debug_logits: bool = False,
                 pool_pages: Optional[int] = None, page_order: Optional[Sequence[int]] = None, pair_mode: int = 0,
                 stream_w16: Optional[bool] = None, stream_wt16: Optional[bool] = None, stream_wt32: Optional[bool] = None,
                 kv_dtype: Optional[str] = None, share_prompt: Optional[bool] = None, stream_w8: Optional[bool] = None,
                 pair_w16: Optional[bool] = None, pair_w8: Optional[bool] = None, stream_wt8: Optional[bool] = None,
                 kv16_small: Optional[bool] = None, pair4: Optional[bool] = None, pair4_pk: Optional[bool] = None,
                 logprobs: bool = False):
        """max_seq: longest sequence (text + audio positions) any ONE row may reach.
        pool_pages: physical KV pages shared by all rows (default rows x pages-per-row, the no-sharing worst case; a batch of short and
        long utterances needs only the sum of their own page counts).
        pair_mode (include/ssrhip.h ssrhip_lm_buffers): 0 = pair launches if this engine gets its device's pairing slot, 1 = never,
        2 = always (tests of the give-up path).
        stream_w16 / stream_wt16 / stream_wt32 / stream_w8 / stream_wt8: the step streams that entry of STREAMS; None = its switch decides.
        pair_w16 / pair_w8 / pair4 / pair4_pk: the step asks for that entry of PAIR_FORMS; None = its switch decides.
        kv_dtype: "bf16" = the paged pool holds 2-byte entries (`resolve_kv_dtype`: 5..32 rows; include/ssrhip.h ssrhip_lm_set_kv16); None = "fp32".
        kv16_small: the bf16 cache of the 1/2/4-row step behind a landing cache (`resolve_kv16_small`, `kv_landing_bytes`, DESIGN.md Part I.23).
        share_prompt: rows admitted TOGETHER with equal text and prompt audio are prefilled once and share the prompt's whole KV pages
        (`resolve_share_prompt`, DESIGN.md Part I.15); refills and the two-phase admission (`admit_begin`) never share. None = off.
        logprobs: the sampler also writes every generated token's log-probability (`logprobs()`, `queue_logprobs`; DESIGN.md Part I.27).
        All of them are decided by `resolve_decode_plan` (the switches are read there, from os.environ) before anything is allocated;
        `self.plan` keeps the answer. Every choice gives the same tokens, bit for bit, on the same arena and cache type."""
        self.lib = _lib.lib()
        self.a = arena
        dev = arena.device
        self.device = dev
        self.n_utt = n_utt
        self.use_cfg = use_cfg
        self.rows_per_utt = 2 if use_cfg else 1
        self.B = n_utt * self.rows_per_utt
        self.plan = resolve_decode_plan(self.B, arena.weight_dtype, arena.L, max_seq, os.environ, pair_mode, kv_dtype, share_prompt, kv16_small, logprobs,
                                        stream_w16=stream_w16, stream_wt16=stream_wt16, stream_wt32=stream_wt32, stream_w8=stream_w8,
                                        stream_wt8=stream_wt8, pair_w16=pair_w16, pair_w8=pair_w8, pair4=pair4, pair4_pk=pair4_pk)
        self.max_pages = self.plan.max_pages
        self.max_seq = self.max_pages * PAGE
        arena.ensure_positions(self.max_seq)      # every text / audio position of a row is < its sequence capacity
        if self.B > 4:
            arena.ensure_streaming_copies()       # the matrix-core GEMV streams W in its own order
        arena.ensure_split_planes()               # the prefill GEMMs run on the bf16 matrix cores with exactly split operands
        if self._stream is not None:
            arena.ensure_order(self._stream.order)    # the step streams packed 2-byte weights or 1-byte codes and their scales
        self.max_steps = max_steps
        D, H, L, K = arena.D, arena.H, arena.L, arena.K
        self.hd = D // H
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        n_pages = self.B * self.max_pages if pool_pages is None else int(pool_pages)
        self.pages = PagePool(n_pages, page_order)
        self.scratch_page = n_pages              # one extra page: where the rows of a FINISHED utterance keep (harmlessly) writing
        self.kv_pool = torch.empty((n_pages + 1) * L * 2 * H * PAGE * self.hd, device=dev,
                                   dtype=torch.bfloat16 if self.kv_dtype == "bf16" else torch.float32)
        # kv16_small: the QKV launch's fp32 landing cache [B][1][2][H][PAGE][hd], its page table (row b owns page b) and the positions the
        # layers append at (layer l: position l) — written here, once; the captured step only holds their pointers
        self.kv_land = torch.zeros(self.B * 2 * H * PAGE * self.hd, **f32) if self.kv16_small else None
        self.kv_land_table = torch.arange(self.B, **i32) if self.kv16_small else None
        self.kv_land_pos = torch.arange(L, **i32).repeat_interleave(self.B).contiguous() if self.kv16_small else None
        self.page_table = torch.full((self.B, self.max_pages), self.scratch_page, **i32)
        self._table_host = np.full((self.B, self.max_pages), self.scratch_page, dtype=np.int32)
        self._row_pages: List[List[int]] = [[] for _ in range(self.B)]
        # prompt sharing: chunk_head[r] = the lowest row of r's attention chunk, n_shared[r] (read at the head) = how many leading table
        # entries the chunk's rows have in common; identity and 0 = no sharing. The device twins are what the captured step reads.
        self.group_members = int(self.lib.ssrhip_attn_group_members()) if self.share_prompt else 1
        self._chunk_host = np.stack([np.arange(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)])
        self.chunk_dev = torch.from_numpy(self._chunk_host.copy()).to(dev) if self.share_prompt else None
        self._chunks: List[List[int]] = []       # the chunks of more than one row that are live
        self.prefilled_rows = 0                  # rows the last blocking admission prefilled
        self._kv0 = [0] * self.B                 # sequence length of each row after the prefill
        self._steps_enqueued = 0
        self._admit_step = [0] * n_utt           # value of _steps_enqueued when the slot's current utterance was admitted
        self.n_admitted = 0                      # utterances admitted since the last start / run_queue (tests: refill happened)
        self.n_refills = 0                       # ... of which into a slot another utterance had used before
        self._utt_live = [False] * n_utt
        # two-phase admission (run_queue): a slot that is being prefilled on the side stream. Its rows own KV pages, but the table the decode
        # step reads still shows the scratch page for them — the pages are entered in `page_table_warm`, which only that prefill reads.
        self._utt_warm = [False] * n_utt
        self.page_table_warm = torch.full((self.B, self.max_pages), self.scratch_page, **i32)
        self._table_warm_host = np.full((self.B, self.max_pages), self.scratch_page, dtype=np.int32)
        self._side_stream = None
        self._warm_stage = IntStaging()           # one-copy staging of a two-phase admission's integer arrays
        self._warm_free = None                    # event: the last activation has read the warm staging buffers
        self.t_first_chunk = 0.0
        # > 4 rows: x / q / h are 16-column tiled buffers, one 16-row panel per 16 rows (include/ssrhip.h SSRHIP_TILED_P)
        rows = self.B if self.B <= 4 else 16 * ((self.B + 15) // 16)
        self.x = torch.zeros(rows, D, **f32)
        self.q = torch.zeros(rows, D, **f32)
        self.h = torch.zeros(rows, max(arena.F, K * arena.Hh), **f32)
        self.logits = torch.zeros(self.B, K, arena.card, **f32)
        self.part_o = torch.zeros(self.B * H * self.max_pages * self.hd, **f32)
        self.part_ml = torch.zeros(self.B * H * self.max_pages * 2, **f32)
        self.next_tok = torch.zeros(self.B, MAX_CODEBOOKS, **i32)
        self.next_pos = torch.zeros(self.B, **i32)
        self.kv_pos = torch.zeros(self.B, **i32)
        self.row_len = torch.zeros(self.B, **i32)
        self.cfg_dev = torch.zeros(n_utt * C.sizeof(_lib.SamplerCfg), dtype=torch.uint8, device=dev)
        self.state_dev = torch.zeros(n_utt * C.sizeof(_lib.SamplerState), dtype=torch.uint8, device=dev)
        self.generated = torch.zeros(n_utt, max_steps, K, **i32)
        self.logp = torch.full((n_utt, max_steps, K), float("nan"), **f32) if self.want_logprobs else None
        self.queue_logprobs: List[np.ndarray] = []   # run_queue with logprobs: float32 [n_steps, K] per job, in job order
        # ONE persistent buffer for host-drawn sampling noise: its pointer is baked into the captured graph, so generations
        # with / without host noise reuse the same context (ssrhip_sampler_cfg.use_noise selects per utterance)
        self.noise = torch.empty(n_utt, max_steps, K, arena.card, **f32)
        self._uploader: Optional[NoiseUploader] = None         # host-noise pipeline of sampled runs, kept across runs
        self._feed, self._polled = None, False                 # the current run's noise feed (None: no host noise); has it been polled?
        self._admit_stage = IntStaging()          # one-copy staging of a blocking admission's integer arrays ...
        self._admit_sent = None                   # ... and the event of its last copy
        self._prefill_ws = None
        self._arena_gen = arena.generation
        self.dbg_logits = torch.zeros(n_utt, K, arena.card, **f32) if debug_logits else None
        self._take_weights()
        self._ctx = None
        self.pairing = False                      # set by _create_ctx: does this engine's step run the pair launches?
        self.pairing_why = ""

    # ------------------------------------------------------------------ C structs
    def kv_struct(self):
        return _lib.KV(self.kv_pool.data_ptr(), self.page_table.data_ptr(), self.max_pages, self.a.L, self.a.H, self.hd)

    def _take_weights(self):
        """The arena's weights record, and WITH it how many planes its `*_ws` buffers hold (0 = the record has none)."""
        self._w = self.a.c_struct()
        self.prefill_planes = self.a.split_planes if getattr(self.a, "_ws_ready", False) else 0

    def _create_ctx(self):
        if self._ctx is not None:
            self.lib.ssrhip_lm_destroy(self._ctx)
            self._ctx = None
        b = _lib.LMBuffers()
        b.B, b.n_utt, b.max_splits, b.pair_mode = self.B, self.n_utt, self.max_pages, self.pair_mode
        b.x, b.q, b.h, b.logits = self.x.data_ptr(), self.q.data_ptr(), self.h.data_ptr(), self.logits.data_ptr()
        b.part_o, b.part_ml = self.part_o.data_ptr(), self.part_ml.data_ptr()
        b.next_tok, b.next_pos = self.next_tok.data_ptr(), self.next_pos.data_ptr()
        b.kv_pos, b.row_len = self.kv_pos.data_ptr(), self.row_len.data_ptr()
        b.kv = self.kv_struct()
        b.cfg, b.state = self.cfg_dev.data_ptr(), self.state_dev.data_ptr()
        b.noise = self.noise.data_ptr()
        b.generated = self.generated.data_ptr()
        b.dbg_logits = self.dbg_logits.data_ptr() if self.dbg_logits is not None else 0
        d = self.a.dims()
        ctx = C.c_void_p()
        _lib.check(self.lib.ssrhip_lm_create(C.byref(d), C.byref(self._w), C.byref(b), C.byref(ctx)), "ssrhip_lm_create")
        self._ctx = ctx
        if self._stream is not None:              # before the first step is enqueued or captured; a <= 4-row stream gives the pairing slot back
            rec, setter = self.a.order_struct(self._stream.order), "ssrhip_lm_set_" + self._stream.name
            _lib.check(getattr(self.lib, setter)(ctx, C.byref(rec)), setter)
        if self.plan.pair is not None and self.pair_mode != 1:    # (check_pairs sets pair_mode 1 after a give-up: that engine steps unpaired)
            setter = "ssrhip_lm_set_" + self.plan.pair.c_name     # over the stream set above, or the fp32 masters (pair4)
            _lib.check(getattr(self.lib, setter)(ctx, 1), setter)
        if self.kv16_small:                       # <= 4 rows: the 2-byte pool and the landing cache of the QKV launch's append
            _lib.check(self.lib.ssrhip_lm_set_kv16_small(ctx, self.kv_land.data_ptr(), self.kv_land_table.data_ptr(), self.kv_land_pos.data_ptr()),
                       "ssrhip_lm_set_kv16_small")
        elif self.kv_dtype == "bf16":             # the pool's entry type travels with the pool (also for the two-phase admission's prefill)
            _lib.check(self.lib.ssrhip_lm_set_kv16(ctx, 1), "ssrhip_lm_set_kv16")
        if self.share_prompt:                     # the two arrays' pointers travel with the captured step
            _lib.check(self.lib.ssrhip_lm_set_prompt_groups(ctx, self.chunk_dev[0].data_ptr(), self.chunk_dev[1].data_ptr()),
                       "ssrhip_lm_set_prompt_groups")
            # the step's launches are built for the size THIS engine cuts its chunks to, whatever the knob says when a step is enqueued
            _lib.check(self.lib.ssrhip_lm_set_group_members(ctx, self.group_members), "ssrhip_lm_set_group_members")
        if self.prefill_planes == 1:              # the count travels with the arena's buffers (also for the two-phase admission's prefill)
            _lib.check(self.lib.ssrhip_lm_set_prefill_w1(ctx, 1), "ssrhip_lm_set_prefill_w1")
        if self.want_logprobs:                    # the step ends in ssrhip_sample_logp; the buffer's pointer travels with the captured step
            _lib.check(self.lib.ssrhip_lm_set_logprobs(ctx, self.logp.data_ptr()), "ssrhip_lm_set_logprobs")
        why = C.create_string_buffer(256)
        self.pairing = bool(self.lib.ssrhip_lm_pairing(ctx, why, 256))
        self.pairing_why = why.value.decode(errors="replace")

    def _launches_per_step(self, name: str) -> int:       # the `<name>_launches_per_step` properties (COUNTERS, below the class)
        return 0 if self._ctx is None else int(getattr(self.lib, f"ssrhip_lm_{name}_launches")(self._ctx))

    @property
    def kv_pool_bytes(self) -> int:
        """Bytes of the paged KV pool this engine holds (half as many with kv_dtype="bf16")."""
        return self.kv_pool.numel() * self.kv_pool.element_size()

    @property
    def kv_landing_bytes(self) -> int:
        """Bytes of the fp32 landing cache a kv16_small engine holds beside its pool (rows x 2 x d_model x 128 x 4; 0 otherwise)."""
        return 0 if self.kv_land is None else self.kv_land.numel() * self.kv_land.element_size()

    def close(self):
        if self._ctx is not None:
            self.lib.ssrhip_lm_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ set-up of one generation
    def start(self, text_rows: List[np.ndarray], audio_cols: List[np.ndarray], knobs: List[DecodeKnobs],
              noise: Optional[torch.Tensor] = None, host_noise: bool = False):
        """text_rows[b]: int array [L_b] (row b's text ids); audio_cols[u]: int array [K, T0_u]
        (layout-built prompt columns, WITHOUT the mask token that starts generation);
        knobs[u]. Runs the prefill and arms the decode state.

        Sampling noise: `noise` [n_utt, steps, K, card] (any device) is copied into the engine's buffer now; `host_noise=True`
        promises that `run_to_completion(feed=...)` will stream it in chunk by chunk; neither = on-device RNG (knobs.seed)."""
        a = self.a
        K = a.K
        assert len(text_rows) == self.B and len(audio_cols) == self.n_utt and len(knobs) == self.n_utt
        self._reset_generation()                 # KV pages: everything back to the pool; every slot is (re)admitted
        if noise is not None:
            assert noise.dim() == 4 and noise.shape[0] == self.n_utt and tuple(noise.shape[2:]) == (K, a.card), noise.shape
            n = min(noise.shape[1], self.max_steps)
            self.noise[:, :n].copy_(noise[:, :n].to(torch.float32), non_blocking=True)
            if n < self.max_steps:
                self.noise[:, n:].fill_(1.0)          # steps past the supplied draws: a defined value, never uninitialised memory
        rpu = self.rows_per_utt
        return self.admit(list(range(self.n_utt)), [text_rows[u * rpu:(u + 1) * rpu] for u in range(self.n_utt)], list(audio_cols), list(knobs),
                          use_noise=(noise is not None or host_noise))

    def _reset_generation(self):
        """What `start` and `run_queue` begin from: every KV page back in the pool, every slot free, the counters at zero. The two-phase
        form's warm state goes too (a `run_queue` that raised between `admit_begin` and `admit_finish` must not leave any behind)."""
        self.pages.reset()
        self._table_host[:] = self.scratch_page
        self._table_warm_host[:] = self.scratch_page
        self._row_pages = [[] for _ in range(self.B)]
        self._chunks = []
        self._chunk_host[0], self._chunk_host[1] = np.arange(self.B, dtype=np.int32), 0
        self._kv0 = [0] * self.B
        self._steps_enqueued = 0
        self._admit_step = [0] * self.n_utt
        self._utt_live = [False] * self.n_utt
        self._utt_warm = [False] * self.n_utt
        self.n_admitted = self.n_refills = 0

    # ------------------------------------------------------------------ admission: the steps both forms are made of
    def _book_admission(self, slots, text_rows, audio_cols, knobs, share: bool = False):
        """Checks the slots (free, their rows without KV pages, every sequence within the engine's capacity: ValueError before anything is
        booked or enqueued), packs the prefill rows of the new sequences — one per engine row b, with b as its seq_id — and books their
        prompt lengths. Returns (rows b, packed rows, the int32 parts of the ONE staged copy: tok[R][4] | pos[R] | kind[R] | seq[R] |
        rpos[R] | rlen[R] | seq_start[n+1] | next_tok[rows][4] | t0[rows] | kv0[rows] | row index[rows]).
        share: only the LEADERS of `plan_prompt_sharing` (and the rows without company) are packed — a follower books its leader's prompt
        length and is armed like every row; the plan is left in `self._plan` for `admit`."""
        K, rpu = self.a.K, self.rows_per_utt
        assert len(slots) == len(text_rows) == len(audio_cols) == len(knobs) and len(set(slots)) == len(slots)
        seqs = []
        for u, trs, au in zip(slots, text_rows, audio_cols):
            assert 0 <= u < self.n_utt and not self._utt_live[u] and len(trs) == rpu, (u, len(trs))
            for r in range(rpu):
                assert not self._row_pages[u * rpu + r], "slot still owns KV pages"
                seqs.append((u * rpu + r, trs[r], au))
        self._plan = plan_prompt_sharing(seqs, self.group_members) if share else None
        packed = [sq for sq in seqs if self._plan[0][sq[0]] == sq[0]] if share else seqs
        pk = pack_prefill_rows(packed, K)
        if int(pk["lens"].max()) + 1 > self.max_seq:
            raise ValueError("sequence exceeds engine capacity")
        rows_b = [b for b, _, _ in seqs]
        len_of = {sq[0]: int(n) for sq, n in zip(packed, pk["lens"])}
        lens = np.asarray([len_of[self._plan[0][b]] if share else len_of[b] for b in rows_b], dtype=pk["lens"].dtype)
        for b, n in zip(rows_b, lens):
            self._kv0[b] = int(n)
        self.n_admitted += len(slots)
        # first decode input of the new rows: the span-0 mask token at audio position T0 (ssr.py:655-662)
        nt = np.zeros((len(rows_b), MAX_CODEBOOKS), dtype=np.int32)
        nt[:, :K] = int(self.a.args.mts)
        t0 = np.asarray([np.asarray(au).shape[1] for _, _, au in seqs], dtype=np.int32)
        parts = [pk[k] for k in ("tok", "pos", "kind", "row_seq", "row_pos", "row_len", "seq_start")]
        return rows_b, pk, parts + [nt, t0, lens, np.asarray(rows_b, dtype=np.int32)]

    def _slot_records(self, slots, knobs, audio_cols, use_noise: bool):
        """Sampler configuration / initial state of the slots, as the arrays of C records the device reads."""
        args = self.a.args
        cfgs = (_lib.SamplerCfg * len(slots))()
        sts = (_lib.SamplerState * len(slots))()
        for c, st, kn, au in zip(cfgs, sts, knobs, audio_cols):
            c.top_k, c.top_p, c.temperature, c.stop_repetition = int(kn.top_k), float(kn.top_p), float(kn.temperature), int(kn.stop_repetition)
            c.cfg_coef, c.cfg_one_minus = float(kn.cfg_coef), float(1 - kn.cfg_coef)
            c.cfg_stride, c.use_cfg = int(kn.cfg_stride), int(self.use_cfg)
            sil = list(kn.silence_tokens)[: _lib.MAX_SILENCE]
            c.n_silence = len(sil)
            for j, sv in enumerate(sil):
                c.silence[j] = int(sv)
            c.text_len, c.n_spans = int(kn.text_len), int(kn.n_spans)
            c.empty_token, c.eog, c.eos, c.sos = int(args.empty_token), int(args.eog), int(args.eos), int(args.sos)
            c.mts, c.max_n_spans, c.max_steps = int(args.mts), int(args.max_n_spans), int(self.max_steps)
            c.seed_lo, c.seed_hi = int(kn.seed) & 0xFFFFFFFF, (int(kn.seed) >> 32) & 0xFFFFFFFF
            c.use_noise = int(use_noise)
            st.span, st.num_gen, st.num_eog, st.num_cfg_tag, st.prev_token, st.consec_silence = 0, 0, 0, 1, -1, 0
            st.audio_pos = int(np.asarray(au).shape[1])
            st.n_steps, st.done = 0, 0
        return cfgs, sts

    def _write_slot_records(self, slots, cfgs=None, sts=None):
        """`cfgs[i]` / `sts[i]` (ctypes arrays of SamplerCfg / SamplerState; None: leave alone) into slot slots[i] of `cfg_dev` /
        `state_dev`, on the caller's stream: ONE copy per buffer when the slots are all of them in order, one per slot otherwise."""
        as_bytes = lambda rec: torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8)
        pairs = [(dst, recs) for dst, recs in ((self.cfg_dev, cfgs), (self.state_dev, sts)) if recs is not None]
        if list(slots) == list(range(self.n_utt)):
            for dst, recs in pairs:
                dst.copy_(as_bytes(recs))
            return
        for i, u in enumerate(slots):
            for dst, recs in pairs:
                n = C.sizeof(recs[i])
                dst[u * n:(u + 1) * n].copy_(as_bytes(recs[i]))

    def _arm_rows(self, rows_b, nt, t0, kv0, rows_d):
        """Pending input token, its audio position, cache position and row length of the new rows, from the staged views (the last four
        parts of `_book_admission`), on the caller's stream. Returns the index tensor it used (None when every row is armed)."""
        nt = nt.view(-1, MAX_CODEBOOKS)
        if rows_b == list(range(self.B)):        # every row (the first fill): plain copies, no index tensor
            self.next_tok.copy_(nt)
            self.next_pos.copy_(t0)
            self.kv_pos.copy_(kv0)
            self.row_len.copy_(kv0 + 1)
            return None
        idx = rows_d.long()
        self.next_tok.index_copy_(0, idx, nt)
        self.next_pos.index_copy_(0, idx, t0)
        self.kv_pos.index_copy_(0, idx, kv0)
        self.row_len.index_copy_(0, idx, kv0 + 1)
        return idx

    def _prefill_ws_rows(self) -> int:
        return 0 if self._prefill_ws is None else self._prefill_ws["x"].shape[0]

    def _launch_prefill(self, p) -> None:
        """`ssrhip_lm_prefill` of the argument block `p` on the current stream: the ONE place a prefill is enqueued from (blocking start /
        admission, and the two-phase admission inside its side-stream context). A measuring tool may wrap this method on an engine instance
        to put device events around the prefill (tools/prefill_time.py)."""
        _lib.check(self.lib.ssrhip_lm_prefill(self._ctx, C.byref(p), _lib.stream_ptr()), "ssrhip_lm_prefill")

    def _prefill_args(self, pk, views):
        """The prefill workspaces (kept across admissions, grown when a larger prompt arrives) and the argument block of ONE
        `ssrhip_lm_prefill` over the packed rows, whose integer arrays are the first seven staged views. Returns (args, workspaces): the
        caller launches, and keeps the workspaces alive until its stream has consumed them."""
        a = self.a
        f32 = dict(dtype=torch.float32, device=self.device)
        D, F, H = a.D, a.F, a.H
        R, max_len = int(pk["tok"].shape[0]), int(pk["lens"].max())
        ms = (max_len + PAGE - 1) // PAGE
        if self._prefill_ws_rows() < R:
            Rc = max(R, int(1.25 * self._prefill_ws_rows()))
            self._prefill_ws = dict(x=torch.empty(Rc, D, **f32), xn=torch.empty(Rc, D, **f32), qkv=torch.empty(Rc, 3 * D, **f32),
                                    o=torch.empty(Rc, D, **f32), h=torch.empty(Rc, F, **f32))
        ws = dict(self._prefill_ws)
        if os.environ.get("SSRHIP_PREFILL_ATTN_ROWWISE", "0") not in ("", "0"):      # A/B knob: the round-1 per-row attention needs its partials
            ws.update(part_o=torch.empty(R * H * ms * self.hd, **f32), part_ml=torch.empty(R * H * ms * 2, **f32))
        # rows of one sequence are contiguous and in position order: the tiled prefill attention needs only where each starts (seq_start)
        p = _lib.PrefillArgs()
        for name, v in zip(("tok", "pos", "kind", "row_seq", "row_pos", "row_len", "seq_start"), views):
            setattr(p, name, v.data_ptr())
        p.R, p.max_splits, p.n_seq, p.max_len = R, ms, len(pk["lens"]), max_len
        for k, v in ws.items():
            setattr(p, k, v.data_ptr())
        return p, ws

    # ------------------------------------------------------------------ admission: the blocking and the two-phase form
    def admit(self, slots: Sequence[int], text_rows: Sequence[Sequence[np.ndarray]], audio_cols: Sequence[np.ndarray],
              knobs: Sequence[DecodeKnobs], use_noise: bool = False):
        """Put new utterances into the utterance slots `slots` (free ones: never used, or released by `release_utterance`) while
        the other slots keep decoding: KV pages from the pool, sampler configuration / state, pending input token, and the
        PREFILL of just those rows (the reference prefills one utterance at a time anyway: models/ssr.py:627-642). Everything is
        ordered on the caller's stream between two decode chunks; the captured step graph is untouched (it only holds pointers).
        text_rows[i]: the 1 (or 2 with CFG) text rows of slot slots[i]; audio_cols[i]: [K, T0]. Returns the prefilled row count.
        A share_prompt engine shares in its FIRST admission since `start` / `run_queue` began (the rows that arrive together): only one
        row of every group of equal prompts is prefilled, so the count shrinks. Later admissions (refills) never share."""
        a, dev = self.a, self.device
        share = self.share_prompt and self.n_admitted == 0
        rows_b, pk, parts = self._book_admission(slots, text_rows, audio_cols, knobs, share)
        for u in slots:
            self._utt_live[u] = True
            self._admit_step[u] = self._steps_enqueued
        tails = self._share_pages(*self._plan) if share else []
        self._grow_pages(0)                      # pages for the prompts (+ the first decoded position) of the new rows
        stage = self._admit_stage
        total = sum(p_.size for p_ in parts)
        if stage.capacity < total:
            stage.grow(total, dev)
            self._admit_sent = None
        if self._admit_sent is not None:
            self._admit_sent.synchronize()       # the previous admission's copy has left the staging buffer (admissions are >= 16 steps apart)
        views = stage.send(parts)
        self._admit_sent = torch.cuda.Event()
        self._admit_sent.record(torch.cuda.current_stream(dev))
        self._write_slot_records(slots, *self._slot_records(slots, knobs, audio_cols, use_noise))
        if self._arena_gen != a.generation:      # the arena re-allocated a table (position table grown): refresh the pointers
            self._take_weights()
            self._arena_gen = a.generation
            self.close()
        if self._ctx is None:
            self._create_ctx()
        idx = self._arm_rows(rows_b, *views[7:])
        p, ws = self._prefill_args(pk, views)
        # (the prefill ends by embedding the pending input token of EVERY row into x: for rows in mid-decode that re-writes the
        # very values the sampler's fused embedding left there — same function, same inputs)
        self._launch_prefill(p)
        if tails:
            # a prompt that ends inside a page: the follower appends into its OWN page from position n on, and reads the leader's
            # positions below n there — one contiguous block of the pool per (leader, follower), copied behind the prefill
            pool = self.kv_pool.view(self.pages.n_pages + 1, -1)
            for lead, f in tails:
                e = self._kv0[f] // PAGE
                pool[int(self._table_host[f, e])].copy_(pool[int(self._table_host[lead, e])])
        self.prefilled_rows = int(pk["tok"].shape[0])
        self._keep = (ws, idx)                   # alive until the stream has consumed them (the integer arrays live in the engine's workspace)
        return int(pk["tok"].shape[0])

    def admit_begin(self, slots: Sequence[int], text_rows: Sequence[Sequence[np.ndarray]], audio_cols: Sequence[np.ndarray],
                    knobs: Sequence[DecodeKnobs], use_noise: bool = False) -> dict:
        """First half of a TWO-PHASE admission (continuous batching without stalling the live rows): KV pages for the new rows, the
        integer arrays and the PREFILL of just those rows on a SIDE stream — concurrently with the decode chunks of the rows that keep
        running; the decode step does not see the new rows yet (their slots stay parked: `done` set, table rows on the scratch page; the
        prefill reads `page_table_warm`). `admit_finish(handle)` later puts them into the lock-step batch. Returns the handle."""
        dev = self.device
        assert self._arena_gen == self.a.generation and self._ctx is not None, "two-phase admission needs the running engine's context"
        assert not any(self._utt_warm[u] for u in slots)
        rows_b, pk, parts = self._book_admission(slots, text_rows, audio_cols, knobs)
        for u in slots:
            self._utt_warm[u] = True
        for b in rows_b:                         # pages for the prompts (+ the first decoded position), entered in the WARM table only
            for have in range(min(self._kv0[b] // PAGE + 1, self.max_pages)):
                pg = self.pages.take(b)
                self._row_pages[b].append(pg)
                self._table_warm_host[b, have] = pg
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(dev)
        side, stage = self._side_stream, self._warm_stage
        total = sum(p_.size for p_ in parts)
        if stage.capacity < total:
            torch.cuda.synchronize(dev)          # growth is rare: nothing in flight may still read the old buffer, and the new block (allocated
            stage.grow(total, dev)               # on this stream, used on the side stream) has no pending user
        side.synchronize()                       # the previous two-phase prefill is through (>= one 16-step chunk ago): its staging is free
        if self._warm_free is not None:
            side.wait_event(self._warm_free)     # ... and the activation that read the staging views has run
        views = stage.send(parts, side)
        with torch.cuda.stream(side):
            self.page_table_warm.copy_(torch.from_numpy(self._table_warm_host))
        # the decode step must not see the new slots yet: admit_finish writes cfg / state / pending token
        cfgs, sts = self._slot_records(slots, knobs, audio_cols, use_noise)
        if self._prefill_ws_rows() < pk["tok"].shape[0]:
            torch.cuda.synchronize(dev)          # (rare) the workspace is allocated on this stream and used on the side stream
        p, ws = self._prefill_args(pk, views)
        # on the SIDE stream, against the warm table, without the closing embedding (x is live decode state)
        p.table, p.no_embed = self.page_table_warm.data_ptr(), 1
        with torch.cuda.stream(side):
            self._launch_prefill(p)
            done = torch.cuda.Event()
            done.record(side)
        return dict(slots=list(slots), rows_b=rows_b, prefill_done=done, cfgs=cfgs, sts=sts, arm=views[7:], ws=ws)

    def admit_finish(self, h: dict) -> None:
        """Second half: on the caller's (decode) stream, behind the side stream's prefill — sampler configuration / state, pending token,
        cache position and the table rows of the new slots, then the embedding of the pending tokens (every row: for rows in mid-decode
        that re-writes what the sampler's fused embedding left). A few small device copies; the rows step with the next chunk."""
        main = torch.cuda.current_stream(self.device)
        main.wait_event(h["prefill_done"])
        self._write_slot_records(h["slots"], h["cfgs"], h["sts"])
        self._arm_rows(h["rows_b"], *h["arm"])
        for u in h["slots"]:
            self._utt_warm[u] = False
            self._utt_live[u] = True
            self._admit_step[u] = self._steps_enqueued
            for b in range(u * self.rows_per_utt, (u + 1) * self.rows_per_utt):
                self._table_host[b, :] = self._table_warm_host[b, :]
                self._table_warm_host[b, :] = self.scratch_page
        self.page_table.copy_(torch.from_numpy(self._table_host))
        _lib.check(self.lib.ssrhip_lm_embed_pending(self._ctx, _lib.stream_ptr()), "ssrhip_lm_embed_pending")
        self._warm_free = torch.cuda.Event()
        self._warm_free.record(main)
        self._keep_warm = h                       # the workspaces and the staging views stay alive until the stream has consumed them

    # ------------------------------------------------------------------ KV page bookkeeping
    def _grow_pages(self, steps_ahead: int):
        """Make sure every row of a live utterance owns the pages for positions [0, kv0 + steps_ahead] (the decode step at
        sequence length S appends position S), round-robin over rows so that concurrent rows interleave in the pool, then
        push the table if it changed. Ordered on the caller's stream before the launches that need it."""
        want = [0] * self.B
        for b in range(self.B):
            u = b // self.rows_per_utt
            if self._utt_live[u]:       # steps this row has been through = steps enqueued since ITS utterance was admitted
                want[b] = min((self._kv0[b] + max(steps_ahead - self._admit_step[u], 0)) // PAGE + 1, self.max_pages)
        changed = False
        more = True
        while more:
            more = False
            for b in range(self.B):
                have = len(self._row_pages[b])
                if have < want[b]:
                    p = self.pages.take(b)
                    self._row_pages[b].append(p)
                    self._table_host[b, have] = p
                    changed = more = True
        if changed:
            self._push_table()                    # pageable source: staged before this call returns

    def _share_pages(self, leader, chunks):
        """The page side of a sharing admission, before `_grow_pages` hands out what is left: a leader takes the n // PAGE WHOLE pages of
        its prompt (n = `_kv0`) and every follower holds them too (`PagePool.share`), as the first entries of its table row; the entry
        behind them (where position n is appended) stays each row's own. Enters the chunks into the two arrays (pushed with the table by
        `_grow_pages`, which always has a page to hand out here). Returns the (leader, follower) pairs whose prompt ends inside a page."""
        tails = []
        for lead in sorted(set(leader.values())):
            followers = [b for b, l_ in sorted(leader.items()) if l_ == lead and b != lead]
            ns = self._kv0[lead] // PAGE
            if not followers:
                continue
            for i in range(ns):
                pg = self.pages.take(lead)
                self._row_pages[lead].append(pg)
                self._table_host[lead, i] = pg
                for f in followers:
                    self._row_pages[f].append(self.pages.share(pg, f))
                    self._table_host[f, i] = pg
            if self._kv0[lead] % PAGE:
                tails += [(lead, f) for f in followers]
        # a chunk is worth a workgroup of its own only where it has pages in common
        self._chunks = [list(c) for c in chunks if len(c) > 1 and self._kv0[c[0]] // PAGE > 0]
        self._enter_chunks()
        return tails

    def _enter_chunks(self):
        self._chunk_host[0], self._chunk_host[1] = np.arange(self.B, dtype=np.int32), 0
        for c in self._chunks:
            self._chunk_host[0, c] = c[0]
            self._chunk_host[1, c[0]] = self._kv0[c[0]] // PAGE

    def release_utterance(self, u: int):
        """Utterance u is done: its rows' pages go back to the pool and the rows are pointed at the scratch page (they stay in
        the lock-step batch and keep appending at a frozen position; nothing reads what they produce). Rows that shared their prompt
        leave their chunk (the lowest row that stays becomes its head); a shared page is free when its last holder has let go."""
        if not self._utt_live[u]:
            return
        self._utt_live[u] = False
        gone = range(u * self.rows_per_utt, (u + 1) * self.rows_per_utt)
        for b in gone:
            self.pages.give_back(self._row_pages[b])
            self._row_pages[b] = []
            self._table_host[b, :] = self.scratch_page
        if self._chunks:
            self._chunks = [c for c in ([b for b in c if b not in gone] for c in self._chunks) if len(c) > 1]
            self._enter_chunks()
        self._push_table()

    def _push_table(self):
        self.page_table.copy_(torch.from_numpy(self._table_host))
        if self.share_prompt:                     # the chunks travel with the table they describe
            self.chunk_dev.copy_(torch.from_numpy(self._chunk_host))

    # ------------------------------------------------------------------ decode
    def decode(self, n_steps: int, use_graph: bool = True):
        self._steps_enqueued += int(n_steps)
        self._grow_pages(self._steps_enqueued)
        _lib.check(self.lib.ssrhip_lm_decode(self._ctx, int(n_steps), int(use_graph), _lib.stream_ptr()), "ssrhip_lm_decode")

    def check_pairs(self) -> None:
        """Raise if a pair launch of this engine's step gave up (csrc/gemv.hip gemv_pair_kernel: a workgroup that waited ~1 s for the other
        255 — something else held CUs for that long — flags it and the step's results are garbage from there on). EVERY way a token
        leaves the engine goes through here first (`states`, `tokens`). The library hands the pairing slot to one engine per device
        (ssrhip_lm_create), so this needs a foreign kernel that squats on CUs; when it happens the engine recreates its context WITHOUT
        pair launches — the utterances in flight are lost (their KV cache is garbage), the next `start` / `run_queue` is correct."""
        if not self.pairing:
            return
        rc = self.lib.ssrhip_lm_pair_status(self._ctx, _lib.stream_ptr())
        if rc == 1:
            self.plan = self.plan._replace(pair_mode=1)
            self._create_ctx()                    # destroys the context (gives the slot back), new one steps with the ordinary launches
            raise RuntimeError("a paired GEMV launch of the decode step gave up waiting for its other workgroups (another kernel held CUs "
                               "for about a second): every token since the last poll is invalid and the utterances in flight must be "
                               "submitted again. This engine now steps without pair launches (same tokens, ~5 % slower).")
        _lib.check(rc, "ssrhip_lm_pair_status")

    def states(self) -> List[_lib.SamplerState]:
        raw = bytes(self.state_dev.cpu().numpy().tobytes())
        self.check_pairs()
        arr = (_lib.SamplerState * self.n_utt).from_buffer_copy(raw)
        return list(arr)

    def tokens(self, u: int, n: int, start: int = 0) -> np.ndarray:
        """The generated steps [start, n) of slot u as int64 [n - start, K] — after the pair-launch check (never read `generated`
        directly)."""
        out = self.generated[u, start:n].cpu().numpy().astype(np.int64)
        self.check_pairs()
        return out

    def logprobs(self, u: int, n: int, start: int = 0) -> np.ndarray:
        """The log-probabilities of the generated steps [start, n) of slot u as float32 [n - start, K], NaN where the state machine
        decided the token (include/ssrhip.h ssrhip_sample_logp) — `tokens()` for an engine built with logprobs=True, after the same
        pair-launch check."""
        if self.logp is None:
            raise RuntimeError("this engine was built without logprobs=True: its step does not write log-probabilities")
        out = self.logp[u, start:n].cpu().numpy()
        self.check_pairs()
        return out

    def run_to_completion(self, chunk: int = 16, use_graph: bool = True, max_total: Optional[int] = None,
                          feed: Optional[TorchCpuNoiseFeed] = None, on_chunk=None):
        """Decode in chunks of `chunk` steps until every utterance reports done (the flags are polled once per chunk).
        With `feed`, the host draws and uploads the NEXT chunk's sampling noise while the GPU runs the current chunk (`NoiseUploader`);
        a `PhiloxNoise` as `feed` writes it on the device instead, between two chunks on this stream.
        `on_chunk(states)` is called after every poll with the states read there (`iter_chunks` is the same loop as a generator)."""
        states = None
        for states in self.iter_chunks(chunk, use_graph, max_total, feed):
            if on_chunk is not None:
                on_chunk(states)
        return states

    def iter_chunks(self, chunk: int = 16, use_graph: bool = True, max_total: Optional[int] = None,
                    feed: Optional[TorchCpuNoiseFeed] = None):
        """`run_to_completion` as a generator: yields the sampler states after every poll (the rows they count exist on the device; read
        them with `tokens`), the last yield being the final states. The consumer's work runs between two chunks on the caller's stream;
        the noise feed is put back (`feed.finish`) when the loop ends, so a sampled run has to be consumed to its end."""
        total = 0
        limit = self.max_steps if max_total is None else min(max_total, self.max_steps)
        live = list(range(self.n_utt))
        up = self._begin_run(chunk, feed)
        if up:
            up.send(0, live, limit)                             # overlaps with the prefill `start()` enqueued
        states = None
        while total < limit:
            n = min(chunk, limit - total)
            if up:
                up.wait(torch.cuda.current_stream(self.device))
            self.decode(n, use_graph)
            total += n
            if up and total < limit:
                up.send(total // chunk & 1, live, limit)        # host draws the next chunk while the GPU runs this one
            states = self._poll()                               # blocks until that chunk has finished
            live = [u for u, s_ in enumerate(states) if not s_.done]
            for u, s_ in enumerate(states):
                if s_.done:
                    self.release_utterance(u)
            if not live or total >= limit:
                break
            yield states
        states = states or self.states()                        # a limit of 0 steps: nothing was decoded
        if feed is not None:
            for u, s_ in enumerate(states):
                feed.finish(u, int(s_.n_steps))
        yield states

    def _begin_run(self, chunk: int, feed):
        """A decode loop starts: not polled yet and, with a feed, the engine's one uploader (rebuilt only when `chunk` changes) on it. A
        `PhiloxNoise` is its own uploader: it writes `noise` on the decode stream, and nothing is built for it."""
        self._polled, self._feed = False, feed
        if feed is None:
            return None
        if getattr(feed, "on_device", False):
            return feed.bind(self.noise, chunk)
        if self._uploader is None or self._uploader.chunk != chunk:
            self._uploader = NoiseUploader(self.noise, chunk)
        self._uploader.begin(feed)
        return self._uploader

    def _poll(self) -> List[_lib.SamplerState]:
        """`states()`; a run's first poll is when its first `chunk` frames exist (bench: time to first frames)"""
        states = self.states()
        if not self._polled:
            self._polled, self.t_first_chunk = True, time.perf_counter()
        return states

    # ------------------------------------------------------------------ continuous batching
    def run_queue(self, jobs: Sequence[dict], chunk: int = 16, use_graph: bool = True, sampling: bool = False):
        """Decode a QUEUE of utterances through this engine's utterance slots with row refill: the slots run in lock-step; every
        `chunk` steps the done flags are read, a finished utterance's tokens are collected and its KV pages released, and the next
        pending utterance is admitted into those rows (`admit`: prefill of just those rows, sampler state reset, same graph). A
        lock-step group would instead idle its finished rows until its longest member ends. The reference runs utterances one
        after the other (inference_v2.py:331-333); the result of each job does not depend on what shares the engine with it.

        jobs[i]: {text_rows: [row0(, row1)], audio_cols: [K, T0], knobs: DecodeKnobs, gen: torch.Generator | None (sampling),
        cap: max steps of this utterance, rng: "torch_cpu" | "philox" (sampling; optional, one value per queue: with "philox" the noise is
        drawn on the device from knobs.seed and `gen` is not consumed)}. Returns a list of (SamplerState, generated int64 [n_steps, K]) in job order."""
        it = self.iter_queue(jobs, chunk, use_graph, sampling)
        while True:
            try:
                next(it)
            except StopIteration as done:
                return done.value

    def iter_queue(self, jobs: Sequence[dict], chunk: int = 16, use_graph: bool = True, sampling: bool = False):
        """`run_queue` as a generator: yields `(states, slot_job)` after every poll — the sampler states read there and, per slot, the
        job it runs (None: idle) — before the finished utterances are collected; the rows the states count exist on the device and the
        pair-launch check has passed. The consumer's work runs between two chunks on the caller's stream. `StopIteration.value` is the
        list `run_queue` returns; the generator has to be consumed to its end (the noise feed is put back there)."""
        n_jobs = len(jobs)
        results: List[Optional[tuple]] = [None] * n_jobs
        self.queue_logprobs = [None] * n_jobs if self.want_logprobs else []   # filled where the tokens are collected, in job order
        if n_jobs == 0:
            return results
        slot_job: List[Optional[int]] = [None] * self.n_utt
        local: List[int] = [0] * self.n_utt           # steps enqueued for the slot's current utterance
        # longest (by its step cap) first: the utterances that will run longest start earliest and the short ones fill the slots freed
        # towards the end — the tail with a few long utterances on a mostly idle engine shrinks (simulated on the bench's ragged queue:
        # 344 -> 327 chunks). Which utterance sits in which slot when does not change any result.
        pending = sorted(range(n_jobs), key=lambda j: -int(jobs[j]["cap"])) if n_jobs > self.n_utt else list(range(n_jobs))
        # the noise source is the run's: every job names the same one ("rng", SAMPLING_RNGS; absent = "torch_cpu")
        rngs = sorted({j.get("rng", "torch_cpu") for j in jobs})
        if len(rngs) != 1:
            raise ValueError(f"the jobs of one queue name different sampling noise sources: {rngs}")
        feed = make_noise_feed(rngs[0], self.n_utt, self.a.K, self.a.card) if sampling else None
        up = self._begin_run(chunk, feed)

        # Two-phase admission is built, bit-exact and OFF by default: on the bench's ragged queue (64 utterances through 8
        # slots, 56 refills) it measured 19,785 codec-tokens/s against 19,930 for the blocking form, same token CRC
        # (profiles/r05_microbench/dp64_ragged_two_phase_ab.log). The 9 ms of prefill work do not disappear by moving to a side stream: the
        # prefill's workgroups take CU slots from the decode step's 83 dependent launches, each of which then starts late — the two
        # time-slice the GPU instead of overlapping HBM-bound with matrix-bound work — and the admitted slot idles one more 16-step chunk.
        two_phase = os.environ.get("SSRHIP_ADMIT_TWO_PHASE", "0") not in ("", "0")

        def take_jobs(slots: Sequence[int]):
            take = [pending.pop(0) for _ in slots[: len(pending)]]
            return list(slots[: len(take)]), take

        def job_args(take: Sequence[int]):
            return [jobs[j]["text_rows"] for j in take], [jobs[j]["audio_cols"] for j in take], [jobs[j]["knobs"] for j in take]

        def now_running(slots: Sequence[int], take: Sequence[int]):
            """slots[i] runs job take[i] from the next chunk on: the queue's bookkeeping, the slot's noise stream"""
            for u, j in zip(slots, take):
                slot_job[u] = j
                local[u] = 0
                if up:
                    feed.reset_slot(u, jobs[j].get("gen"), jobs[j]["knobs"].seed)
            if up:
                up.send(2, slots, self.max_steps)               # the new utterances' first chunk, before their first step

        def admit_into(slots: Sequence[int]):
            """blocking admission (the first fill; refills with SSRHIP_ADMIT_TWO_PHASE=0): prefill on the decode stream"""
            slots, take = take_jobs(slots)
            if take:
                self.admit(slots, *job_args(take), use_noise=sampling)
                now_running(slots, take)

        def begin_into(slots: Sequence[int]):
            """two-phase admission, first half: the prefill of the new rows starts on the side stream NOW and overlaps the decode chunk that
            is already enqueued; the slots join the lock-step batch at the next poll (`admit_finish`, then `now_running`)"""
            slots, take = take_jobs(slots)
            return (self.admit_begin(slots, *job_args(take), use_noise=sampling), take) if take else None

        # first fill: as `start` (pool reset), but only as many slots as there are jobs; the others stay parked on the scratch page
        self._reset_generation()
        # idle slots: done = 1 so that the sampler leaves them alone
        idle = (_lib.SamplerState * self.n_utt)()
        for st in idle:
            st.done = 1
        self._write_slot_records(range(self.n_utt), sts=idle)
        self.page_table.copy_(torch.from_numpy(self._table_host))
        admit_into(list(range(self.n_utt)))
        warm = None                                             # handle of the slots being prefilled on the side stream

        def enqueue_chunk():
            """one more chunk for the slots that run a job; returns them: the slots stepping in the chunk that is enqueued and not yet polled"""
            if up:
                up.wait(torch.cuda.current_stream(self.device))
            stepping = [u for u in range(self.n_utt) if slot_job[u] is not None]
            self.decode(chunk, use_graph)
            for u in stepping:
                local[u] += chunk
            if up:
                up.send(self._steps_enqueued // chunk & 1, stepping, self.max_steps)     # the host draws while the GPU runs this chunk
            return stepping

        in_flight = enqueue_chunk()
        while True:
            states = self._poll()                               # blocks until the enqueued chunk has finished
            yield states, list(slot_job)
            for u in in_flight:
                j = slot_job[u]
                cap_j = min(int(jobs[j]["cap"]), self.max_steps)
                if states[u].done or local[u] >= cap_j:
                    if self.want_logprobs:                      # the same rows as the tokens, at the same poll, before a refill's start
                        self.queue_logprobs[j] = self.logprobs(u, int(states[u].n_steps))
                    results[j] = self._collect(u, states[u], cap_j)
                    slot_job[u] = None
            # the slots whose prefill was started one poll ago join the batch now (their prefill had a whole chunk to finish)
            if warm is not None:
                self.admit_finish(warm[0])
                now_running(warm[0]["slots"], warm[1])
                warm = None
            free_slots = [u for u in range(self.n_utt) if slot_job[u] is None]
            if two_phase and any(j is not None for j in slot_job):
                # keep the GPU busy FIRST: the next chunk of the live rows is enqueued before the host prepares the admission, whose
                # prefill then overlaps that chunk on the side stream
                in_flight = enqueue_chunk()
                if free_slots and pending:
                    self.n_refills += min(len(free_slots), len(pending))
                    warm = begin_into(free_slots)
                continue
            if free_slots and pending:                          # nothing is decoding (or the knob is off): the blocking form
                self.n_refills += min(len(free_slots), len(pending))
                admit_into(free_slots)
            if not any(j is not None for j in slot_job):
                break
            in_flight = enqueue_chunk()
        return results

    def _collect(self, u: int, st, cap_j: int):
        """Slot u's utterance finished, or ran into its cap of cap_j steps, at the poll that read `st`: its (state snapshot, generated
        int64 [n_steps, K]); the slot's noise stream is put back, its pages are released and the slot is left parked."""
        n = int(st.n_steps)
        if st.done and n > cap_j:
            # the flags are polled every `chunk` steps: an utterance may finish up to chunk - 1 steps past ITS OWN cap before the
            # poll sees it. The fixed-group path bounded every member by the group's cap; here the bound is per utterance, and a
            # result longer than its cap is the same failure as not finishing (the caller raises on done != 1).
            st.done = 2
        gen = self.tokens(u, n)
        snap = _lib.SamplerState.from_buffer_copy(bytes(st))
        if self._feed is not None:
            self._feed.finish(u, n)
        if not st.done:                                         # ran into its cap without finishing: park the slot (the caller raises)
            parked = (_lib.SamplerState * 1)(_lib.SamplerState.from_buffer_copy(bytes(st)))
            parked[0].done = 1
            self._write_slot_records([u], sts=parked)
        self.release_utterance(u)
        return snap, gen

    def time_kernels(self, n_steps: int):
        """Event-timed eager steps: list of (kind, avg_us) per launch slot of one decode step
        (kind: 'gemv' | 'attn' | 'sample')."""
        self._steps_enqueued += int(n_steps)
        self._grow_pages(self._steps_enqueued)
        n_out = 8 * self.a.L + 16
        us = (C.c_float * n_out)()
        kind = (C.c_int32 * n_out)()
        n = self.lib.ssrhip_lm_time_steps(self._ctx, int(n_steps), _lib.stream_ptr(), us, kind, n_out)
        if n < 0:
            _lib.check(n, "ssrhip_lm_time_steps")
        names = ("gemv", "attn", "sample")
        return [(names[kind[i]], float(us[i])) for i in range(n)]

    def time_category(self, kind: str, n_replays: int = 50):
        """(avg_us_per_launch, launches_per_step) of one kernel category, graph-chained (no per-launch event overhead).
        Leaves the hidden-state buffers dirty: `start()` again before decoding."""
        us = C.c_float()
        n = C.c_int32()
        if kind == "sample":                     # the sampler advances the positions on every replay (3 warm-up replays inside)
            self._steps_enqueued += int(n_replays) + 3
            self._grow_pages(self._steps_enqueued)
        _lib.check(self.lib.ssrhip_lm_time_category(self._ctx, ("gemv", "attn", "sample").index(kind), int(n_replays),
                                                    _lib.stream_ptr(), C.byref(us), C.byref(n)), "ssrhip_lm_time_category")
        return float(us.value), int(n.value)


# DecodeEngine's read-only views of its plan: `stream_<name>` / `<pair form>` = is that entry the plan's; the rest are the plan's fields.
for _st in STREAMS:
    setattr(DecodeEngine, "stream_" + _st.name, property(lambda self, _st=_st: self.plan.stream is _st))
for _pf in PAIR_FORMS:
    setattr(DecodeEngine, _pf.name, property(lambda self, _pf=_pf: self.plan.pair is _pf))
for _name, _field in (("_stream", "stream"), ("pair_mode", "pair_mode"), ("kv_dtype", "kv_dtype"), ("kv16_small", "kv16_small"),
                      ("share_prompt", "share_prompt"), ("want_logprobs", "logprobs")):
    setattr(DecodeEngine, _name, property(lambda self, _field=_field: getattr(self.plan, _field)))

# DecodeEngine's `<name>_launches_per_step` properties: what `ssrhip_lm_<name>_launches` counted in the last enqueued decode step (0 for an
# engine that has not stepped yet).
COUNTERS = (
    ("kv16", "Attention launches that read the bf16 KV cache (the layer count for a kv_dtype=\"bf16\" engine, 0 otherwise)."),
    ("group", "Attention launches that ran the grouped walk (the layer count for a share_prompt engine, else 0)."),
    ("w16", "GEMV launches that ran a bf16-stream kernel (4 * layers + 2 when every family qualifies; 0 for an engine that streams fp32 weights)."),
    ("w16_pair", "Pair launches that streamed packed bf16 weights (2 * layers when every family has a packed copy; `w16_launches_per_step` then "
                 "counts the two single launches left). 0 for an engine that does not pair its bf16 stream."),
    ("w8", "GEMV launches that ran an e4m3-stream kernel (4 * layers + 2 when every family qualifies; 0 for an engine that streams other weights)."),
    ("w8_pair", "Pair launches that streamed e4m3 codes (2 * layers when every family has codes; `w8_launches_per_step` then counts the two "
                "single launches left). 0 for an engine that does not pair its e4m3 stream."),
    ("pair4", "Pair launches that ran a 4-row pair kernel (2 * layers when both forms apply). 0 for an engine that does not run them."),
    ("pair4_pk", "Pair launches that ran a 4-row pair kernel over packed weights (2 * layers when every family has a packed copy; the stream's "
                 "own counter then counts the two single launches left). 0 for an engine that does not run them."),
    ("wt8", "GEMV launches that ran a kernel of the 5..16-row e4m3 weight stream (4 * layers + 2 when every family qualifies)."),
    ("wt16", "The same for the kernels of the 5..16-row bf16 weight stream."),
    ("wt32", "The same for the kernels of the 17..32-row bf16 weight stream."),
)
for _name, _doc in COUNTERS:
    setattr(DecodeEngine, _name + "_launches_per_step", property(lambda self, _name=_name: self._launches_per_step(_name), doc=_doc))
