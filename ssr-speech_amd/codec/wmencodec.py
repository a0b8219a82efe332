"""`WMEncodecModel` — drop-in for the reference's watermarked Encodec on the inference path
(`audiocraft/audiocraft/models/wmencodec.py:324-386`: `encode`, `decode`, `wmdecode`, `detect_watermark`,
`decode_latent`), built from a state-dict with the reference's key names. All arithmetic runs in libssrhip.so:
the SEANet convolutions / transposed convolutions / residual blocks as fp32 MFMA GEMMs over time-major
strided views (weight-norm folded and weights repacked once at load), the LSTM recurrence, RVQ search and
dequantisation, the watermark-label conditioning as dedicated HIP kernels. PyTorch only allocates buffers.

Layout: an activation is `[B][padL + T + padR][C]` fp32 (time-major, channels contiguous, halo rows zero or
reflected) so that the im2col matrix of a Conv1d is a *view* (row t = k consecutive time rows).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..weights import CodecConfig


def _extra_padding(length: int, k: int, s: int, pt: int) -> int:
    """audiocraft/modules/conv.py:47-53."""
    n_frames = (length - k + pt) / s + 1
    return (math.ceil(n_frames) - 1) * s + (k - pt) - length


def _empty(*shape, dtype, device):
    """torch.empty for the activation / state workspaces. SSRHIP_POISON_ALLOC=1 (debug; tools/poison_check.py, read at every call) fills them
    with NaN (float) / 0x7FC0 = bf16 NaN (int16) / a huge index (int32) instead: a kernel that READS a location no producer wrote turns its
    outputs NaN, where with plain torch.empty the result silently depends on what the allocator's block held before."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    if os.environ.get("SSRHIP_POISON_ALLOC", "0") not in ("", "0"):
        if dtype == torch.float32:
            t.fill_(float("nan"))
        elif dtype == torch.int16:
            t.fill_(0x7FC0)
        else:
            t.fill_(0x3FFFFFFF)
    return t


class _NoLaunch:
    """Stands in for the library during a sizing pass (`WMEncodecModel._sized`): every entry point "succeeds" without launching anything."""

    def __getattr__(self, name):
        if not name.startswith("ssrhip_"):
            raise AttributeError(name)
        return lambda *args: 0


def _tensors_of(obj):
    """the tensors inside a (nested) tuple / list result"""
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, (tuple, list)):
        return [t for o in obj for t in _tensors_of(o)]
    return []


def _device_mallocs(device) -> int:
    """How many times the caching allocator has gone to the driver for memory on this device (hipMalloc calls)."""
    return int(torch.cuda.memory_stats(device).get("num_device_alloc", 0))


class TM:
    """Time-major activation buffer with halo rows."""

    def __init__(self, B: int, T: int, Cc: int, padL: int, padR: int, device, lens: "Optional[Ragged]" = None, data=None, keep_halo=False):
        """`data`: caller-owned memory [B][padL + T + padR][C] to use instead of a fresh allocation (`DecodeStream`); `keep_halo`: its halo
        rows already hold what the consumer must read."""
        self.B, self.T, self.C, self.padL, self.padR = B, T, Cc, padL, padR
        self.lens = lens                   # ragged batch: per-item valid rows (None = every item has T rows)
        self.elu = False                   # True: the producer stored ELU(y) (its only consumers read it through ELU: they skip theirs)
        self.rows = padL + T + padR
        # every producer writes the whole interior; only the halo rows need a defined value before the consumer reads them
        # (zero for constant / structural padding; reflect padding overwrites them). A torch.zeros of the whole buffer was 24
        # full-size memsets per encode+decode (6.7 ms at 32 clips x 30 s).
        self.data = _empty(B, self.rows, Cc, dtype=torch.float32, device=device) if data is None else data
        assert tuple(self.data.shape) == (B, self.rows, Cc), (tuple(self.data.shape), B, self.rows, Cc)
        if keep_halo:
            return
        if padL:
            self.data[:, :padL].zero_()
        if padR:
            self.data[:, padL + T:].zero_()

    @property
    def base(self) -> int:
        return self.data.data_ptr()

    @property
    def interior(self) -> int:
        return self.data.data_ptr() + 4 * self.padL * self.C

    @property
    def bstride(self) -> int:
        return self.rows * self.C

    def interior_view(self) -> torch.Tensor:
        return self.data[:, self.padL: self.padL + self.T]


class Ragged:
    """Per-item lengths of a ragged batch at one time resolution: host list + the same numbers as a device int32 array (what
    `ssrhip_pad_ragged` reads). `scaled` derives the lengths after an up-/down-sampling layer; the device arrays are cached
    per resolution so that a decode creates four small tensors, not one per layer."""

    def __init__(self, lens: Sequence[int], device, _cache=None):
        self.host = [int(v) for v in lens]
        self.dev = torch.tensor(self.host, dtype=torch.int32, device=device)
        self._cache = _cache if _cache is not None else {}
        self._cache[tuple(self.host)] = self

    def scaled(self, num: int, den: int = 1) -> "Ragged":
        if any((v * num) % den for v in self.host):
            raise ValueError(f"ragged lengths {self.host} are not whole frames at a stride of {den}")
        new = tuple(v * num // den for v in self.host)
        hit = self._cache.get(new)
        return hit if hit is not None else Ragged(new, self.dev.device, self._cache)


def _fold_wn(sd, pfx: str, which: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """weight = g * v / ||v|| (old-style weight_norm, dim 0; conv.py:21-30) or a plain weight."""
    k = f"{pfx}{which}.{which}."
    if k + "weight" in sd:
        return sd[k + "weight"], sd[k + "bias"]
    return torch._weight_norm(sd[k + "weight_v"], sd[k + "weight_g"], 0), sd[k + "bias"]


CODEC_WEIGHT_DTYPES = ("fp32", "bf16")
CODEC_ACT_DTYPES = ("fp32", "bf16")


def _round_w(w: torch.Tensor, wdt: str) -> torch.Tensor:
    """A folded weight matrix as the model keeps it: with "bf16" every value rounded once (nearest even) to a bf16 value, kept in fp32."""
    return w.to(torch.bfloat16).to(torch.float32) if wdt == "bf16" else w


class _Conv:
    def __init__(self, sd, pfx, stride, act_in, dev, wdt="fp32"):
        w, b = _fold_wn(sd, pfx, "conv")
        w = _round_w(w, wdt)                         # behind the weight-norm fold, in front of everything derived from the matrix
        self.Cout, self.Cin, self.k = w.shape
        self.s = stride
        self.act_in = act_in
        self.W = w.permute(0, 2, 1).contiguous().view(self.Cout, self.k * self.Cin).to(dev)     # [Cout][k][Cin]
        self.Wraw = w.contiguous().view(self.Cout, self.Cin * self.k).to(dev)                   # Cin == 1 path
        self.b = b.contiguous().to(dev)
        pt = self.k - self.s
        self.pr = pt // 2
        self.pl = pt - self.pr

    def pads(self, T):
        return self.pl, self.pr + _extra_padding(T, self.k, self.s, self.k - self.s)

    def out_len(self, T):
        pl, pr = self.pads(T)
        return (T + pl + pr - self.k) // self.s + 1


class _ConvTr:
    def __init__(self, sd, pfx, stride, dev, wdt="fp32"):
        w, b = _fold_wn(sd, pfx, "convtr")          # [Cin][Cout][k]
        w = _round_w(w, wdt)
        self.Cin, self.Cout, self.k = w.shape
        self.s = stride
        assert self.k == 2 * stride, "SEANet uses kernel = 2*stride for its transposed convolutions"
        s = stride
        # W_all[(p, co)][0:Cin] multiplies in[q-1] (tap p+s), [Cin:2Cin] multiplies in[q] (tap p)
        wa = torch.empty(s, self.Cout, 2 * self.Cin, dtype=torch.float32)
        for p in range(s):
            wa[p, :, : self.Cin] = w[:, :, p + s].t()
            wa[p, :, self.Cin:] = w[:, :, p].t()
        self.W = wa.view(s * self.Cout, 2 * self.Cin).contiguous().to(dev)
        self.b = b.repeat(s).contiguous().to(dev)
        pt = self.k - self.s
        self.trim_r = pt // 2
        self.trim_l = pt - self.trim_r


def pack_lstm_whh_planes(planes: torch.Tensor) -> torch.Tensor:
    """bf16 planes [3][4C][C] of a recurrent matrix (`ssrhip_split_weights` of `weight_hh`, torch's gate order i f g o) -> the fragment
    order `csrc/lstm_split.hip` streams them in (include/ssrhip.h ssrhip_lstm_args.w_split):
        out[ub][w][s][mb][q][lh][li][e] = planes[q][g C + 16 ub + u][w C/4 + 16 s + 8 lh + e]      with 32 mb + li = 16 g + u,
    ub = unit block (C/16), w = wave = K quarter, s = k-step of 16 inside the quarter (C/64 of them), lane = 32 lh + li. Needs C % 64 == 0."""
    q3, rows, Cc = planes.shape
    assert q3 == 3 and rows == 4 * Cc and Cc % 64 == 0, planes.shape
    ks = Cc // 64
    x = planes.reshape(3, 4, Cc // 16, 16, 4, ks, 2, 8)           # q, g, ub, u, w, s, lh, e
    x = x.permute(2, 4, 5, 1, 3, 0, 6, 7)                         # ub, w, s, g, u, q, lh, e
    x = x.reshape(Cc // 16, 4, ks, 2, 32, 3, 2, 8)                # (g, u) -> m = 16 g + u = 32 mb + li
    return x.permute(0, 1, 2, 3, 5, 6, 4, 7).contiguous()         # ub, w, s, mb, q, lh, li, e


def pack_lstm_whh_plane(W: torch.Tensor) -> torch.Tensor:
    """A recurrent matrix of bf16 values, [4C][C] bfloat16 -> the ONE plane `csrc/lstm_w1.hip` streams (`ssrhip_lstm_layer_w1`):
        out[ub][w][s][mb][lh][li][e] = W[g C + 16 ub + u][w C/4 + 16 s + 8 lh + e]      with 32 mb + li = 16 g + u,
    the slice q = 0 of `pack_lstm_whh_planes` of the matrix's exact split, whose planes 1 and 2 are zeros. Needs C % 64 == 0."""
    rows, Cc = W.shape
    assert W.dtype == torch.bfloat16 and rows == 4 * Cc and Cc % 64 == 0, (W.dtype, W.shape)
    ks = Cc // 64
    x = W.reshape(4, Cc // 16, 16, 4, ks, 2, 8)                   # g, ub, u, w, s, lh, e
    x = x.permute(1, 3, 4, 0, 2, 5, 6)                            # ub, w, s, g, u, lh, e
    x = x.reshape(Cc // 16, 4, ks, 2, 32, 2, 8)                   # (g, u) -> m = 16 g + u = 32 mb + li
    return x.permute(0, 1, 2, 3, 5, 4, 6).contiguous()            # ub, w, s, mb, lh, li, e


class _Lstm:
    def __init__(self, sd, pfx, layers, dev, wdt="fp32"):
        self.layers = []
        for l in range(layers):
            wih, whh = _round_w(sd[pfx + f"lstm.weight_ih_l{l}"], wdt), _round_w(sd[pfx + f"lstm.weight_hh_l{l}"], wdt)
            bias = sd[pfx + f"lstm.bias_ih_l{l}"] + sd[pfx + f"lstm.bias_hh_l{l}"]
            self.layers.append((wih.contiguous().to(dev), whh.contiguous().to(dev), bias.contiguous().to(dev)))
        self.C = self.layers[0][1].shape[1]
        # the recurrent matrix once more, in the order the matrix-core step kernel's lanes read it (include/ssrhip.h w_packed)
        Cc = self.C
        self.packed = []
        for _, whh, _ in self.layers:
            if Cc % 16 == 0:
                self.packed.append(whh.view(4, Cc // 4, 4, Cc // 16, 4, 4).permute(1, 3, 4, 2, 0, 5).contiguous())
            else:
                self.packed.append(None)
        self.split = [None] * layers     # W_hh planes in MFMA fragment order (csrc/lstm_split.hip), made by CodecModel._prepare_planes when enabled


class _SeaNet:
    """One nn.Sequential of the reference (SEANetEncoder.model / SEANetDecoder.model), as a list of fused nodes."""

    def __init__(self, sd, pfx: str, cfg: CodecConfig, decoder: bool, dev, wdt: str = "fp32"):
        self.cfg, self.dev = cfg, dev
        # (model index of the node's first module, kind, obj, model index of the module whose OUTPUT the node produces)
        self.nodes: List[tuple] = []
        i = 0
        if not decoder:                  # seanet.py:113-150
            self.nodes.append((i, "conv", _Conv(sd, f"{pfx}model.{i}.", 1, 0, dev, wdt), i))
            i += 1
            for r in reversed(cfg.ratios):
                self.nodes.append((i, "res", (_Conv(sd, f"{pfx}model.{i}.block.1.", 1, 1, dev, wdt), _Conv(sd, f"{pfx}model.{i}.block.3.", 1, 1, dev, wdt)), i))
                self.nodes.append((i + 1, "conv", _Conv(sd, f"{pfx}model.{i + 2}.", r, 1, dev, wdt), i + 2))      # ELU (i+1) folded in
                i += 3
            if cfg.lstm:
                self.nodes.append((i, "lstm", _Lstm(sd, f"{pfx}model.{i}.", cfg.lstm, dev, wdt), i))
                i += 1
            self.nodes.append((i, "conv", _Conv(sd, f"{pfx}model.{i + 1}.", 1, 1, dev, wdt), i + 1))
        else:                            # seanet.py:209-254
            self.nodes.append((i, "conv", _Conv(sd, f"{pfx}model.{i}.", 1, 0, dev, wdt), i))
            i += 1
            if cfg.lstm:
                self.nodes.append((i, "lstm", _Lstm(sd, f"{pfx}model.{i}.", cfg.lstm, dev, wdt), i))
                i += 1
            for r in cfg.ratios:
                self.nodes.append((i, "convtr", _ConvTr(sd, f"{pfx}model.{i + 1}.", r, dev, wdt), i + 1))      # ELU (i) folded in
                self.nodes.append((i + 2, "res", (_Conv(sd, f"{pfx}model.{i + 2}.block.1.", 1, 1, dev, wdt), _Conv(sd, f"{pfx}model.{i + 2}.block.3.", 1, 1, dev, wdt)), i + 2))
                i += 3
            self.nodes.append((i, "conv", _Conv(sd, f"{pfx}model.{i + 1}.", 1, 1, dev, wdt), i + 1))

    def slice_nodes(self, lo: int, hi: Optional[int]):
        return [n for n in self.nodes if n[0] >= lo and (hi is None or n[0] < hi)]


# ----------------------------------------------------------------------------- streamed decode: the window plan (host arithmetic only)
def _conv_pads(k: int, s: int) -> Tuple[int, int]:
    """(left, right) padding of a non-causal StreamableConv1d (conv.py:185-201), without the length-dependent extra padding (0 at stride 1)"""
    pt = k - s
    return pt - pt // 2, pt // 2


def stream_lookahead(cfg: CodecConfig) -> int:
    """Frames of look-ahead the decoder's first convolution needs before its output at a frame is final."""
    return _conv_pads(cfg.kernel_size, 1)[1]


def stream_margins(cfg: CodecConfig) -> Tuple[int, int]:
    """(left, right) margin, in frames, a window of the decoder's part BEHIND the LSTM (transposed convolutions, residual blocks, last
    convolution) needs so that every sample of its core is computed from true neighbours only: the chain's receptive field, walked from
    the output back to the frames. (L, R) = samples of context the outputs of a layer need on either side; a stride-1 convolution adds
    its paddings; a transposed convolution (kernel 2s, `trim_l` raw samples cut in front) maps output o to the inputs
    floor((o + trim_l) / s) - 1 and floor((o + trim_l) / s), so a core that starts / ends on a frame boundary needs
    1 + ceil((L - trim_l) / s) inputs in front and 1 + floor((R + trim_l - 1) / s) behind."""
    L, R = _conv_pads(cfg.last_kernel_size, 1)
    for s in reversed(cfg.ratios):
        for _ in range(cfg.n_residual_layers):
            for k in (1, cfg.residual_kernel_size):                  # the block's 1x1 and its k-tap convolution (seanet.py:16-60)
                pl, pr = _conv_pads(k, 1)
                L, R = L + pl, R + pr
        pt = 2 * s - s
        trim_l = pt - pt // 2
        L, R = 1 + -((trim_l - L) // s), 1 + (R + trim_l - 1) // s
    return max(L, 0), max(R, 0)


def stream_window(c0: int, c1: int, n: int, margins: Tuple[int, int]) -> Tuple[int, int]:
    """The frames [lo, hi) a window with the core [c0, c1) reads when frames [0, n) exist: the core plus the margins, cut at the ends —
    an end at 0, or at n once n is the utterance's length, is a true edge that gets the layers' own padding and no margin."""
    assert 0 <= c0 < c1 <= n, (c0, c1, n)
    return max(0, c0 - margins[0]), min(n, c1 + margins[1])


def skip_stream_margins(cfg: CodecConfig) -> Tuple[int, int]:
    """(left, right) margin, in frames, a window of the watermark decoder's skip-encoder CHAIN — its first convolution, then per ratio a
    residual block and a strided convolution, up to and including the last strided one (seanet.py:113-150) — needs so that its three
    high-rate taps and its frame-rate rows are computed from true samples only: the receptive field walked from the frame-rate rows back
    to the samples, as `stream_margins` walks the decoder's. (L, R) = rows of context a layer's outputs need on either side; a strided
    convolution (kernel 2s, paddings (pl, pr)) maps output o to the inputs [o s - pl, o s + s + pr), so its input needs L s + pl rows in
    front and R s + pr behind; a stride-1 convolution adds its paddings. A tap's own field lies inside that of the rows behind it."""
    L = R = 0
    for s in cfg.ratios:                                             # the encoder applies reversed(ratios): walked backwards
        pl, pr = _conv_pads(2 * s, s)
        L, R = L * s + pl, R * s + pr
        for _ in range(cfg.n_residual_layers):
            for k in (1, cfg.residual_kernel_size):
                pl, pr = _conv_pads(k, 1)
                L, R = L + pl, R + pr
    pl, pr = _conv_pads(cfg.kernel_size, 1)
    hop = int(math.prod(cfg.ratios))
    return -(-(L + pl) // hop), -(-(R + pr) // hop)


def wm_stream_holdback(cfg: CodecConfig) -> int:
    """Frames that must exist behind a frame before its watermarked samples are final (`WMDecodeStream`): the skip-encoder chain's right
    margin, the look-ahead of the skip encoder's last convolution (behind its LSTM), the look-ahead of the decoder's first convolution,
    and the right margin of the layers behind the decoder's LSTM. The two forward-only LSTMs add nothing."""
    return skip_stream_margins(cfg)[1] + _conv_pads(cfg.last_kernel_size, 1)[1] + stream_lookahead(cfg) + stream_margins(cfg)[1]


# the three truth rules of the switches below (kept apart: "" counts as on for the first, as off for the second)
_not0 = lambda v: v != "0"                                             # noqa: E731
_on = lambda v: v not in ("", "0")                                     # noqa: E731
_ints = lambda v: tuple(int(c) for c in v.split(",") if c)             # noqa: E731

# WMEncodecModel's environment switches, read once in __init__: (attribute, switch, value when unset, parser). Tests and bench.py assign the
# attributes directly. INTEGRATION.md §4 lists the switches; the measurements behind the defaults are in DESIGN.md (Part II, codec).
_ENV_KNOBS = (
    ("lstm_packed", "SSRHIP_LSTM_PACKED", "1", _not0),             # the recurrent matrix in the matrix-core step kernel's lane order
    ("lstm_split", "SSRHIP_LSTM_SPLIT", "1", _on),                 # the recurrence on the bf16 matrix cores with split operands (csrc/lstm_split.hip)
    ("lstm_split_min_b", "SSRHIP_LSTM_SPLIT_MIN_B", "128", int),   # ... from this many items on; below it, and with 0 above, the fp32 pipe
    ("split_gemm", "SSRHIP_GEMM_SPLIT", "1", _not0),               # fp32 GEMMs as exactly split bf16 operands (csrc/gemm_split.hip); 0: the fp32 FMA chain
    ("elu_on_store", "SSRHIP_ELU_ON_STORE", "1", _not0),           # ELU on store wherever a tensor is only read through ELU; 0: every consumer applies it
    ("lanes", "SSRHIP_CODEC_LANES", "1", int),                     # batch lanes, a memory knob (`_in_lanes`) ...
    ("lane_min_items", "SSRHIP_CODEC_LANE_MIN", "8", int),         # ... of at least this many items each
    # the two-stream LSTM pipeline (`_lstm`) only from this many items on: a single-utterance call keeps to ONE hardware queue (DESIGN.md Part I.4)
    ("lstm_pipe_min_b", "SSRHIP_LSTM_PIPE_MIN_B", "8", int),
    ("presize", "SSRHIP_CODEC_PRESIZE", "1", _on),                 # the sizing passes of `_sized`; 0 is the A/B arm of tools/race_trials.py
    # channel counts whose residual block runs as one kernel: 64 and 128 pay, 256 / 512 lose to two GEMM launches
    ("fuse_channels", "SSRHIP_RESBLOCK_FUSE", "64,128", _ints),
    # a weight_dtype="bf16" model: ONE bf16 plane per matrix and the one-plane kernels (three products per k block); 0: three planes of the
    # rounded weights through the six-product kernels — the same bits (DESIGN.md Part I.30). Ignored for weight_dtype="fp32"
    ("codec_w1", "SSRHIP_CODEC_W1", "1", _not0),
    # ... and its LSTM recurrence: ONE plane of W_hh in fragment order through `ssrhip_lstm_layer_w1` (csrc/lstm_w1.hip: three products per
    # k-step, a third of the W_hh bytes); 0: three planes of the rounded W_hh through the six-product step — the same bits (DESIGN.md
    # Part I.31: 9.6 against 11.8 us per step at 256 items, 7 % of a 256 x 30 s pass). Ignored unless the model is `one_plane` and
    # `lstm_split` is on
    ("lstm_w1", "SSRHIP_LSTM_W1", "1", _not0),
)


def _codec_w1_env() -> bool:
    """The `codec_w1` switch as the environment has it now (what `WMEncodecModel.__init__` will read)."""
    _, switch, unset, parse = next(k for k in _ENV_KNOBS if k[0] == "codec_w1")
    return bool(parse(os.environ.get(switch, unset)))


class WMEncodecModel:
    def __init__(self, cfg: CodecConfig, state_dict: dict, device, *, weight_dtype: str = "fp32", act_dtype: str = "fp32"):
        """`weight_dtype="bf16"`: every convolution, transposed-convolution and LSTM weight matrix is rounded once to a bf16 value (kept in
        fp32) behind the weight-norm fold; biases, codebooks and the label table stay fp32. The model is then the fp32 codec on the rounded
        weights whatever kernel a shape takes, and its GEMMs and residual blocks run one weight plane (DESIGN.md Part I.30).

        `act_dtype="bf16"` (with `weight_dtype="bf16"` and `codec_w1` on only): every matrix product that takes a one-plane entry rounds its
        activation operand to bf16 (nearest even) where it is split in three today and keeps one product per k block; accumulation,
        epilogues and the activations in memory stay fp32 (DESIGN.md Part I.32). Which layers round is a property of the layer, not of
        the batch, window or stream an item is computed in."""
        if weight_dtype not in CODEC_WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype {weight_dtype!r} not in {CODEC_WEIGHT_DTYPES}")
        if act_dtype not in CODEC_ACT_DTYPES:
            raise ValueError(f"act_dtype {act_dtype!r} not in {CODEC_ACT_DTYPES}")
        if act_dtype == "bf16" and weight_dtype != "bf16":
            raise ValueError("act_dtype='bf16' needs weight_dtype='bf16' (bf16 activations against fp32 weights have no kernel)")
        if act_dtype == "bf16" and not _codec_w1_env():
            raise ValueError("act_dtype='bf16' needs the one-plane kernels: SSRHIP_CODEC_W1=0 switches them off")
        self.weight_dtype = weight_dtype
        self.act_dtype = act_dtype
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ssr_speech_amd codec needs a ROCm GPU device; there is no CPU path in this package")
        self.lib = _lib.lib()
        self.fuse_resblock = True            # tests switch it off to compare with the two-GEMM path
        self.force_few_out = False           # tests: take the few-output-channel kernel also for short inputs
        self._stream_few_out = False         # `_stream_pass`: a stream's window whose whole utterance takes that kernel is running
        self._tm_pool = None                 # `_stream_pass`: where `_alloc_for` takes its buffers from while a stream's window runs
        for attr, switch, unset, parse in _ENV_KNOBS:
            setattr(self, attr, parse(os.environ.get(switch, unset)))
        self._plane_cache = {}
        self._side_streams, self._keep = {}, {}
        self._envelopes = {}                 # (entry point, stream) -> [(items, samples-or-frames)] already sized
        self._small_reserved = set()
        self.passes_repeated = 0             # passes run again because the driver was asked for memory while they were in flight
        self.mallocs_in_flight = 0           # hipMallocs that happened during a call although it had been sized (tests assert 0)
        self.sizing_passes = 0
        self.n_launches = 0                  # library entry points called so far, dry passes included (tools/stream_latency.py)
        sd = {k: v.detach().to(torch.float32).cpu() for k, v in state_dict.items()}
        dev = self.device
        wdt = weight_dtype
        self.encoder = _SeaNet(sd, "encoder.", cfg, False, dev, wdt)
        self.decoder = _SeaNet(sd, "decoder.", cfg, True, dev, wdt)
        self.has_wm = "wmdecoder.wm_embed.weight" in sd
        if self.has_wm:
            self.wmdecoder = _SeaNet(sd, "wmdecoder.", cfg, True, dev, wdt)
            self.skip_encoder = _SeaNet(sd, "wmdecoder.skip_encoder.", cfg, False, dev, wdt)
            self.wm_encoder = _SeaNet(sd, "wmdecoder.wm_encoder.", cfg, False, dev, wdt)
            self.wm_proj = [_Conv(sd, f"wmdecoder.wm_proj{j}.1.", 1, 1, dev, wdt) for j in range(4)]
            self.wm_predictor = _Conv(sd, "wmdecoder.wm_predictor.1.", 1, 1, dev, wdt)
            w = sd["wmdecoder.wm_embed.weight"]                       # nn.Embedding(2, D/16, max_norm=True) (seanet.py:503)
            norm = w.norm(p=2, dim=1, keepdim=True)
            self.wm_table = torch.where(norm > 1.0, w * (1.0 / (norm + 1e-7)), w).contiguous().to(dev)
            # label conditioning folded: per projection (W_a [Cout][C_skip], class bias [n_labels][Cout] = W_b . ELU(embed(label)))
            self.wm_cls = []
            E = self.wm_table.shape[1]
            emb_act = torch.nn.functional.elu(self.wm_table.cpu().double())
            for c in self.wm_proj:
                assert c.k == 1, "wm_proj is a 1x1 convolution (seanet.py:513-539)"
                Wfull = c.W.cpu()                                                  # [Cout][C_skip + E]
                Cs = Wfull.shape[1] - E
                self.wm_cls.append((Wfull[:, :Cs].contiguous().to(dev), (emb_act @ Wfull[:, Cs:].double().t()).float().contiguous().to(dev)))
        self.codebooks = torch.stack([sd[f"quantizer.vq.layers.{q}._codebook.embed"] for q in range(cfg.n_q)]).contiguous().to(dev)
        self.e2 = self.codebooks.pow(2).sum(-1).contiguous()          # |e|^2 (core_vq.py:169)
        self.sample_rate, self.channels, self.frame_rate = cfg.sample_rate, cfg.channels, cfg.frame_rate
        self._prepare_planes()

    def _prepare_planes(self):
        """Split every GEMM weight once, now, on the current stream (the batch lanes run on their own streams later: nothing may be
        created lazily there), and wait for it."""
        nets = [self.encoder, self.decoder] + ([self.wmdecoder, self.skip_encoder, self.wm_encoder] if self.has_wm else [])
        for net in nets:
            for _, kind, obj, _ in net.nodes:
                if kind == "conv":
                    self._planes(obj.W)
                elif kind == "convtr":
                    self._planes(obj.W)
                elif kind == "res":
                    self._planes(obj[0].W)
                    self._planes(obj[1].W)
                    if obj[0].Cin in self.fuse_channels:
                        self._resblock_planes(obj[0], obj[1])
                elif kind == "lstm":
                    for l, (wih, whh, _) in enumerate(obj.layers):
                        self._planes(wih)
                        if self.lstm_split and obj.C % 128 == 0 and obj.split[l] is None:
                            if self.lstm_one_plane:      # bfloat16: `_lstm_steps` tells the two packs apart by their dtype
                                # == pack_lstm_whh_plane(whh.to(bfloat16)): plane 0 of the three-plane pack (planes 1 and 2 of a rounded
                                # matrix are zeros). Cut out of the three-plane temporaries, which then go back to the caching allocator:
                                # construction requests what it requested before, and the pool it leaves to the passes is no smaller
                                # (a pass covered by an earlier envelope of `_sized` has no dry pass of its own and lives on that pool)
                                obj.split[l] = pack_lstm_whh_planes(self._split_planes(whh))[:, :, :, :, 0].contiguous().view(torch.bfloat16)
                            else:
                                obj.split[l] = pack_lstm_whh_planes(self._split_planes(whh))
        if self.has_wm:
            for Wa, _ in self.wm_cls:
                self._planes(Wa)
            self._planes(self.wm_predictor.W)
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ sizing passes
    def _sized(self, kind: str, B: int, T: int, run):
        """Run one dense codec pass `run()` so that the caching allocator never has to map device memory (hipMalloc) while the pass's
        kernels are in flight.

        Why: on this platform a kernel that runs while ANOTHER hardware queue of the process is busy and the host maps fresh device memory
        can come back with wrong values (DESIGN.md "the multi-stream failure" has the trials). A codec pass IS several queues — the two LSTM
        layers run on two streams — and a cold process maps memory for every layer. What the pass will allocate is a deterministic function
        of (entry point, items, length): the first time a shape is not covered by one already seen on this stream, the pass runs once DRY —
        the device idle (synchronised), every library launch a no-op, the same tensors allocated and freed in the same order — which leaves
        the allocator holding exactly the blocks the real pass then reuses. Later calls of that size or smaller find them there.
        `mallocs_in_flight` counts the driver allocations that still happened during real passes (a smaller shape can fall into another
        size class, the caller may hold more live tensors than the sizing pass saw): such a pass is REPEATED — its results are dropped,
        the device synchronised, and it runs again from the now sufficient pool (`passes_repeated`)."""
        if not self.presize:
            return run()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._keep.pop(stream, None)           # the previous call's LSTM state: its kernels are behind us on this stream
        env = self._envelopes.setdefault((kind, stream), [])
        if not any(b >= B and t >= T for b, t in env):
            torch.cuda.synchronize(self.device)                  # nothing in flight, on any stream, while memory is mapped
            real, self.lib = self.lib, _NoLaunch()
            try:
                dry_out = run()
                # room for ONE more generation of the results: a caller that still holds the previous call's outputs while this one runs
                # (`out = codec.decode(...)` in a loop) must not push the real pass to the driver either
                spare = [torch.empty_like(t) for t in _tensors_of(dry_out)]
                # ... and for a SMALLER shape later on: every large block can be split for a smaller request, but tensors that shrink below
                # the allocator's 1 MB class boundary move to its small pool (2 MB segments) — 32 MB of those per stream, once
                if stream not in self._small_reserved:
                    spare += [torch.empty((1 << 20) - 4096, dtype=torch.uint8, device=self.device) for _ in range(32)]
                    self._small_reserved.add(stream)
                del spare, dry_out
            finally:
                self.lib = real
                self._keep.pop(stream, None)
            torch.cuda.synchronize(self.device)                  # the dry pass's own fills and copies (torch kernels on garbage)
            self.sizing_passes += 1
            env[:] = [(b, t) for b, t in env if not (b <= B and t <= T)] + [(B, T)]
        for attempt in range(3):
            n0 = _device_mallocs(self.device)
            out = run()
            grown = _device_mallocs(self.device) - n0
            if not grown:
                return out
            # The driver was asked for memory while this pass was in flight after all (a live set the sizing pass did not see, a size-class
            # crossing, another thread's allocation): its results are SUSPECT on this platform — they are dropped and the pass runs again,
            # now from a pool that holds what it needs (the kernels are deterministic; inputs are untouched). Counted, so tests can assert 0.
            self.mallocs_in_flight += grown
            self.passes_repeated += 1
            del out
            torch.cuda.synchronize(self.device)
        return run()

    # ------------------------------------------------------------------ low-level launches
    @property
    def one_plane(self) -> bool:
        """One bf16 plane per matrix and the one-plane entries: a bf16-rounded model with `codec_w1` on."""
        return self.weight_dtype == "bf16" and bool(self.codec_w1)

    @property
    def bf16_acts(self) -> bool:
        """The one-plane entries with the activation operand rounded to bf16: a `one_plane` model built with `act_dtype="bf16"`."""
        return self.one_plane and self.act_dtype == "bf16"

    @property
    def lstm_one_plane(self) -> bool:
        """W_hh as one plane and the one-plane recurrence step: a `one_plane` model with `lstm_split` and `lstm_w1` on."""
        return self.one_plane and bool(self.lstm_split) and bool(self.lstm_w1)

    def _call_w1(self, name: str, a) -> bool:
        """A one-plane entry (`ssrhip_codec_gemm_w1`, `ssrhip_resblock_w1`, their `_a1` forms) on the current stream: False when it
        answered 1 — nothing was launched and the caller takes the fp32 path on the rounded masters, WITHOUT planes."""
        self.n_launches += 1
        rc = getattr(self.lib, name)(C.byref(a), _lib.stream_ptr())
        if rc == 1:
            return False
        _lib.check(rc, name)
        return True

    def _call(self, name: str, *args):
        """One library launch on the current stream. The entry point is looked up at call time: `_sized` swaps `self.lib` for its dry pass
        and tests wrap it."""
        self.n_launches += 1
        _lib.check(getattr(self.lib, name)(*args, _lib.stream_ptr()), name)

    def _planes(self, W: torch.Tensor) -> Optional[torch.Tensor]:
        """bf16 planes [3][N][K] of a weight matrix for the split GEMM (csrc/gemm_split.hip: the fp32 operand as the exact sum of three
        bf16 pieces), made once per matrix on the device; None when the split path is switched off or the shape can never take it.
        A `one_plane` model keeps ONE plane [N][K] — the rounded matrix as bfloat16 — which only the one-plane entries may be given: the
        plane count is part of the cache key."""
        if not self.split_gemm or W.dim() != 2 or W.shape[0] <= 64 or W.shape[1] % 8 != 0:
            return None
        n = 1 if self.one_plane else 3
        key = (W.data_ptr(), n)
        hit = self._plane_cache.get(key)
        if hit is None:
            hit = self._plane_cache[key] = self._split_planes(W, n)
        return hit

    def _split_planes(self, W: torch.Tensor, n: int = 3) -> torch.Tensor:
        """bf16 planes [3][N][K] of any fp32 matrix (uncached: for callers that repack them, e.g. pack_lstm_whh_planes); n = 1: the one
        plane [N][K] of a matrix of bf16 values"""
        if n == 1:
            assert self.weight_dtype == "bf16", "one plane holds a matrix of bf16 values only"
            return W.to(torch.bfloat16).contiguous()
        out = torch.empty(3, W.shape[0], W.shape[1], dtype=torch.int16, device=W.device)
        self._call("ssrhip_split_weights", W.data_ptr(), out.data_ptr(), W.numel())
        return out

    def _resblock_planes(self, c3, c1):
        """bf16 planes of a residual block's two matrices for csrc/resblock_split.hip (C in {64, 128}): W3 [C/2][3C] as it is, W1 [C][C/2]
        with its columns in the order the kernel's stage-1 accumulator hands the hidden channels on (include/ssrhip.h w1_split).
        Made once per block on the device; None when the split path is off."""
        if not self.split_gemm or c3.Cin not in (64, 128):
            return None
        n = 1 if self.one_plane else 3
        key = ("res", c3.W.data_ptr(), c1.W.data_ptr(), n)
        hit = self._plane_cache.get(key)
        if hit is None and n == 1:            # one plane each: the rounded matrices as bfloat16, W1 in the same column order
            Hh = c3.Cout
            kp = torch.arange(Hh, device=c1.W.device)
            j, g, i = kp // 16, (kp // 8) % 2, kp % 8
            perm = 16 * j + (i % 4) + 8 * (i // 4) + 4 * g
            hit = (c3.W.reshape(Hh, -1).to(torch.bfloat16).contiguous(), c1.W.reshape(c1.Cout, Hh)[:, perm].to(torch.bfloat16).contiguous())
            self._plane_cache[key] = hit
        if hit is None:
            Hh = c3.Cout
            kp = torch.arange(Hh, device=c1.W.device)
            j, g, i = kp // 16, (kp // 8) % 2, kp % 8
            perm = 16 * j + (i % 4) + 8 * (i // 4) + 4 * g
            w1p = c1.W.reshape(c1.Cout, Hh)[:, perm].contiguous()
            w3 = c3.W.reshape(Hh, -1).contiguous()
            p3 = torch.empty(3, w3.shape[0], w3.shape[1], dtype=torch.int16, device=w3.device)
            p1 = torch.empty(3, w1p.shape[0], w1p.shape[1], dtype=torch.int16, device=w3.device)
            self._call("ssrhip_split_weights", w3.data_ptr(), p3.data_ptr(), w3.numel())
            self._call("ssrhip_split_weights", w1p.data_ptr(), p1.data_ptr(), w1p.numel())
            torch.cuda.current_stream(w3.device).synchronize()       # w1p / w3 temporaries may be freed after this call
            hit = (p3, p1)
            self._plane_cache[key] = hit
        return hit

    def _gemm(self, A, W, bias, Cp, M, N, K, lda, ldc, act_in=0, R=0, ldr=0, batch=1, sA=0, sC=0, sR=0, tm=(0, 0, 0), rowcls=None, act_out=0):
        a = _lib.GemmArgs()
        a.act_out = act_out
        a.A, a.W, a.bias, a.C = A, W.data_ptr(), (bias.data_ptr() if bias is not None else 0), Cp
        planes = self._planes(W)
        a.W_split = planes.data_ptr() if planes is not None else 0
        a.M, a.N, a.K, a.lda, a.ldc = M, N, K, lda, ldc
        a.act_in, a.R, a.ldr, a.batch = act_in, R, ldr, batch
        a.strideA, a.strideC, a.strideR = sA, sC, sR
        a.tm_c, a.tm_lo, a.tm_hi = tm
        if rowcls is not None:           # (class bias [n_class][N], class ids int32 [batch][n], rows per id)
            # (the ids' item stride: shape[1] for a dense [batch][n]; a batched stream hands in a window of columns of a wider array)
            a.rbias, a.rclass, a.rrep = rowcls[0].data_ptr(), rowcls[1].data_ptr(), int(rowcls[2])
            a.rclass_stride = int(rowcls[1].stride(0)) if batch > 1 else int(rowcls[1].shape[1])
        if planes is not None and planes.dim() == 2:      # one plane: its own entry; on answer 1 the fp32 chain on the rounded master
            if self._call_w1("ssrhip_codec_gemm_a1" if self.bf16_acts else "ssrhip_codec_gemm_w1", a):
                return
            a.W_split = 0
        self._call("ssrhip_gemm", C.byref(a))

    def _fill_pads(self, buf: TM, structural_zero: bool = False):
        if self.cfg.pad_mode not in ("constant", "reflect"):
            raise ValueError(self.cfg.pad_mode)
        if buf.lens is not None:
            # ragged batch: every item gets ITS OWN halo right behind its last valid row (and in front, for reflect)
            if buf.padL + buf.padR > 0:
                refl = int(self.cfg.pad_mode == "reflect" and not structural_zero)
                self._call("ssrhip_pad_ragged", buf.base, buf.lens.dev.data_ptr(), buf.B, buf.T, buf.padL, buf.padR, buf.C, buf.bstride,
                           refl)
            return
        if self.cfg.pad_mode == "reflect" and not structural_zero and (buf.padL + buf.padR) > 0:
            self._call("ssrhip_pad_reflect", buf.base, buf.B, buf.T, buf.padL, buf.padR, buf.C, buf.bstride)
        elif self.cfg.pad_mode not in ("constant", "reflect"):
            raise ValueError(self.cfg.pad_mode)

    def _need(self, node, T) -> Tuple[int, int, bool]:
        """(padL, padR, structural) the node wants on its input of interior length T."""
        if node is None:
            return 0, 0, False
        kind, obj = node[1], node[2]
        if kind == "conv":
            pl, pr = obj.pads(T)
            return pl, pr, False
        if kind == "res":
            pl, pr = obj[0].pads(T)
            return pl, pr, False
        if kind == "convtr":
            return 1, 1, True
        return 0, 0, False

    def _alloc_for(self, B, T, Cc, nxt, lens: Optional[Ragged] = None) -> TM:
        pl, pr, _ = self._need(nxt, T)
        if self._tm_pool is not None:                # a `DecodeStream` window: its buffers exist since the stream was created
            return self._tm_pool.take(B, T, Cc, pl, pr, self.device)
        return TM(B, T, Cc, pl, pr, self.device, lens)

    @contextlib.contextmanager
    def _stream_pass(self, pool: "_WindowPool", few: bool):
        """While one stage-2 window of a stream runs (`_StreamCore._tail_pass`): `_alloc_for` hands out the stream's own buffers, from the
        pool's first on, and with `few` the last layer runs as the few-output kernel whatever the window's length."""
        pool.at = 0
        self._tm_pool, self._stream_few_out = pool, bool(few)
        try:
            yield
        finally:
            self._tm_pool, self._stream_few_out = None, False

    # ------------------------------------------------------------------ nodes
    def _act_in(self, wants_elu: bool, x: TM) -> int:
        """ELU-on-load flag of a consumer: needed unless the producer already stored ELU(x) (`x.elu`). A consumer that wants the RAW
        tensor must never be handed an ELU'd one."""
        if x.elu and not wants_elu:
            raise AssertionError("a layer that reads its input without ELU was given a tensor stored through ELU")
        return _lib.ACT_ELU if (wants_elu and not x.elu) else 0

    FEW_OUT_MIN_T = 4096     # output rows from which the 1-channel last layer runs as `ssrhip_conv_few_out`

    def _conv(self, c: _Conv, x: TM, nxt, R: Optional[TM] = None, post_elu: bool = False) -> TM:
        """`post_elu`: store ELU(result) (the caller knows that every consumer reads this output through ELU; `self.elu_on_store`)."""
        B = x.B
        T_out = (x.T + x.padL + x.padR - c.k) // c.s + 1
        out = self._alloc_for(B, T_out, c.Cout, nxt, x.lens.scaled(1, c.s) if x.lens is not None else None)
        act_in = self._act_in(bool(c.act_in), x)
        if c.Cin == 1:
            assert c.act_in == 0 and not post_elu
            self._call("ssrhip_conv_cin1", x.base, c.Wraw.data_ptr(), c.b.data_ptr(), out.interior, B, T_out, c.k, c.s, c.Cout,
                       x.bstride, out.bstride)
        elif c.Cout <= 4 and c.s == 1 and R is None and c.Cin % 8 == 0 and (T_out >= self.FEW_OUT_MIN_T or self.force_few_out or self._stream_few_out) and not post_elu:
            # the 1-channel output layer at the sample rate: a read-bound dot-product kernel instead of a GEMM tile with 1 useful column
            self._call("ssrhip_conv_few_out", x.base, c.W.data_ptr(), c.b.data_ptr(), out.interior, B, T_out, c.k, c.Cin, c.Cout,
                       act_in, x.bstride, out.bstride)
        else:
            self._gemm(x.base, c.W, c.b, out.interior, T_out, c.Cout, c.k * c.Cin, c.s * c.Cin, c.Cout, act_in=act_in,
                       R=(R.interior if R is not None else 0), ldr=(R.C if R is not None else 0), batch=B, sA=x.bstride, sC=out.bstride,
                       sR=(R.bstride if R is not None else 0), act_out=(_lib.ACT_ELU if post_elu else 0))
        out.elu = post_elu
        self._fill_pads(out, structural_zero=(nxt is not None and nxt[1] == "convtr"))
        return out

    def _convtr(self, c: _ConvTr, x: TM, nxt) -> TM:
        assert x.padL == 1 and x.padR == 1
        T_out = x.T * c.s
        out = self._alloc_for(x.B, T_out, c.Cout, nxt, x.lens.scaled(c.s) if x.lens is not None else None)
        Cp = out.interior - 4 * c.trim_l * c.Cout
        self._gemm(x.base, c.W, c.b, Cp, x.T + 1, c.s * c.Cout, 2 * c.Cin, c.Cin, c.s * c.Cout, act_in=self._act_in(True, x), batch=x.B,
                   sA=x.bstride, sC=out.bstride, tm=(c.Cout, c.trim_l, c.trim_l + T_out))
        self._fill_pads(out, structural_zero=(nxt is not None and nxt[1] == "convtr"))
        return out

    def _res(self, cs, x: TM, nxt, post_elu: bool = False) -> TM:
        c3, c1 = cs
        assert not x.elu, "a residual block adds its RAW input back (seanet.py:58-60)"
        if self.fuse_resblock and c3.Cin in self.fuse_channels and c3.Cout * 2 == c3.Cin and c3.k == 3 and c3.s == 1 and c1.k == 1 and c1.s == 1 \
                and x.padL == 1 and x.padR == 1:
            # the whole block as one kernel (csrc/resblock.hip): one read + one write of the activation, the C/2 intermediate stays on chip
            out = self._alloc_for(x.B, x.T, c1.Cout, nxt, x.lens)
            a = _lib.ResblockArgs()
            a.x, a.y = x.base, out.interior
            a.w3, a.b3, a.w1, a.b1 = c3.W.data_ptr(), c3.b.data_ptr(), c1.W.data_ptr(), c1.b.data_ptr()
            a.B, a.T, a.C = x.B, x.T, c3.Cin
            a.x_bstride, a.y_bstride = x.bstride, out.bstride
            a.out_act = _lib.ACT_ELU if post_elu else 0
            planes = self._resblock_planes(c3, c1)
            if planes is not None:
                a.w3_split, a.w1_split = planes[0].data_ptr(), planes[1].data_ptr()
            if planes is not None and planes[0].dtype == torch.bfloat16:      # one plane each: its own entry; on answer 1, no planes
                if not self._call_w1("ssrhip_resblock_a1" if self.bf16_acts else "ssrhip_resblock_w1", a):
                    a.w3_split = a.w1_split = 0
                    self._call("ssrhip_resblock", C.byref(a))
            else:
                self._call("ssrhip_resblock", C.byref(a))
            out.elu = post_elu
            self._fill_pads(out, structural_zero=(nxt is not None and nxt[1] == "convtr"))
            return out
        h = self._conv(c3, x, None, post_elu=self.elu_on_store)        # the intermediate feeds only `ELU -> 1x1 conv`
        return self._conv(c1, h, nxt, R=x, post_elu=post_elu)

    LSTM_CHUNK = 64          # time steps per pipeline stage of the two stacked LSTM layers

    def _lstm_use_split(self, L: _Lstm, B: int) -> bool:
        return bool(self.lstm_split and B >= self.lstm_split_min_b and not (B <= 4 and L.C in (256, 512, 1024, 2048)))

    def _lstm_in_gemm(self, L: _Lstm, l: int, src_ptr: int, src_bs: int, gin: torch.Tensor, B: int, T: int, t0: int, t1: int):
        """gin[:, t0:t1] = in[:, t0:t1] W_ih^T + b of layer l; `T` = rows per item of `gin`."""
        Cc = L.C
        wih, _, bias = L.layers[l]
        self._gemm(src_ptr + 4 * t0 * Cc, wih, bias, gin.data_ptr() + 4 * t0 * 4 * Cc, t1 - t0, 4 * Cc, Cc, Cc, 4 * Cc,
                   batch=B, sA=src_bs, sC=T * 4 * Cc)

    def _lstm_steps(self, L: _Lstm, l: int, gin, hbuf, cbuf, hsplit, out_ptr: int, out_bs: int, skip_ptr: int, skip_bs: int,
                    B: int, T: int, t0: int, t1: int, out_elu: bool):
        """The time steps [t0, t1) of layer l (`ssrhip_lstm_layer`; t0 > 0 continues from the state the call that ended at t0 left in
        `hbuf` / `cbuf`); `T` = rows per item of `gin` and of the output."""
        Cc = L.C
        a = _lib.LstmArgs()
        small_b = B <= 4 and Cc in (256, 512, 1024, 2048)            # ssrhip_lstm_layer's path choice
        use_packed = (not small_b) and L.packed[l] is not None and self.lstm_packed
        a.gin, a.w_hh, a.out = gin.data_ptr(), (L.packed[l] if use_packed else L.layers[l][1]).data_ptr(), out_ptr
        a.w_packed = int(use_packed)
        if hsplit is not None:
            a.w_split, a.hsplit = L.split[l].data_ptr(), hsplit.data_ptr()
        a.skip = skip_ptr                                             # y = lstm(x) + x (lstm.py:21-23) on the last layer
        a.hbuf, a.cbuf, a.gates = hbuf.data_ptr(), cbuf.data_ptr(), 0
        a.B, a.T, a.C = B, T, Cc
        a.gin_bstride, a.out_bstride, a.skip_bstride = T * 4 * Cc, out_bs, skip_bs
        a.t_begin, a.t_end = t0, t1
        a.out_act = _lib.ACT_ELU if out_elu else 0
        # the entry follows the BUFFER held (bfloat16 = the one-plane pack, int16 = three planes), never the knob: a one-plane buffer in the
        # three-plane entry would be read twice its size past its end
        if hsplit is not None and L.split[l].dtype == torch.bfloat16:
            if self._call_w1("ssrhip_lstm_layer_w1", a):
                return
            a.w_split = a.hsplit = 0          # answered 1: the fp32 pipe on the rounded W_hh, what a three-plane model runs at such a shape
        self._call("ssrhip_lstm_layer", C.byref(a))

    def _lstm(self, L: _Lstm, x: TM, nxt, post_elu: bool = False) -> TM:
        """2-layer LSTM + skip (lstm.py:10-25). Each layer: input GEMM over time (MFMA) + one launch per time step. With two
        layers the recurrences are software-pipelined over chunks of LSTM_CHUNK steps on two streams: layer 2 works on chunk
        i (its input GEMM for that chunk, then its steps) while layer 1 already runs chunk i+1 — the step kernels are
        latency-bound and leave most of the GPU idle, so the two chains overlap almost completely."""
        B, T, Cc = x.B, x.T, x.C
        dev = self.device
        assert x.padL == 0 and x.padR == 0 and not x.elu
        nl = len(L.layers)
        rows = (B + 15) // 16 * 16                                     # include/ssrhip.h ssrhip_lstm_args
        gins = [_empty(B, T, 4 * Cc, dtype=torch.float32, device=dev) for _ in range(nl)]
        hbufs = [_empty(2, rows, Cc, dtype=torch.float32, device=dev) for _ in range(nl)]
        cbufs = [_empty(B, Cc, dtype=torch.float32, device=dev) for _ in range(nl)]
        outs = [self._alloc_for(B, T, Cc, nxt, x.lens) if l == nl - 1 else TM(B, T, Cc, 0, 0, dev) for l in range(nl)]
        # h of the split-operand path: two buffers of bf16 planes in fragment order (zeroed by the library at t = 0)
        use_split = self._lstm_use_split(L, B)
        hsplits = [_empty(2 * ((B + 63) // 64) * 64 * Cc * 3, dtype=torch.int16, device=dev) if (use_split and L.split[l] is not None) else None
                   for l in range(nl)]

        def in_gemm(l, t0, t1):                                        # gin_l[:, t0:t1] = in_l[:, t0:t1] W_ih^T + b
            src_ptr, src_bs = (x.interior, x.bstride) if l == 0 else (outs[l - 1].interior, outs[l - 1].bstride)
            self._lstm_in_gemm(L, l, src_ptr, src_bs, gins[l], B, T, t0, t1)

        def steps(l, t0, t1):
            self._lstm_steps(L, l, gins[l], hbufs[l], cbufs[l], hsplits[l], outs[l].interior, outs[l].bstride,
                             (x.interior if l == nl - 1 else 0), x.bstride, B, T, t0, t1, post_elu and l == nl - 1)

        if nl == 2 and T > self.LSTM_CHUNK and B >= self.lstm_pipe_min_b:
            main = torch.cuda.current_stream(dev)
            side = self._side_stream()
            # Every tensor the side stream touches was allocated on `main`, and `main` joins the side stream (`fin`) before this function
            # returns — also when a launch fails half way (the `finally`): the stream order alone makes reuse of a freed block safe.
            # `record_stream(side)` would defer reuse until the GPU passes an event recorded at release time, which a sizing pass (`_sized`)
            # never waits for: the two would allocate differently. SSRHIP_RECORD_STREAM=1 brings the calls back.
            if os.environ.get("SSRHIP_RECORD_STREAM", "0") not in ("", "0"):
                for tns in gins + hbufs + cbufs + [o.data for o in outs] + [x.data] + [h for h in hsplits if h is not None]:
                    tns.record_stream(side)
            try:
                in_gemm(0, 0, T)
                for t0 in range(0, T, self.LSTM_CHUNK):
                    t1 = min(t0 + self.LSTM_CHUNK, T)
                    steps(0, t0, t1)
                    ev = torch.cuda.Event()
                    ev.record(main)
                    with torch.cuda.stream(side):
                        side.wait_event(ev)
                        in_gemm(1, t0, t1)
                        steps(1, t0, t1)
            finally:
                fin = torch.cuda.Event()
                fin.record(side)
                main.wait_event(fin)
        else:
            for l in range(nl):
                in_gemm(l, 0, T)
                steps(l, 0, T)
        out = outs[-1]
        out.elu = post_elu
        self._fill_pads(out, structural_zero=(nxt is not None and nxt[1] == "convtr"))
        self._keep[torch.cuda.current_stream(dev).cuda_stream] = (gins, hbufs, cbufs, outs, hsplits)
        return out

    def _side_stream(self):
        """The second stream of the LSTM layer pipeline: one per stream the codec is called on (every batch lane has its own)."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        if key not in self._side_streams:
            self._side_streams[key] = torch.cuda.Stream(self.device)
        return self._side_streams[key]

    def _lane_cuts(self, B: int):
        n = min(self.lanes, B // max(self.lane_min_items, 1))
        if n <= 1:
            return None
        edges = [B * i // n for i in range(n + 1)]
        return list(zip(edges[:-1], edges[1:]))

    def _in_lanes(self, B: int, body):
        """Run `body(lo, hi) -> tuple of tensors` for the batch lanes [lo, hi) ONE AFTER THE OTHER on the calling stream and return
        the list of per-lane results. Lanes are a memory knob: a lane's intermediates are freed before the next lane allocates its
        own, so the peak falls with the lane size. Lanes on streams of their own were slower and unsafe (DESIGN.md "Batch lanes")."""
        cuts = self._lane_cuts(B)
        if cuts is None:
            return [body(0, B)]
        return [body(lo, hi) for lo, hi in cuts]

    @staticmethod
    def _join(parts, i):
        vals = [p[i] for p in parts]
        if vals[0] is None:
            return None
        return vals[0] if len(vals) == 1 else torch.cat(vals, dim=0)

    def _run(self, nodes, x: TM, after=None) -> TM:
        """Run consecutive nodes; `after` = the node that will consume the result (decides its halo and whether the result is stored
        through ELU: a residual block's or the LSTM's output goes into `ELU -> conv / convtr` and nowhere else — the watermark
        decoder's skip taps are read through ELU as well, seanet.py:577-591 — so the producer applies the ELU once, on store)."""
        for idx, node in enumerate(nodes):
            nxt = nodes[idx + 1] if idx + 1 < len(nodes) else after
            kind, obj = node[1], node[2]
            post = self.elu_on_store and kind in ("res", "lstm") and nxt is not None and \
                ((nxt[1] == "conv" and bool(nxt[2].act_in)) or nxt[1] == "convtr")
            if kind == "conv":
                x = self._conv(obj, x, nxt)
            elif kind == "convtr":
                x = self._convtr(obj, x, nxt)
            elif kind == "res":
                x = self._res(obj, x, nxt, post_elu=post)
            elif kind == "lstm":
                x = self._lstm(obj, x, nxt, post_elu=post)
        return x

    def _input_tm(self, wav: torch.Tensor, first, lens: Optional[Ragged] = None) -> TM:
        """[B,1,T] -> time-major buffer with the first node's halo."""
        assert wav.dim() == 3 and wav.shape[1] == self.channels == 1, wav.shape
        B, _, T = wav.shape
        x = self._alloc_for(B, T, 1, first, lens)
        x.data[:, x.padL: x.padL + T, 0] = wav[:, 0].to(self.device, torch.float32)
        self._fill_pads(x)
        return x

    # ------------------------------------------------------------------ public API (wmencodec.py:324-386)
    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """-> (codes int64 [B,K,T'], scale=None (renormalize False), emb f32 [B,D,T'])."""
        assert x.dim() == 3

        def body(lo, hi):
            inp = self._input_tm(x[lo:hi], self.encoder.nodes[0])
            emb = self._run(self.encoder.nodes, inp)
            B, T, D = emb.B, emb.T, emb.C
            codes = _empty(B, self.cfg.n_q, T, dtype=torch.int32, device=self.device)
            self._call("ssrhip_rvq_encode", emb.interior, self.codebooks.data_ptr(), self.e2.data_ptr(), codes.data_ptr(), B, T, D,
                       self.cfg.n_q, self.cfg.bins, emb.bstride)
            return codes.to(torch.int64), emb.interior_view().transpose(1, 2).contiguous()

        parts = self._in_lanes(x.shape[0], lambda lo, hi: self._sized("encode", hi - lo, int(x.shape[-1]), lambda: body(lo, hi)))
        return self._join(parts, 0), None, self._join(parts, 1)

    def _codes32(self, codes: torch.Tensor) -> torch.Tensor:
        """Code ids on the device as int32, range-checked once for the whole batch (before it is cut into lanes)."""
        assert codes.dim() == 3
        c32 = codes.to(self.device, torch.int32).contiguous()
        if c32.numel() > 0:
            lo, hi = torch.aminmax(c32)                               # one kernel; the two scalars come back in one wait
            lo_hi = torch.stack([lo, hi]).tolist()
            if lo_hi[1] >= self.cfg.bins or lo_hi[0] < 0:
                raise IndexError("index out of range in self")        # what F.embedding raises in the reference (core_vq.py:175)
        return c32

    def _dequant(self, c32: torch.Tensor, nxt, lens: Optional[Ragged] = None) -> TM:
        B, K, T = c32.shape
        c32 = c32.contiguous()
        out = self._alloc_for(B, T, self.cfg.dimension, nxt, lens)
        self._call("ssrhip_rvq_decode", c32.data_ptr(), self.codebooks.data_ptr(), out.interior, B, T, self.cfg.dimension, K,
                   self.cfg.bins, out.bstride)
        self._fill_pads(out)
        return out

    @staticmethod
    def _channel_major(y: TM) -> torch.Tensor:
        """[B][T][C] time-major result -> the reference's [B, C, T]. A 1-channel waveform without halo rows is the same memory
        either way (a view, no copy); anything else is one transposing copy of a small tensor (latents, detector output)."""
        if y.C == 1 and y.padL == 0 and y.padR == 0:
            return y.data.view(y.B, 1, y.T)
        return y.interior_view().transpose(1, 2).contiguous()

    @torch.no_grad()
    def decode_latent(self, codes: torch.Tensor) -> torch.Tensor:
        c32 = self._codes32(codes)
        return self._sized("latent", int(c32.shape[0]), int(c32.shape[-1]), lambda: self._dequant(c32, None).interior_view().transpose(1, 2).contiguous())

    @torch.no_grad()
    def decode(self, codes: torch.Tensor, scale=None) -> torch.Tensor:
        assert scale is None, "renormalize=False codec: scale must be None (wmencodec.py:199-203)"
        c32 = self._codes32(codes)

        def body(lo, hi):
            z = self._dequant(c32[lo:hi], self.decoder.nodes[0])
            return (self._channel_major(self._run(self.decoder.nodes, z)),)

        return self._join(self._in_lanes(c32.shape[0], lambda lo, hi: self._sized("decode", hi - lo, int(c32.shape[-1]), lambda: body(lo, hi))), 0)

    # ------------------------------------------------------------------ streamed decode
    def decode_stream(self, max_frames: int, max_window: int = 16) -> "DecodeStream":
        """`decode` of ONE utterance in pieces, while its codes are still being generated: `push(codes [1, K, n])` returns the samples
        that have become final, `finish()` the rest; their concatenation is bit-identical to `decode` of all the codes. Every buffer is
        allocated here, for up to `max_frames` frames (create the stream before the decode engine's first launch); `max_window` = frames
        of one pass over the layers behind the LSTM."""
        return DecodeStream(self, int(max_frames), int(max_window))

    def decode_stream_batch(self, prompt_lens: Sequence[int], max_new_frames: int, max_window: int = 16) -> "BatchDecodeStream":
        """`decode_stream` for B utterances whose frames are generated in lock-step: item u has a prompt of prompt_lens[u] frames
        (`push_prompts`, never returned) and at most `max_new_frames` generated ones; `advance(new_frames, ended)` returns, per item, the
        samples that have become final. Per item the concatenation is `decode` of that item's codes at batch 1, without its prompt part,
        within the bound that holds a batched decode to the batch-1 one. Every buffer is allocated here (`BatchDecodeStream`)."""
        return BatchDecodeStream(self, [int(p) for p in prompt_lens], int(max_new_frames), int(max_window))

    def wmdecode_stream(self, max_frames: int, max_window: int = 16) -> "WMDecodeStream":
        """`wmdecode(..., with_mark=False)` of ONE utterance in pieces, while its frames are still being generated:
        `push(codes [1, K, n], labels [n], audio [1, 1, n * hop] | None)` returns the watermarked samples that have become final,
        `finish()` the rest; their concatenation is bit-identical to `wmdecode` of all the inputs. Every buffer is allocated here, for up
        to `max_frames` frames (create the stream before the decode engine's first launch); `max_window` = frames of one pass over the
        skip encoder's convolutions, and of one pass over the decoder's layers behind its LSTM."""
        return WMDecodeStream(self, int(max_frames), int(max_window))

    def wmdecode_stream_batch(self, prompt_lens: Sequence[int], max_new_frames: int, max_window: int = 16) -> "BatchWMDecodeStream":
        """`wmdecode_stream` for B utterances whose frames are generated in lock-step as zero-shot TTS: item u has a prompt of
        prompt_lens[u] frames (`push_prompts(codes, audio)`: label 0, its original audio in the kept-audio track; never returned) and at
        most `max_new_frames` generated ones (label 1, silence); `advance(new_frames, ended)` returns, per item, the watermarked samples
        that have become final. Per item the concatenation is `wmdecode(..., with_mark=False)` of that item at batch 1, without its
        prompt part, within the bound that holds a batched decode to the batch-1 one. Every buffer is allocated here
        (`BatchWMDecodeStream`)."""
        return BatchWMDecodeStream(self, [int(p) for p in prompt_lens], int(max_new_frames), int(max_window))

    # ------------------------------------------------------------------ ragged batches (items of different lengths in one pass)
    # cost model of one dense pass over a bucket, in microseconds per frame of its longest item: every frame is one LSTM time step
    # of each layer (a latency-bound launch whose cost hardly depends on the batch) + the convolutions' share per item
    # (profiles/r02_codec_b32_kernel_trace_summary.md: ~10 us per step and layer; 85 ms / (32 items x 1500 frames) per item)
    RAGGED_STEP_US = 20.0
    RAGGED_ITEM_US = 1.8
    RAGGED_MAX_FRAMES = 256 * 1500          # items x frames of one dense pass (memory: ~0.3 GB per 1500 frames in the decoder)

    def _ragged_buckets(self, lens: Sequence[int], per_item_us: Optional[float] = None) -> List[List[int]]:
        """Partition item indices into buckets that are decoded as ONE dense pass each (every item padded to its bucket's
        longest). Optimal contiguous partition of the items sorted by length under the cost model above (O(n^2)): short items
        ride along with long ones as long as the padding they add costs less than another pass's per-frame launch chain."""
        order = sorted(range(len(lens)), key=lambda i: -int(lens[i]))
        n = len(order)
        item_us = self.RAGGED_ITEM_US if per_item_us is None else per_item_us
        best = [0.0] + [float("inf")] * n           # best[j]: cost of the first j items (longest first)
        cut = [0] * (n + 1)
        for j in range(1, n + 1):
            for i in range(j):                      # bucket = sorted items i .. j-1, its longest is item i
                t_max, cnt = int(lens[order[i]]), j - i
                if cnt > 1 and cnt * t_max > self.RAGGED_MAX_FRAMES:
                    continue
                c = best[i] + t_max * (self.RAGGED_STEP_US + item_us * cnt)
                if c < best[j]:
                    best[j], cut[j] = c, i
        buckets, j = [], n
        while j > 0:
            buckets.append(order[cut[j]: j])
            j = cut[j]
        return buckets[::-1]

    def _stack_ragged(self, items: Sequence[torch.Tensor], idx: Sequence[int], lead: int, dtype, fill=0) -> Tuple[torch.Tensor, List[int]]:
        """items[i]: [1, *lead dims, T_i] (or without the leading 1) -> dense [len(idx), *lead, T_max] on the device + the lengths."""
        ts = [items[i].reshape(*items[i].shape[-(lead + 1):]) for i in idx]
        lens = [int(t.shape[-1]) for t in ts]
        out = torch.full((len(idx),) + tuple(ts[0].shape[:-1]) + (max(lens),), fill, dtype=dtype, device=self.device)
        for j, t in enumerate(ts):
            out[j, ..., : lens[j]] = t.to(self.device, dtype)
        return out, lens

    @torch.no_grad()
    def decode_ragged(self, codes: Sequence[torch.Tensor], scale=None) -> List[torch.Tensor]:
        """Batched `decode` of items of DIFFERENT lengths: codes[i] is [1, K, T_i] (or [K, T_i]); returns the list of waveforms
        [1, 1, T_i * hop]. Contract: result i == `decode(codes[i])` of that item alone (same arithmetic per output sample; the
        LSTM step kernel is chosen by batch size, so the last bits may differ) — the SEANet convolutions are not causal, so every
        layer gives each item its own halo right behind its own last row (`ssrhip_pad_ragged`) instead of padding to the longest.
        The reference decodes one utterance at a time (inference_v2.py:331-358, wmencodec.py:341-356)."""
        assert scale is None, "renormalize=False codec: scale must be None (wmencodec.py:199-203)"
        out: List[Optional[torch.Tensor]] = [None] * len(codes)
        hop = int(math.prod(self.cfg.ratios))
        for idx in self._ragged_buckets([int(c.shape[-1]) for c in codes]):
            dense, lens = self._stack_ragged(codes, idx, 1, torch.int64)
            c32 = self._codes32(dense)
            rg = Ragged(lens, self.device) if min(lens) != max(lens) else None
            # (a ragged pass allocates what the dense pass of its longest item allocates: same envelope family as `decode`)
            wav = self._sized("decode", len(idx), max(lens), lambda: self._channel_major(self._run(self.decoder.nodes, self._dequant(c32, self.decoder.nodes[0], rg))))
            for j, i in enumerate(idx):
                out[i] = wav[j: j + 1, :, : lens[j] * hop]
        return out

    @torch.no_grad()
    def wmdecode_ragged(self, codes: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], wavforms: Sequence[torch.Tensor], scale=None,
                        with_mark: bool = True):
        """Batched `wmdecode` of items of different lengths (see `decode_ragged`): codes[i] [1,K,T_i], labels[i] [1,T_i],
        wavforms[i] [1,1,T_i*hop]. Returns (list of wav [1,1,T_i*hop], list of mark [1,T_i,2] or None)."""
        assert scale is None and self.has_wm
        hop = int(math.prod(self.cfg.ratios))
        n = len(codes)
        assert len(labels) == n and len(wavforms) == n
        wavs: List[Optional[torch.Tensor]] = [None] * n
        marks: List[Optional[torch.Tensor]] = [None] * n
        for i in range(n):
            T = int(codes[i].shape[-1])
            if int(labels[i].shape[-1]) != T or int(wavforms[i].shape[-1]) != T * hop:
                raise ValueError(f"item {i}: {T} frames need {T} labels and {T * hop} samples, got {tuple(labels[i].shape)} / {tuple(wavforms[i].shape)}")
        # 3x the decoder's work per item (skip encoder + decoder [+ detector]): the per-item share of the cost model scales with it
        for idx in self._ragged_buckets([int(c.shape[-1]) for c in codes], per_item_us=3 * self.RAGGED_ITEM_US):
            dense, lens = self._stack_ragged(codes, idx, 1, torch.int64)
            lab, _ = self._stack_ragged(labels, idx, 0, torch.int64)
            wv, _ = self._stack_ragged(wavforms, idx, 0, torch.float32)
            rg = Ragged(lens, self.device) if min(lens) != max(lens) else None
            c32, l32, wv1 = self._codes32(dense), self._labels32(lab), wv.unsqueeze(1)
            w, m = self._sized("wmdecode" + ("+mark" if with_mark else ""), len(idx), max(lens), lambda: self._wmdecode_dense(c32, l32, wv1, with_mark, rg))
            for j, i in enumerate(idx):
                wavs[i] = w[j: j + 1, :, : lens[j] * hop]
                if m is not None:
                    marks[i] = m[j: j + 1, : lens[j]]
        return wavs, (marks if with_mark else None)

    def _concat_proj(self, j: int, skip: TM, labels32: torch.Tensor, rep: int, x: TM, nxt) -> TM:
        """wm_proj_j(ELU(cat(skip, wm_embed(labels upsampled)))) + x   (seanet.py:577-591) without building the concatenation:
        the 1x1 convolution splits into W_a . ELU(skip) + W_b . ELU(embed(label)); the second term has one value per label
        (`self.wm_cls[j]`, computed at load) and enters the GEMM's epilogue as a per-row class bias (include/ssrhip.h rbias)."""
        c, (Wa, cls) = self.wm_proj[j], self.wm_cls[j]
        assert skip.T == x.T and skip.C == Wa.shape[1] and labels32.shape[1] * rep >= skip.T, (skip.T, x.T, skip.C, Wa.shape, labels32.shape, rep)
        out = self._alloc_for(skip.B, skip.T, c.Cout, nxt, skip.lens)
        assert not x.elu
        self._gemm(skip.interior, Wa, c.b, out.interior, skip.T, c.Cout, skip.C, skip.C, c.Cout, act_in=self._act_in(True, skip), R=x.interior, ldr=x.C,
                   batch=skip.B, sA=skip.bstride, sC=out.bstride, sR=x.bstride, rowcls=(cls, labels32, rep))
        self._fill_pads(out, structural_zero=(nxt is not None and nxt[1] == "convtr"))
        return out

    def _labels32(self, labels: torch.Tensor) -> torch.Tensor:
        """Watermark labels on the device as int32, range-checked like the code ids: they index the class-bias table in the GEMM
        epilogue, where the reference's F.embedding (seanet.py:562) raises IndexError for an id outside the table."""
        lab = labels.to(self.device, torch.int32).contiguous()
        if lab.numel() > 0:
            lo_hi = torch.stack(torch.aminmax(lab)).tolist()
            if lo_hi[1] >= self.wm_table.shape[0] or lo_hi[0] < 0:
                raise IndexError("index out of range in self")
        return lab

    @torch.no_grad()
    def wmdecode(self, codes: torch.Tensor, labels: torch.Tensor, wavform: torch.Tensor, scale=None, with_mark: bool = True):
        """-> (wav [B,1,T], mark [B,T',2]) as wmencodec.py:358-375. `with_mark=False` skips the detector pass whose
        output `AudioTokenizer.wmdecode` discards (data/tokenizer.py:133) and returns mark=None."""
        assert scale is None and self.has_wm
        lab_all = self._labels32(labels)
        c32 = self._codes32(codes)
        parts = self._in_lanes(c32.shape[0], lambda b0, b1: self._sized(
            "wmdecode" + ("+mark" if with_mark else ""), b1 - b0, int(c32.shape[-1]),
            lambda: self._wmdecode_dense(c32[b0:b1], lab_all[b0:b1].contiguous(), wavform[b0:b1], with_mark, None)))
        return self._join(parts, 0), self._join(parts, 1)

    def _wmdecode_dense(self, c32: torch.Tensor, lab: torch.Tensor, wavform: torch.Tensor, with_mark: bool, lens: Optional[Ragged]):
        """One dense pass of the watermark decoder (seanet.py:555-600) over a batch; `lens` = per-item frame counts of a ragged batch."""
        r = list(self.cfg.ratios)
        assert len(r) == 4, "the watermark decoder's slicing (seanet.py:560-591) is written for 4 ratios"
        dec, senc = self.wmdecoder, self.skip_encoder
        cuts = [(0, 4), (4, 7), (7, 10), (10, None)]
        dn = [dec.slice_nodes(lo, hi) for lo, hi in cuts]
        reps = [r[0] * r[1] * r[2], r[0] * r[1], r[0], 1]
        lens_s = lens.scaled(int(math.prod(r))) if lens is not None else None
        # skip features at 4 scales; every skip is consumed by a k=1 conv => no halo
        z = self._run(senc.slice_nodes(0, 2), self._input_tm(wavform, senc.nodes[0], lens_s), after=senc.slice_nodes(2, 5)[0])
        sk = []
        for lo, hi in [(2, 5), (5, 8), (8, 11), (11, None)]:
            nxt_nodes = senc.slice_nodes(hi, None) if hi is not None else []
            z = self._run(senc.slice_nodes(lo, hi), z, after=(nxt_nodes[0] if nxt_nodes else None))
            sk.append(z)
        x = self._dequant(c32, None, lens)
        for j in range(4):
            skip, rep = sk[3 - j], reps[3 - j]
            out = self._concat_proj(j, skip, lab, rep, x, dn[j][0])
            x = self._run(dn[j], out, after=None)
        wav = self._channel_major(x)
        if not with_mark:
            return wav, None
        m = self._run(self.wm_encoder.nodes, self._input_tm(wav, self.wm_encoder.nodes[0], lens_s), after=None)
        mk = self._conv(self.wm_predictor, m, None)
        return wav, mk.interior_view().contiguous()

    @torch.no_grad()
    def detect_watermark(self, x: torch.Tensor) -> torch.Tensor:
        """wmencodec.py:377-382, including its argmax over the LAST dim of [B,2,T'] (time)."""
        assert x.dim() == 3

        def body(lo, hi):
            m = self._run(self.wm_encoder.nodes, self._input_tm(x[lo:hi], self.wm_encoder.nodes[0]), after=None)
            mk = self._conv(self.wm_predictor, m, None).interior_view().transpose(1, 2)      # [B,2,T']
            return (torch.argmax(mk.squeeze(-1), dim=-1),)

        return self._join(self._in_lanes(x.shape[0], lambda lo, hi: self._sized("detect", hi - lo, int(x.shape[-1]), lambda: body(lo, hi))), 0)


class _WindowPool:
    """The activation buffers of a stream's stage-2 window: allocated once, by a dry pass over the largest window, and handed out again in
    the same order for every later window (`WMEncodecModel._alloc_for`)."""

    def __init__(self):
        self.bufs: List[torch.Tensor] = []
        self.at, self.frozen = 0, False

    def take(self, B: int, T: int, Cc: int, padL: int, padR: int, device) -> TM:
        n = B * (padL + T + padR) * Cc
        if not self.frozen:
            self.bufs.append(_empty(n, dtype=torch.float32, device=device))
        if self.at >= len(self.bufs) or self.bufs[self.at].numel() < n:
            raise RuntimeError("DecodeStream: a window asks for a buffer the stream did not allocate when it was created")
        flat = self.bufs[self.at]
        self.at += 1
        return TM(B, T, Cc, padL, padR, device, data=flat[:n].view(B, padL + T + padR, Cc))


class _TMView(TM):
    """A window of rows of a larger [B][rows][C] buffer, read in place: the items are `bstride` elements apart, not rows * C."""

    def __init__(self, data: torch.Tensor, T: int, bstride: int, device):
        super().__init__(int(data.shape[0]), T, int(data.shape[2]), 1, 1, device, data=data, keep_halo=True)
        self._bstride = int(bstride)

    @property
    def bstride(self) -> int:
        return self._bstride


class _StreamCore:
    """What `DecodeStream` and `BatchDecodeStream` share: the decoder cut in two, the buffers of both halves, and every launch over them.

    Stage 1 — dequantiser, first convolution, LSTM + skip — runs once over every row: the convolution's GEMM over the rows whose
    look-ahead has arrived, the LSTM behind it as `ssrhip_lstm_layer` calls that continue (`t_begin` > 0) on the stream's own `gin` /
    `hbuf` / `cbuf`. Stage 2 — everything behind the LSTM — runs over windows of stage-1 output, read in place, into buffers that one
    dry pass over the largest window allocated. Every launch is the one `decode` issues for the same layer, over fewer rows, on the
    caller's stream.

    The core counts ROWS of a time axis [B][rows]; which frame of which item lives in which row is the derived class's business
    (`DecodeStream`: frame t is row t; `BatchDecodeStream`: `batch_align_plan`). The one thing it has to be told is `conv_row0`, the first
    row the convolution computes: the convolution's row r reads the rows [r - conv_row0, r - conv_row0 + pl0 + pr0] of `z.data`."""

    def __init__(self, model: WMEncodecModel, entry: str, max_window: int, nodes: Optional[List[tuple]] = None):
        """`nodes`: the decoder to stream (`WMDecodeStream`: the watermark decoder's); None = `model.decoder`'s."""
        cfg, nodes = model.cfg, (model.decoder.nodes if nodes is None else nodes)
        self.m, self.max_window = model, max_window
        self.hop = int(math.prod(cfg.ratios))
        self.conv0: _Conv = nodes[0][2]
        self.lstm: Optional[_Lstm] = nodes[1][2] if nodes[1][1] == "lstm" else None
        self.tail = nodes[2:] if self.lstm is not None else nodes[1:]
        c0 = self.conv0
        if not (nodes[0][1] == "conv" and c0.s == 1 and c0.Cin > 1 and c0.Cout > 4 and self.tail and self.tail[0][1] == "convtr"):
            raise NotImplementedError(f"{entry}: the decoder does not start with a stride-1 convolution into a transposed convolution")
        self.pl0, self.pr0 = c0.pl, c0.pr                             # stride 1: no length-dependent extra padding
        self.margins = stream_margins(cfg)
        self.reflect = cfg.pad_mode == "reflect"
        last = nodes[-1][2]
        self._few_eligible = last.Cout <= 4 and last.s == 1 and last.Cin % 8 == 0       # `_conv`'s conditions on the layer itself

    def _allocate(self, B: int, rows: int, conv_row0: int, out_frames: int):
        """Every buffer of both stages, for B items of `rows` rows each, and `wav` for `out_frames` frames per item. Zero-filled: halo
        rows, and rows behind an item's last frame, must read as zeros."""
        m, c0 = self.m, self.conv0
        dev, D, C0 = m.device, m.cfg.dimension, c0.Cout
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.rows, self.conv_row0 = B, rows, conv_row0
        self.z = TM(B, rows - conv_row0, D, self.pl0, self.pr0, dev, data=torch.zeros(B, self.pl0 + rows - conv_row0 + self.pr0, D, **f32))
        self.s1 = TM(B, rows, C0, 1, 1, dev, data=torch.zeros(B, rows + 2, C0, **f32))      # what the first convtr reads
        self.s1.elu = bool(m.elu_on_store and self.lstm is not None)
        # the item stride of `s1` as the stage-1 launches are given it. One item: nothing multiplies it by anything but 0, and
        # `DecodeStream` has always passed the plain rows * C0 of its other buffers
        self._s1_bs = self.s1.bstride if B > 1 else rows * C0
        if self.lstm is not None:
            L, nl = self.lstm, len(self.lstm.layers)
            assert L.C == C0
            self.y0 = torch.zeros(B, rows, C0, **f32)
            self.gins = [torch.zeros(B, rows, 4 * C0, **f32) for _ in range(nl)]
            self.hbufs = [torch.zeros(2, (B + 15) // 16 * 16, C0, **f32) for _ in range(nl)]
            self.cbufs = [torch.zeros(B, C0, **f32) for _ in range(nl)]
            self.mids = [torch.zeros(B, rows, C0, **f32) for _ in range(nl - 1)]
            split = m._lstm_use_split(L, B)
            self.hsplits = [torch.zeros(2 * ((B + 63) // 64) * 64 * C0 * 3, dtype=torch.int16, device=dev) if (split and L.split[l] is not None)
                            else None for l in range(nl)]
        self.wav = torch.zeros(B, 1, out_frames * self.hop, **f32)
        self.n1 = 0                                                    # rows whose stage-1 output is final
        self.windows = self.windows_batched = 0                        # stage-2 passes so far; those of them over every item at once
        # stage 2: the buffers of the largest window — an interior one of max_window frames — of all B items at once (B > 1) and of one
        # item, each by one dry pass (no launch)
        self.pool_b, self.pool_1 = (_WindowPool() if B > 1 else None), _WindowPool()
        real, m.lib = m.lib, _NoLaunch()
        try:
            n = min(rows, self.max_window + self.margins[0] + self.margins[1])
            if B > 1:
                self._tail_pass(0, n, None)
                self.pool_b.frozen = True
            self._tail_pass(0, n, 0)
            self.pool_1.frozen = True
        finally:
            m.lib = real
        torch.cuda.current_stream(dev).synchronize()                  # the fills above are done before anything else is enqueued

    def _tail_pass(self, lo: int, hi: int, item: Optional[int], few: bool = False) -> TM:
        """The layers behind the LSTM over the stage-1 rows [lo, hi), read in place (the rows next to the window are its halo: a true
        neighbour, or the zero row an end of the utterance needs): of every item (`item` None: one batched call per layer) or of one.
        `few`: the last layer runs as the few-output kernel, as `decode` of the whole utterance runs it."""
        m, s1 = self.m, self.s1
        if item is None:
            x, pool = _TMView(s1.data[:, lo: hi + 2], hi - lo, s1.bstride, m.device), self.pool_b
        else:
            x, pool = TM(1, hi - lo, s1.C, 1, 1, m.device, data=s1.data[item: item + 1, lo: hi + 2], keep_halo=True), self.pool_1
        x.elu = s1.elu
        with m._stream_pass(pool, few):
            return m._run(self.tail, x)

    def _stage1_rows(self, a: int, b: int, front=()):
        """Stage 1 over the rows [a, b) of every item, a = `n1`: the first convolution's GEMM over those of them it computes, then per LSTM
        layer `_lstm_in_gemm` and `_lstm_steps`. `front` = (item, e) pairs: the rows [a, e) lie in front of that item's first frame — the
        skip input and every layer's `gin` are zeroed there, so that the item's LSTM state stays exactly zero (`BatchDecodeStream`)."""
        m, z, c0, s1, B, rows = self.m, self.z, self.conv0, self.s1, self.B, self.rows
        D, C0, L = z.C, c0.Cout, self.lstm
        bs = rows * C0                                                # item stride of y0 / mids
        dst, dst_bs = (self.y0, bs) if L is not None else (s1.data[:, 1:], self._s1_bs)
        ca = max(a, self.conv_row0)
        if b > ca:                                                    # `_conv`'s GEMM: row t of the im2col view starts at z's row t - conv_row0
            m._gemm(z.base + 4 * (ca - self.conv_row0) * D, c0.W, c0.b, dst.data_ptr() + 4 * ca * C0, b - ca, C0, c0.k * c0.Cin, c0.s * c0.Cin, C0,
                    act_in=m._act_in(bool(c0.act_in), z), batch=B, sA=z.bstride, sC=dst_bs)
        for u, e in front:
            dst[u, a:e].zero_()
        nl = len(L.layers) if L is not None else 0
        for l in range(nl):
            src, last = (self.y0 if l == 0 else self.mids[l - 1]), l == nl - 1
            m._lstm_in_gemm(L, l, src.data_ptr(), bs, self.gins[l], B, rows, a, b)
            for u, e in front:
                self.gins[l][u, a:e].zero_()                          # zero pre-activation from h = c = 0: the state stays exactly zero
            m._lstm_steps(L, l, self.gins[l], self.hbufs[l], self.cbufs[l], self.hsplits[l], (s1.interior if last else self.mids[l].data_ptr()),
                          (self._s1_bs if last else bs), (self.y0.data_ptr() if last else 0), bs, B, rows, a, b, s1.elu and last)
        self.n1 = b

    def _window_rule(self) -> tuple:
        """What `batch_window_item` takes behind an item's own state: (margins, max_window, hop, few_min_t, few_eligible)"""
        m = self.m          # (`force_few_out`: `_conv` takes the few-output kernel whatever the rule says, so the rule waits for nothing)
        return self.margins, self.max_window, self.hop, m.FEW_OUT_MIN_T, self._few_eligible and not m.force_few_out

    def _run_window(self, win: tuple, item: Optional[int], who: Sequence[int], row0: int):
        """One stage-2 pass over the window `win` — of every item (`item` None) or of one — and the copy of its core [c0, c1) into `wav`
        for the items `who`; `row0` = the row of `wav`'s first frame."""
        (c0, c1, lo, hi, few), hop = win, self.hop
        y = self._tail_pass(lo, hi, item, few)
        assert y.C == 1 and y.padL == 0 and y.T == (hi - lo) * hop
        flat = y.data.view(y.B, -1)
        s0, s1_, d0, d1 = (c0 - lo) * hop, (c1 - lo) * hop, (c0 - row0) * hop, (c1 - row0) * hop
        if item is None and len(who) == self.B:
            self.wav[:, 0, d0:d1].copy_(flat[:, s0:s1_])
        else:
            for u in who:
                self.wav[u, 0, d0:d1].copy_(flat[u if item is None else 0, s0:s1_])
        self.windows += 1
        self.windows_batched += int(item is None)


class DecodeStream(_StreamCore):
    """`WMEncodecModel.decode_stream`: the decoder of one utterance (B = 1), advanced as its frames arrive — `_StreamCore` with frame t in
    row t.

    Stage 1 runs over the frames whose look-ahead (`stream_lookahead`) has arrived. Stage 2 runs over windows of stage-1 output with the
    margins of `stream_margins` on either side, whose samples are dropped; an end of the utterance is a true edge (the layers' own
    padding, no margin). Frames nearer to the current end than look-ahead + margin wait for more frames or for `finish()`. Where a
    launcher chooses by length (`_conv`'s few-output kernel from `FEW_OUT_MIN_T` rows on) the stream waits until the whole utterance's
    choice is known and takes it (`batch_window_item`, the one window rule of both streams)."""

    def __init__(self, model: WMEncodecModel, max_frames: int, max_window: int):
        if max_frames < 1 or max_window < 1:
            raise ValueError("decode_stream needs max_frames >= 1 and max_window >= 1")
        super().__init__(model, "decode_stream", max_window)
        self.cap = max_frames
        self.codes = torch.zeros(model.cfg.n_q * max_frames, dtype=torch.int32, device=model.device)
        self.lohi = torch.zeros(2, dtype=torch.int32, device=model.device)
        self.n_pushed = 0          # frames whose codes have arrived
        self.n2 = 0                # frames whose samples have been written (and, from `emit_from` on, returned)
        self.emit_from: Optional[int] = None
        self.finished = False
        self._allocate(1, max_frames, 0, max_frames)

    def _stage1(self, final: bool):
        m, z, n = self.m, self.z, self.n_pushed
        ready = n if final else n - self.pr0
        if self.reflect and not final and n <= max(self.pl0, self.pr0):
            ready = 0                                                 # reflect padding of so short an input depends on its length
        a, b = self.n1, max(ready, self.n1)
        if b == a:
            return
        if self.reflect:                                             # (constant padding: the zero rows the buffer was created with)
            if final:
                m._call("ssrhip_pad_reflect", z.base, 1, n, self.pl0, self.pr0, z.C, z.bstride)
            elif a == 0:
                m._call("ssrhip_pad_reflect", z.base, 1, n, self.pl0, 0, z.C, z.bstride)
        self._stage1_rows(a, b)

    def _stage2(self, final: bool):
        if self.emit_from is None:
            return
        rule = self._window_rule()
        while True:                                                   # one item: off = 0, E = emit_from, top = n_pushed, closed = final
            win = batch_window_item(0, self.emit_from, self.n2, self.n_pushed, self.n1, final, *rule)
            if win is None:
                return
            self._run_window(win, 0, [0], 0)
            self.n2 = win[1]

    def _out(self, a: int) -> torch.Tensor:
        return self.wav[:, :, a * self.hop: self.n2 * self.hop]

    @torch.no_grad()
    def push(self, codes: torch.Tensor, emit: bool = True) -> torch.Tensor:
        """codes [1, K, n] (any device; n may be 0): the next n frames. Returns the samples that became final, [1, 1, m * hop] (a view
        of the stream's output buffer; m may be 0). `emit=False` (only in front of every emitted frame): the frames run through stage
        1 — the LSTM state has to pass through them — and are never returned."""
        if self.finished:
            raise RuntimeError("DecodeStream.push after finish()")
        cfg = self.m.cfg
        assert codes.dim() == 3 and codes.shape[0] == 1 and codes.shape[1] == cfg.n_q, tuple(codes.shape)
        n = int(codes.shape[-1])
        if self.n_pushed + n > self.cap:
            raise ValueError(f"DecodeStream: {self.n_pushed} + {n} frames exceed max_frames = {self.cap}")
        if not emit and self.emit_from is not None:
            raise ValueError("DecodeStream: emit=False frames must come before every emitted frame")
        if emit and self.emit_from is None:
            self.emit_from = self.n2 = self.n_pushed
        a = self.n2
        if n == 0:
            return self._out(a)
        c32 = self.codes[: cfg.n_q * n].view(1, cfg.n_q, n)
        c32.copy_(codes)
        # the range check `decode` makes (core_vq.py:175 raises in the reference), before the ids index the codebooks
        torch.amin(c32, dim=(0, 1, 2), out=self.lohi[0])
        torch.amax(c32, dim=(0, 1, 2), out=self.lohi[1])
        lo, hi = self.lohi.tolist()
        if hi >= cfg.bins or lo < 0:
            raise IndexError("index out of range in self")
        z = self.z
        self.m._call("ssrhip_rvq_decode", c32.data_ptr(), self.m.codebooks.data_ptr(), z.interior + 4 * self.n_pushed * z.C, 1, n, z.C, cfg.n_q,
                   cfg.bins, z.bstride)
        self.n_pushed += n
        self._stage1(False)
        self._stage2(False)
        return self._out(a)

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """The utterance ends here: its right edge gets the layers' own padding, and the samples still held back are returned."""
        if self.finished:
            raise RuntimeError("DecodeStream.finish called twice")
        self.finished = True
        if self.emit_from is None:
            self.emit_from = self.n2 = self.n_pushed
        a = self.n2
        if self.n_pushed:
            self._stage1(True)
            self._stage2(True)
        return self._out(a)


# ----------------------------------------------------------------------------- streamed watermarked decode (DESIGN.md Part I.17)
def _wm_stream_cut(st: "_StreamCore", model: WMEncodecModel, entry: str, max_window: int):
    """What the watermarked streams (`WMDecodeStream`, `BatchWMDecodeStream`) share ahead of their buffers: `_StreamCore` over the
    watermark decoder's nodes, the skip encoder cut as `_wmdecode_dense` cuts it, the margins and the rows per frame of the taps."""
    if not model.has_wm:
        raise ValueError(f"{entry}: this codec has no watermark decoder")
    cfg = model.cfg
    r = list(cfg.ratios)
    senc, dec = model.skip_encoder, model.wmdecoder
    rest = senc.slice_nodes(11, None)
    if len(r) != 4 or [n[1] for n in rest] != ["conv", "lstm", "conv"] or [n[1] for n in dec.nodes[:3]] != ["conv", "lstm", "convtr"]:
        raise NotImplementedError(f"{entry}: the watermark decoder's slicing (seanet.py:560-591) is written for 4 ratios and an LSTM")
    _StreamCore.__init__(st, model, entry, max_window, nodes=dec.nodes)       # (not DecodeStream's: other buffers)
    # the skip encoder, cut as `_wmdecode_dense` cuts it; its last slice once more, around the LSTM
    st.ch_head = senc.slice_nodes(0, 2)
    st.ch_cuts = [senc.slice_nodes(lo, hi) for lo, hi in ((2, 5), (5, 8), (8, 11))]
    st.ch_last, st.sk_lstm_node, st.sk_conv = rest[0], rest[1], rest[2][2]
    st.sk_lstm = rest[1][2]
    c = st.sk_conv
    if not (c.s == 1 and c.Cin == st.sk_lstm.C and c.Cout > 4):
        raise NotImplementedError(f"{entry}: the skip encoder does not end with a stride-1 convolution behind its LSTM")
    st.smargins = skip_stream_margins(cfg)
    st.holdback = wm_stream_holdback(cfg)
    st.reps = [r[0] * r[1] * r[2], r[0] * r[1], r[0]]          # rows per frame of the taps, in the chain's order
    # the decoder behind its LSTM, cut where the taps enter: [convtr] | [res, convtr] | [res, convtr] | [res, convtr, res, conv]
    dn = [dec.slice_nodes(lo, hi) for lo, hi in ((0, 4), (4, 7), (7, 10), (10, None))]
    st.dn = [dn[0][2:]] + dn[1:]
    assert [n for part in st.dn for n in part] == list(st.tail)


class WMDecodeStream(DecodeStream):
    """`WMEncodecModel.wmdecode_stream`: `_wmdecode_dense` of one utterance (B = 1, no detector pass), advanced as its frames arrive.
    Frame t is row t of every frame-rate buffer. Per `push`, in this order, each stage as far as its input allows:

      track   the kept-audio samples of the new frames, copied into a zero-filled [max_frames * hop] buffer (None = silence);
      chain   the skip encoder's convolutions up to its last strided one, over windows of the track with `skip_stream_margins` on either
              side (an end of the utterance is a true edge): the cores of the three high-rate taps go into whole-utterance buffers —
              STORED, not recomputed per decoder window — and the frame-rate rows into `p`;
      LSTM    the skip encoder's, as continuation calls over the new rows of `p` (`ssrhip_lstm_layer`, t_begin > 0) into `u`;
      tap 4   the skip encoder's last convolution over the rows of `u` whose look-ahead has arrived;
      z       wm_proj0(ELU(tap 4), label) + dequantised codes — `_concat_proj(0, ...)`'s GEMM over those rows, into the decoder's input;
      stage 1 the decoder's first convolution and LSTM (`_stage1_rows`);
      stage 2 windows of the layers behind it (`batch_window_item`), `_concat_proj(j)` behind each of the first three transposed
              convolutions with the label and tap pointers at the window's first row.

    So a frame's samples leave once `wm_stream_holdback` further frames exist. With reflect padding a frame-rate convolution whose input
    is not yet longer than its padding waits (the padding of so short an input depends on its length). Every launch is the one
    `wmdecode` issues for the same layer, over fewer rows, on the caller's stream; everything is allocated here."""

    def __init__(self, model: WMEncodecModel, max_frames: int, max_window: int):
        if max_frames < 1 or max_window < 1:
            raise ValueError("wmdecode_stream needs max_frames >= 1 and max_window >= 1")
        _wm_stream_cut(self, model, "wmdecode_stream", max_window)
        cfg, dev, c = model.cfg, model.device, self.sk_conv
        self.cap = cap = max_frames
        hop, D, Cs = self.hop, cfg.dimension, self.sk_lstm.C
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.codes = torch.zeros(cfg.n_q * cap, **i32)
        self.lab = torch.zeros(1, cap, **i32)
        self.lohi = torch.zeros(4, **i32)
        self.track = torch.zeros(cap * hop, **f32)
        self.q = torch.zeros(cap, D, **f32)                           # the dequantised codes
        self.taps = [torch.zeros(1, cap * rep, part[-1][2][1].Cout, **f32) for part, rep in zip(self.ch_cuts, self.reps)]
        self.p = torch.zeros(1, cap, Cs, **f32)                       # the chain's frame-rate rows: what the skip encoder's LSTM reads
        nl = len(self.sk_lstm.layers)
        self.sk_gins = [torch.zeros(1, cap, 4 * Cs, **f32) for _ in range(nl)]
        self.sk_hbufs = [torch.zeros(2, 16, Cs, **f32) for _ in range(nl)]
        self.sk_cbufs = [torch.zeros(1, Cs, **f32) for _ in range(nl)]
        self.sk_mids = [torch.zeros(1, cap, Cs, **f32) for _ in range(nl - 1)]
        split = model._lstm_use_split(self.sk_lstm, 1)
        self.sk_hsplits = [torch.zeros(2 * 64 * Cs * 3, dtype=torch.int16, device=dev) if (split and self.sk_lstm.split[l] is not None) else None
                           for l in range(nl)]
        self.u = TM(1, cap, Cs, c.pl, c.pr, dev, data=torch.zeros(1, c.pl + cap + c.pr, Cs, **f32))     # LSTM + skip: what `sk_conv` reads
        self.u.elu = bool(model.elu_on_store and c.act_in)
        self.tap4 = torch.zeros(1, cap, c.Cout, **f32)
        self.n_pushed = 0          # frames that have arrived
        self.nA = 0                # frames the chain and the skip encoder's LSTM have reached
        self.nC = 0                # frames whose tap 4 and decoder input `z` are final
        self.n2 = 0
        self.emit_from: Optional[int] = None
        self.finished = False
        # the chain's window buffers by a dry pass over its largest window; those of stage 2 likewise, in `_allocate`
        self.pool_c = _WindowPool()
        self.tap_elu = [False] * 3
        real, model.lib = model.lib, _NoLaunch()
        try:
            taps, _ = self._chain_pass(0, min(cap, max_window + self.smargins[0] + self.smargins[1]))
            self.tap_elu = [t.elu for t in taps]
            self.pool_c.frozen = True
        finally:
            model.lib = real
        self._allocate(1, cap, 0, cap)

    # ------------------------------------------------------------------ the skip encoder
    def _chain_pass(self, lo: int, hi: int) -> Tuple[List[TM], TM]:
        """The skip encoder's convolutions over the track's frames [lo, hi), as `_wmdecode_dense` runs them over a waveform of that
        length -> (the three taps, the frame-rate rows in front of the LSTM), in the chain pool's buffers."""
        m, hop = self.m, self.hop
        with m._stream_pass(self.pool_c, False):
            x = m._input_tm(self.track[lo * hop: hi * hop].view(1, 1, -1), self.ch_head[0])
            z = m._run(self.ch_head, x, after=self.ch_cuts[0][0])
            taps = []
            for i, part in enumerate(self.ch_cuts):
                z = m._run(part, z, after=(self.ch_cuts[i + 1][0] if i + 1 < len(self.ch_cuts) else self.ch_last))
                taps.append(z)
            return taps, m._run([self.ch_last], z, after=self.sk_lstm_node)

    def _chain(self, final: bool):
        """Chain windows over the frames whose right margin has arrived, then the skip encoder's LSTM over the new rows."""
        m, n, a = self.m, self.n_pushed, self.nA
        limit = n if final else n - self.smargins[1]
        while self.nA < limit:
            c0, c1 = self.nA, min(self.nA + self.max_window, limit)
            lo, hi = stream_window(c0, c1, n, self.smargins)
            taps, rows = self._chain_pass(lo, hi)
            for buf, t, rep in zip(self.taps + [self.p], taps + [rows], self.reps + [1]):
                buf[0, c0 * rep: c1 * rep].copy_(t.interior_view()[0, (c0 - lo) * rep: (c1 - lo) * rep])
            self.nA = c1
        b = self.nA
        if b == a:
            return
        L, cap, u = self.sk_lstm, self.cap, self.u
        nl, bs = len(L.layers), cap * L.C
        for l in range(nl):
            src, last = (self.p if l == 0 else self.sk_mids[l - 1]), l == nl - 1
            m._lstm_in_gemm(L, l, src.data_ptr(), bs, self.sk_gins[l], 1, cap, a, b)
            m._lstm_steps(L, l, self.sk_gins[l], self.sk_hbufs[l], self.sk_cbufs[l], self.sk_hsplits[l],
                          (u.interior if last else self.sk_mids[l].data_ptr()), bs, (self.p.data_ptr() if last else 0), bs, 1, cap, a, b,
                          u.elu and last)

    def _edge_rows(self, buf: TM, n: int, done: int, final: bool) -> int:
        """How far a stride-1 convolution over `buf` (halo = its paddings) can go when the rows [0, n) of its input exist and `done` are
        computed: to n less its look-ahead, or to n at the utterance's end — `DecodeStream._stage1`'s rule. Reflect padding: the halo rows
        the new outputs read are written here (the left ones with the first output, the right ones at the end)."""
        ready = n if final else n - buf.padR
        if self.reflect and not final and n <= max(buf.padL, buf.padR):
            ready = 0                                                 # reflect padding of so short an input depends on its length
        ready = max(ready, done)
        if ready > done and self.reflect:
            if final:
                self.m._call("ssrhip_pad_reflect", buf.base, 1, n, buf.padL, buf.padR, buf.C, buf.bstride)
            elif done == 0:
                self.m._call("ssrhip_pad_reflect", buf.base, 1, n, buf.padL, 0, buf.C, buf.bstride)
        return ready

    def _decoder_input(self, final: bool):
        """Tap 4 (`_conv` of the skip encoder's last convolution) and `z` (`_concat_proj(0, ...)`) over the rows whose look-ahead in
        `u` has arrived."""
        m, u, c, z = self.m, self.u, self.sk_conv, self.z
        a, b = self.nC, self._edge_rows(u, self.nA, self.nC, final)
        if b == a:
            return
        m._gemm(u.base + 4 * a * u.C, c.W, c.b, self.tap4.data_ptr() + 4 * a * c.Cout, b - a, c.Cout, c.k * c.Cin, c.s * c.Cin, c.Cout,
                act_in=m._act_in(bool(c.act_in), u), batch=1, sA=u.bstride, sC=self.cap * c.Cout)
        pj, (Wa, cls) = m.wm_proj[0], m.wm_cls[0]
        Cs, D = int(Wa.shape[1]), z.C
        assert Cs == c.Cout and pj.Cout == D
        m._gemm(self.tap4.data_ptr() + 4 * a * Cs, Wa, pj.b, z.interior + 4 * a * D, b - a, D, Cs, Cs, D, act_in=_lib.ACT_ELU,
                R=self.q.data_ptr() + 4 * a * D, ldr=D, batch=1, sA=self.cap * Cs, sC=z.bstride, sR=self.cap * D,
                rowcls=(cls, self.lab[:, a:b], 1))
        self.nC = b

    def _stage1(self, final: bool):
        self._chain(final)
        self._decoder_input(final)
        a, b = self.n1, self._edge_rows(self.z, self.nC, self.n1, final)
        if b > a:
            self._stage1_rows(a, b)

    def _tail_pass(self, lo: int, hi: int, item: Optional[int], few: bool = False) -> TM:
        """`_StreamCore._tail_pass` with the taps: `_concat_proj(j)` behind each of the first three transposed convolutions, reading the
        stored tap's rows of the window in place and the labels from the window's first frame on."""
        m, s1 = self.m, self.s1
        assert item == 0
        x = TM(1, hi - lo, s1.C, 1, 1, m.device, data=s1.data[:, lo: hi + 2], keep_halo=True)
        x.elu = s1.elu
        with m._stream_pass(self.pool_1, few):
            y = m._run(self.dn[0], x, after=None)
            for j in (1, 2, 3):
                tap, rep = self.taps[3 - j], self.reps[3 - j]
                skip = TM(1, (hi - lo) * rep, int(tap.shape[2]), 0, 0, m.device, data=tap[:, lo * rep: hi * rep], keep_halo=True)
                skip.elu = self.tap_elu[3 - j]
                y = m._run(self.dn[j], m._concat_proj(j, skip, self.lab[:, lo:hi], rep, y, self.dn[j][0]), after=None)
            return y

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def push(self, codes: torch.Tensor, labels: torch.Tensor, audio: Optional[torch.Tensor] = None, emit: bool = True) -> torch.Tensor:
        """The next n frames (n may be 0): codes [1, K, n], labels [n] or [1, n] (0 kept / 1 generated), audio [1, 1, n * hop] — the
        kept-audio track under these frames; None = silence, what `kept_audio_track` puts under generated frames. Returns the samples
        that became final, [1, 1, m * hop] (a view of the stream's output buffer; m may be 0). `emit=False` (only in front of every
        emitted frame): the frames pass through both LSTMs and are never returned."""
        if self.finished:
            raise RuntimeError("WMDecodeStream.push after finish()")
        cfg, hop = self.m.cfg, self.hop
        assert codes.dim() == 3 and codes.shape[0] == 1 and codes.shape[1] == cfg.n_q, tuple(codes.shape)
        n, at = int(codes.shape[-1]), self.n_pushed
        if labels.numel() != n or (audio is not None and audio.numel() != n * hop):
            raise ValueError(f"WMDecodeStream: {n} frames need {n} labels and {n * hop} samples, got {tuple(labels.shape)} / "
                             f"{None if audio is None else tuple(audio.shape)}")
        if at + n > self.cap:
            raise ValueError(f"WMDecodeStream: {at} + {n} frames exceed max_frames = {self.cap}")
        if not emit and self.emit_from is not None:
            raise ValueError("WMDecodeStream: emit=False frames must come before every emitted frame")
        if emit and self.emit_from is None:
            self.emit_from = self.n2 = at
        a = self.n2
        if n == 0:
            return self._out(a)
        c32, l32 = self.codes[: cfg.n_q * n].view(1, cfg.n_q, n), self.lab[:, at: at + n]
        c32.copy_(codes)
        l32.copy_(labels.reshape(1, n))
        # the range checks `wmdecode` makes (`_codes32`, `_labels32`), before the ids index the codebooks and the class-bias table
        for i, t in enumerate((c32, l32)):
            torch.amin(t, dim=tuple(range(t.dim())), out=self.lohi[2 * i])
            torch.amax(t, dim=tuple(range(t.dim())), out=self.lohi[2 * i + 1])
        c_lo, c_hi, l_lo, l_hi = self.lohi.tolist()
        if c_hi >= cfg.bins or c_lo < 0 or l_hi >= self.m.wm_table.shape[0] or l_lo < 0:
            raise IndexError("index out of range in self")
        if audio is not None:
            self.track[at * hop: (at + n) * hop].copy_(audio.reshape(-1))
        D = self.q.shape[1]
        self.m._call("ssrhip_rvq_decode", c32.data_ptr(), self.m.codebooks.data_ptr(), self.q.data_ptr() + 4 * at * D, 1, n, D, cfg.n_q,
                     cfg.bins, self.cap * D)
        self.n_pushed += n
        self._stage1(False)
        self._stage2(False)
        return self._out(a)


# ----------------------------------------------------------------------------- streamed decode of a lock-step batch (DESIGN.md Part I.16)
def batch_align_plan(prompt_lens: Sequence[int], pl0: int) -> dict:
    """The one time axis of a `BatchDecodeStream`: item u's frame t lives in row off[u] + t with off[u] = pl0 + (P_max - P_u), so every
    prompt ENDS at row E = pl0 + P_max and generated frame j of every item is row E + j. `zero[u]` = the rows [0, off[u]) in front of
    item u's first frame, whose LSTM input and skip input are zeroed so that its state is exactly zero when its first frame arrives."""
    lens = [int(p) for p in prompt_lens]
    if not lens or min(lens) < 1:
        raise ValueError(f"decode_stream_batch needs at least one item and a prompt of at least one frame each, got {lens}")
    p_max = max(lens)
    off = [int(pl0) + p_max - p for p in lens]
    return dict(off=off, E=int(pl0) + p_max, zero=[(0, o) for o in off])


def batch_stage1_range(n1: int, tops: Sequence[int], ended: Sequence[bool], closed: Sequence[bool], lookahead: int) -> Tuple[int, int]:
    """The rows [a, b) ONE batched stage-1 call (first convolution + LSTM, all items) advances over. tops[u] = the row behind item u's
    last arrived frame. A live item allows the rows whose look-ahead has arrived, tops[u] - lookahead; the call goes as far as every live
    item allows. An item that has ended adds no limit (behind its end its rows are not read by anyone): it is CLOSED by the first call
    with b >= tops[u]. When no live item is left the call runs to the last end."""
    live = [t - int(lookahead) for t, e in zip(tops, ended) if not e]
    if live:
        b = min(live)
    else:
        b = max([t for t, c in zip(tops, closed) if not c], default=n1)
    return int(n1), max(int(b), int(n1))


def batch_window_item(off: int, E: int, n2: int, top: int, n1: int, closed: bool, margins: Tuple[int, int], max_window: int, hop: int,
                      few_min_t: int, few_eligible: bool):
    """The next stage-2 window of ONE item, in rows — the window rule of both streams (a `DecodeStream` is the
    item with off = 0, E = its first emitted frame, top = the frames pushed, closed = `finish()` was called):
    -> (c0, c1, lo, hi, few) or None (nothing to emit yet). off = the item's first row, n2 = the row its output has reached (>= E: the
    prompt is never emitted), top = the row behind its last arrived frame, n1 = the row stage 1 has reached, closed = the item has ended
    and stage 1 has passed its end (`top` is then a true edge: the layers' own padding, no margin). `few`: does `decode` of the whole
    item run its last layer as the few-output kernel — unknown (None -> wait) while the item is short and may still grow."""
    frames = top - off
    if not few_eligible:
        few = False
    elif frames * hop >= few_min_t:
        few = True
    else:
        few = False if closed else None
    if few is None:
        return None
    n = top if closed else min(n1, top)
    limit = n if closed else n - margins[1]
    c0 = max(n2, E)
    if c0 >= limit:
        return None
    c1 = min(c0 + max_window, limit)
    lo, hi = stream_window(c0 - off, c1 - off, n - off, margins)
    return c0, c1, lo + off, hi + off, few


def batch_window_groups(wins: Sequence[Optional[tuple]]) -> Tuple[Optional[tuple], List[int], List[int]]:
    """Which items run their next window in ONE batched call: the items whose windows agree (same rows, same core, same last-layer
    kernel) — the largest such set, when it has at least two members; the others run alone. An item whose prompt is shorter than the
    left margin disagrees at its first window (the window would cross its first frame, a true edge), an item that has ended at its last.
    -> (the batched window or None, its members, the items that run alone)."""
    by_key: dict = {}
    for u, w in enumerate(wins):
        if w is not None:
            by_key.setdefault(w, []).append(u)
    if not by_key:
        return None, [], []
    key = max(by_key, key=lambda k: (len(by_key[k]), [-v for v in k[:4]]))
    if len(by_key[key]) < 2:
        return None, [], sorted(u for us in by_key.values() for u in us)
    return key, by_key[key], sorted(u for k, us in by_key.items() if k != key for u in us)


class BatchDecodeStream(_StreamCore):
    """`WMEncodecModel.decode_stream_batch`: the decoders of B utterances that are generated in lock-step, advanced together as their
    frames arrive — `_StreamCore` with B items: every per-poll operation of `DecodeStream` as ONE dense batched call of the same kernels.

    One aligned time axis (`batch_align_plan`): item u's frame t is row off_u + t of buffers [B][rows][C]; the prompts all end at row E,
    generated frame j of every item is row E + j. Per `advance`: one `ssrhip_rvq_decode` with B items, the first convolution's GEMM with
    batch = B, `_lstm_in_gemm` / `_lstm_steps` with B items over a common [a, b) (`batch_stage1_range`), and the layers behind the LSTM
    over a TM(B, ...) view with a common window (`batch_window_groups`). No arithmetic kernel is new or changed.

    A row in front of an item's first frame must leave its LSTM state exactly zero. The rows [0, off_u) of every layer's `gin` and of the
    skip input `y0` are zeroed ahead of that layer's step call; then with h = c = 0 and a zero pre-activation every gate sees 0:
    c' = sigmoid(0) * 0 + sigmoid(0) * tanh(0) = 0 and h' = sigmoid(0) * tanh(0) = 0 exactly (tanh(0) = 0 and x * 0 = 0 are exact in
    fp32, whatever the kernel's sigmoid returns for 0), the written row is h' + skip = 0, or ELU(0) = 0, and the next layer's input rows
    are zero again. By induction the state entering row off_u is the h = c = 0 a batch-1 decode starts from (tests/test_gpu_stream_batch.py).

    An item that ends gets its right edge — zero rows, or its own reflected rows, behind its last frame in `z` — ahead of the batched
    stage-1 call that passes its end; its stage-1 rows from the end on are zeroed after that call and its last windows run alone (stage 2
    has no state). Later batched calls write junk into a finished item's rows, which nothing reads. B stays constant for the life of the
    stream: `ssrhip_lstm_layer` chooses its kernel by B, and an item's values must not change kernel mid-utterance.

    Everything runs on the caller's stream; every buffer — also those of the largest batched window and of a B = 1 window, each found by
    one dry pass — is allocated here, so create the stream before the decode engine's first launch."""

    def __init__(self, model: WMEncodecModel, prompt_lens: Sequence[int], max_new_frames: int, max_window: int):
        if max_new_frames < 1 or max_window < 1:
            raise ValueError("decode_stream_batch needs max_new_frames >= 1 and max_window >= 1")
        super().__init__(model, "decode_stream_batch", int(max_window))
        self.max_new = int(max_new_frames)
        plan = batch_align_plan(prompt_lens, self.pl0)
        self.prompt_lens = [int(p) for p in prompt_lens]
        self.off, self.E = plan["off"], plan["E"]
        B = len(self.off)
        if self.reflect and min(self.prompt_lens) <= max(self.pl0, self.pr0):
            raise ValueError(f"decode_stream_batch: with reflect padding every prompt must be longer than the first convolution's padding "
                             f"({max(self.pl0, self.pr0)} frames), got {self.prompt_lens}")
        self.codes = torch.zeros(B * model.cfg.n_q * max(max(self.prompt_lens), self.max_new), dtype=torch.int32, device=model.device)
        self.top = list(self.off)                                      # row behind item u's last arrived frame
        self.ended = [False] * B
        self.closed = [False] * B                                      # ended, and stage 1 has passed the end
        self.n2 = [self.E] * B                                         # row item u's samples have reached
        self.primed = False
        # rows of the common time axis: E + max_new. Data row == row, so the convolution's first row is pl0
        self._allocate(B, self.E + self.max_new, self.pl0, self.max_new)

    # ------------------------------------------------------------------ the pieces
    def _item_ptr(self, t: torch.Tensor, u: int, row: int) -> int:
        return t.data_ptr() + 4 * (u * t.stride(0) + row * t.stride(1))

    def _right_edge(self, u: int, upto: int):
        """Item u has ended at row top[u]: behind it `z` holds the layer's own padding — zeros, or the item's reflected rows — whatever
        a batched dequantiser call has written there (the rows [top[u], upto) may hold junk)."""
        z, end = self.z, self.top[u]
        if upto > end:
            z.data[u, end: upto].zero_()
        if self.reflect:
            self.m._call("ssrhip_pad_reflect", self._item_ptr(z.data, u, self.off[u] - self.pl0), 1, end - self.off[u], self.pl0, self.pr0, z.C,
                         z.bstride)

    def _stage1(self):
        a, b = batch_stage1_range(self.n1, self.top, self.ended, self.closed, self.pr0)
        b = min(b, self.rows)
        if b > a:
            # (front: the rows in front of an item's first frame)
            self._stage1_rows(a, b, [(u, min(b, self.off[u])) for u in range(self.B) if a < self.off[u]])
        for u in range(self.B):
            if self.ended[u] and not self.closed[u] and self.top[u] <= b:
                if b > self.top[u]:
                    self.s1.data[u, 1 + self.top[u]: 1 + b].zero_()   # the zero row the last window's transposed convolution reads
                self.closed[u] = True

    def _stage2(self):
        rule = self._window_rule()
        while True:
            wins = [batch_window_item(self.off[u], self.E, self.n2[u], self.top[u], self.n1, self.closed[u], *rule) for u in range(self.B)]
            key, members, alone = batch_window_groups(wins)
            if key is None and not alone:
                return
            for win, item, who in ([(key, None, members)] if key is not None else []) + [(wins[u], u, [u]) for u in alone]:
                self._run_window(win, item, who, self.E)
                for u in who:
                    self.n2[u] = win[1]

    def _dequant(self, n: int, row: int):
        z, cfg = self.z, self.m.cfg
        self.m._call("ssrhip_rvq_decode", self.codes.data_ptr(), self.m.codebooks.data_ptr(), self._item_ptr(z.data, 0, row), self.B, n, z.C,
                     cfg.n_q, cfg.bins, z.bstride)

    def _stage_codes(self, codes: Sequence[torch.Tensor], counts: Sequence[int], n: int, right: bool):
        """The block [B][K][n] the dequantiser reads, from host-checked codes (tests, and the prompts): item u's `counts[u]` columns at
        the left of the block, or at its right; the other columns hold id 0."""
        K, bins = self.m.cfg.n_q, self.m.cfg.bins
        block = np.zeros((self.B, K, n), dtype=np.int32)
        for u, (c, k) in enumerate(zip(codes, counts)):
            if k == 0:
                continue
            c = c.detach().reshape(K, -1).cpu().numpy()
            if c.shape[1] != k:
                raise ValueError(f"item {u}: {k} frames announced, {c.shape[1]} given")
            if c.min() < 0 or c.max() >= bins:
                raise IndexError("index out of range in self")        # what F.embedding raises in the reference (core_vq.py:175)
            block[u, :, (n - k if right else 0): (n if right else k)] = c
        self.codes[: block.size].view(self.B, K, n).copy_(torch.from_numpy(block))

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def push_prompts(self, codes: Sequence[torch.Tensor]) -> None:
        """codes[u]: [K, P_u] (or [1, K, P_u]) — the prompts, range-checked here, once, before the stream's first launch. They run
        through stage 1 (the LSTM state has to pass through them) and are never returned."""
        if self.primed:
            raise RuntimeError("BatchDecodeStream.push_prompts called twice")
        if len(codes) != self.B:
            raise ValueError(f"{self.B} prompts expected, got {len(codes)}")
        p_max = max(self.prompt_lens)
        self._stage_codes(codes, self.prompt_lens, p_max, right=True)
        self.primed = True
        self._dequant(p_max, self.pl0)
        z = self.z
        for u in range(self.B):
            if self.off[u] > self.pl0:
                z.data[u, self.pl0: self.off[u]].zero_()               # id 0 dequantised in front of the item's first frame
            if self.reflect:
                self.m._call("ssrhip_pad_reflect", self._item_ptr(z.data, u, self.off[u] - self.pl0), 1, self.prompt_lens[u], self.pl0, 0, z.C,
                             z.bstride)
            self.top[u] = self.E
        self._stage1()

    @torch.no_grad()
    def advance(self, new_frames: Sequence[int], ended: Sequence[bool], codes: Optional[Sequence[torch.Tensor]] = None,
                flag: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """The next generated frames: new_frames[u] of item u, which has `ended[u]` with them. Lock-step: every item that goes on gets the
        same number of frames, an item that ends here at most that many, an item that had ended none. The frames are in `self.codes`, the
        stream's own int32 buffer, as a [B][K][n] block (n = max(new_frames), item u's in its first new_frames[u] columns) that a producer
        filled on the device (`ssrhip_stream_gather`; `flag`: the device word it sets for an id outside the codebook — read once, after
        everything is enqueued, IndexError before any sample is returned) — or they are given as `codes[u]` [K, new_frames[u]] and checked
        on the host. Returns, per item, the samples that have become final: [1, 1, m * hop] views of item u's row of the one output buffer."""
        if not self.primed:
            raise RuntimeError("BatchDecodeStream.advance before push_prompts")
        B = self.B
        new = [int(v) for v in new_frames]
        if len(new) != B or len(ended) != B:
            raise ValueError(f"{B} items expected")
        n = max(new)
        for u in range(B):
            if self.ended[u] and new[u]:
                raise ValueError(f"item {u} has ended and gets {new[u]} more frames")
            if not self.ended[u] and not ended[u] and new[u] != n:
                raise ValueError(f"lock-step: item {u} goes on with {new[u]} new frames while another item gets {n}")
            if self.top[u] + new[u] > self.rows:
                raise ValueError(f"item {u}: more than max_new_frames = {self.max_new} generated frames")
        a = list(self.n2)
        live_top = [self.top[u] for u in range(B) if not self.ended[u]]
        if n:
            row = live_top[0]
            assert all(t == row for t in live_top)
            if codes is not None:
                self._stage_codes(codes, new, n, right=False)
            self._dequant(n, row)
            for u in range(B):
                if not self.ended[u]:
                    self.top[u] = row + new[u]
                    self.ended[u] = bool(ended[u])
            for u in range(B):
                if self.ended[u] and not self.closed[u]:
                    self._right_edge(u, row + n)
        else:
            for u in range(B):
                if not self.ended[u] and ended[u]:
                    self.ended[u] = True
                    self._right_edge(u, self.top[u])
        self._stage1()
        self._stage2()
        if flag is not None and int(flag.item()):
            raise IndexError("index out of range in self")
        hop, E = self.hop, self.E
        return [self.wav[u: u + 1, :, (a[u] - E) * hop: (self.n2[u] - E) * hop] for u in range(B)]

    @property
    def finished(self) -> bool:
        return all(self.closed) and all(self.n2[u] >= self.top[u] for u in range(self.B))


# ----------------------------------------------------------------------------- streamed watermarked decode of a lock-step batch (DESIGN.md Part I.29)
class RowOp(NamedTuple):
    """One entry of an `ssrhip_stream_rows` table, in FLOATS from the start of its destination / source buffer (the stream adds the
    buffers' addresses): `rows` rows of `width` floats, `dst_ld` / `src_ld` floats apart; mode 0 zeroes, mode 1 copies."""
    dst: int
    src: int
    rows: int
    width: int
    dst_ld: int
    src_ld: int
    mode: int


def rows_front_zero(offs: Sequence[int], a: int, b: int, item_rows: int, C: int) -> List[RowOp]:
    """Zero the rows [a, min(b, off_u)) of every item u of a [B][item_rows][C] buffer: the part of a batched call over the rows [a, b)
    that lies in front of the item's first frame."""
    return [RowOp((u * item_rows + a) * C, 0, min(b, o) - a, C, C, 0, 0) for u, o in enumerate(offs) if a < min(b, o)]


def rows_right_edge(u: int, end: int, pad: int, reflect: bool, item_rows: int, C: int) -> RowOp:
    """Item u has ended at row `end`: the `pad` rows behind it hold the consuming convolution's own padding — zeros, or the item's
    rows mirrored at its last one (row end + i <- row end - 2 - i: a copy that walks its source backwards)."""
    d = (u * item_rows + end) * C
    return RowOp(d, d - 2 * C, pad, C, C, -C, 1) if reflect else RowOp(d, 0, pad, C, C, 0, 0)


def rows_left_edge(u: int, off: int, pad: int, item_rows: int, C: int) -> RowOp:
    """Reflect padding in front of item u's first row `off`: row off - pad + j <- row off + pad - j."""
    return RowOp((u * item_rows + off - pad) * C, (u * item_rows + off + pad) * C, pad, C, C, -C, 1)


def rows_core_copy(pairs: Sequence[Tuple[int, int]], c0: int, c1: int, lo: int, rep: int, C: int, dst_item: int, src_item: int,
                   src_pad: int = 0) -> List[RowOp]:
    """A window's core into a whole-utterance buffer: for (item u, slot j of the window's buffer) in `pairs`, the rows
    [c0 rep, c1 rep) of item u of dst [B][...][C] (`dst_item` floats per item) <- the rows from src_pad + (c0 - lo) rep on of slot j
    (`src_item` floats per slot). The core is contiguous on both sides. Every item in its own slot, in order: ONE op whose "rows"
    are the items."""
    n, d0, s0 = (c1 - c0) * rep * C, c0 * rep * C, (src_pad + (c0 - lo) * rep) * C
    if len(pairs) > 1 and all(u == j == i for i, (u, j) in enumerate(pairs)):
        return [RowOp(d0, s0, len(pairs), n, dst_item, src_item, 1)]
    return [RowOp(u * dst_item + d0, j * src_item + s0, 1, n, dst_item, src_item, 1) for u, j in pairs]


def chain_window_item(off: int, nA: int, top: int, ended: bool, margins: Tuple[int, int], max_window: int):
    """The next skip-encoder chain window of ONE item of a `BatchWMDecodeStream`, in rows -> (c0, c1, lo, hi), ("skip", c1) when the
    whole core lies in front of the item's first frame (nothing to compute), or None (nothing to do yet). off = the item's first row,
    nA = the row its chain has reached, top = the row behind its last arrived frame; an item that has `ended` runs to `top`, a true
    edge, a live one to top less the right margin. A window that would reach in front of `off` is cut there: a true edge too."""
    limit = top if ended else top - margins[1]
    if nA >= limit:
        return None
    c1 = min(nA + max_window, limit)
    if c1 <= off:
        return ("skip", c1)
    c0 = max(nA, off)
    return c0, c1, max(off, c0 - margins[0]), min(top, c1 + margins[1])


class _TMRows(TM):
    """Rows of a larger [B][rows][C] buffer without halo, read in place: the items are `bstride` elements apart."""

    def __init__(self, data: torch.Tensor, bstride: int, device):
        super().__init__(int(data.shape[0]), int(data.shape[1]), int(data.shape[2]), 0, 0, device, data=data, keep_halo=True)
        self._bstride = int(bstride)

    @property
    def bstride(self) -> int:
        return self._bstride


class _RowOpTable:
    """The tables of a stream's `ssrhip_stream_rows` launches: filled on the host (pinned memory), pushed to the device copy on the
    caller's stream without waiting for it, launched. A ring of slots, each with an event that says its push has been read: a slot is
    written again only after that. Created with the stream; nothing is allocated later."""
    SLOTS = 32

    def __init__(self, model: WMEncodecModel):
        self.m = model
        size = _lib.STREAM_ROWS_MAX_OPS * C.sizeof(_lib.RowsOp)
        self.host = torch.zeros(self.SLOTS, size, dtype=torch.uint8).pin_memory()
        self.dev = torch.zeros(self.SLOTS, size, dtype=torch.uint8, device=model.device)
        self.recs = [(_lib.RowsOp * _lib.STREAM_ROWS_MAX_OPS).from_address(self.host[i].data_ptr()) for i in range(self.SLOTS)]
        self.events = [torch.cuda.Event() for _ in range(self.SLOTS)]
        self.used = [False] * self.SLOTS
        self.slot, self.n, self.launches = 0, 0, 0

    @staticmethod
    def _inside(at: int, ld: int, rows: int, width: int, buf: torch.Tensor) -> bool:
        last = (rows - 1) * ld
        return at + min(last, 0) >= 0 and at + max(last, 0) + width <= buf.numel()

    def add(self, ops: Sequence[RowOp], dst: torch.Tensor, src: Optional[torch.Tensor] = None):
        """`ops` with their offsets turned into addresses: dst / src = the (dense) buffers the offsets count from. An op that would
        leave its buffer is an error here, before anything is launched."""
        for op in ops:
            if op.rows <= 0 or op.width <= 0:
                continue
            if not self._inside(op.dst, op.dst_ld, op.rows, op.width, dst) or (op.mode and not self._inside(op.src, op.src_ld, op.rows, op.width, src)):
                raise RuntimeError(f"BatchWMDecodeStream: the row operation {tuple(op)} leaves its buffer")
            if self.n == _lib.STREAM_ROWS_MAX_OPS:
                self.launch()
            if self.n == 0 and self.used[self.slot]:
                self.events[self.slot].synchronize()                   # the slot's last push has left the host
            r = self.recs[self.slot][self.n]
            r.dst, r.src = dst.data_ptr() + 4 * op.dst, (src.data_ptr() + 4 * op.src if op.mode else 0)
            r.dst_ld, r.src_ld, r.rows, r.width, r.mode, r.reserved_ = op.dst_ld, op.src_ld, op.rows, op.width, op.mode, 0
            self.n += 1

    def launch(self):
        """One launch for everything added since the last one (none when nothing was)."""
        if self.n == 0:
            return
        i, size = self.slot, self.n * C.sizeof(_lib.RowsOp)
        self.dev[i, :size].copy_(self.host[i, :size], non_blocking=True)
        self.events[i].record(torch.cuda.current_stream(self.m.device))
        self.used[i] = True
        self.m._call("ssrhip_stream_rows", self.host[i].data_ptr(), self.dev[i].data_ptr(), self.n)
        self.slot, self.n = (i + 1) % self.SLOTS, 0
        self.launches += 1


class BatchWMDecodeStream(BatchDecodeStream):
    """`WMEncodecModel.wmdecode_stream_batch`: the watermarked decode (`wmdecode(..., with_mark=False)`) of B utterances that are
    generated in lock-step as zero-shot TTS — `WMDecodeStream`'s seven steps on `BatchDecodeStream`'s aligned axis, each step ONE dense
    batched call of the kernel `WMDecodeStream` calls for it.

    The axis (`batch_align_plan` with F = the larger left padding of the two frame-rate convolutions in front): item u's frame t is
    row off_u + t of every frame-rate buffer [B][rows][C]; the prompts end at row E, generated frame j of every item is row E + j. The
    kept-audio track holds item u's original audio under its prompt and silence from row E on; the label is 0 below E and 1 from E on.

    Per `advance`: the dequantiser into `q`; chain windows (`chain_window_item`, grouped by `batch_window_groups`) whose cores go into
    the whole-utterance taps and `p`; the skip encoder's LSTM over a common row range (`batch_stage1_range`) into `u`; tap 4 and `z`
    (two GEMMs with batch = B); the decoder's first convolution and LSTM; stage-2 windows with `_concat_proj` reading the stored taps
    in place. What is per item — the zero rows in front of a short prompt (`p`, `y0` and all four `gin`s: with biases in the skip
    encoder the chain over a zero track is not zero), an ended item's right edges in `u`, `z` and `s1`, the reflected rows, the cores
    of the taps and of the output — is a table of row operations executed by ONE `ssrhip_stream_rows` launch per stage.

    An item that ends runs its last chain windows alone (its end is a true edge of the track); behind its end `u` and `z` get the
    consuming convolution's own padding after every batched call that wrote there, until that convolution has passed the end; its last
    stage-2 windows run alone. Later batched calls write junk behind a finished item's end, which nothing reads. B stays constant.

    Everything runs on the caller's stream and is allocated here: create the stream before the decode engine's first launch."""

    def __init__(self, model: WMEncodecModel, prompt_lens: Sequence[int], max_new_frames: int, max_window: int):
        if max_new_frames < 1 or max_window < 1:
            raise ValueError("wmdecode_stream_batch needs max_new_frames >= 1 and max_window >= 1")
        _wm_stream_cut(self, model, "wmdecode_stream_batch", int(max_window))
        cfg, dev, c = model.cfg, model.device, self.sk_conv
        self.max_new = int(max_new_frames)
        self.front = max(c.pl, self.pl0)
        plan = batch_align_plan(prompt_lens, self.front)
        self.prompt_lens = [int(p) for p in prompt_lens]
        self.off, self.E = plan["off"], plan["E"]
        B = len(self.off)
        need = self.smargins[1] + max(c.pl, c.pr) + max(self.pl0, self.pr0)
        if self.reflect and min(self.prompt_lens) <= need:
            raise ValueError(f"wmdecode_stream_batch: with reflect padding every prompt must be longer than the chain's right margin plus "
                             f"the paddings of the two frame-rate convolutions ({need} frames), got {self.prompt_lens}")
        rows = self.E + self.max_new
        hop, D, Cs = self.hop, cfg.dimension, self.sk_lstm.C
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.codes = torch.zeros(B * cfg.n_q * max(max(self.prompt_lens), self.max_new), **i32)
        self.lab = torch.zeros(B, rows, **i32)
        self.lab[:, self.E:] = 1
        self.track = torch.zeros(B, rows * hop, **f32)
        self.q = torch.zeros(B, rows, D, **f32)                        # the dequantised codes
        self.taps = [torch.zeros(B, rows * rep, part[-1][2][1].Cout, **f32) for part, rep in zip(self.ch_cuts, self.reps)]
        self.p = torch.zeros(B, rows, Cs, **f32)                       # the chain's frame-rate rows: what the skip encoder's LSTM reads
        nl = len(self.sk_lstm.layers)
        self.sk_gins = [torch.zeros(B, rows, 4 * Cs, **f32) for _ in range(nl)]
        self.sk_hbufs = [torch.zeros(2, (B + 15) // 16 * 16, Cs, **f32) for _ in range(nl)]
        self.sk_cbufs = [torch.zeros(B, Cs, **f32) for _ in range(nl)]
        self.sk_mids = [torch.zeros(B, rows, Cs, **f32) for _ in range(nl - 1)]
        split = model._lstm_use_split(self.sk_lstm, B)
        self.sk_hsplits = [torch.zeros(2 * ((B + 63) // 64) * 64 * Cs * 3, dtype=torch.int16, device=dev)
                           if (split and self.sk_lstm.split[l] is not None) else None for l in range(nl)]
        # LSTM + skip, what `sk_conv` reads: data row == row, the rows in front of an item's first frame are its left halo
        self.u = TM(B, rows - c.pl, Cs, c.pl, c.pr, dev, data=torch.zeros(B, rows + c.pr, Cs, **f32))
        self.u.elu = bool(model.elu_on_store and c.act_in)
        self.tap4 = torch.zeros(B, rows, c.Cout, **f32)
        self.ops = _RowOpTable(model)
        self.top = list(self.off)                                      # row behind item u's last arrived frame
        self.ended = [False] * B
        self.nA = [self.front] * B                                     # row item u's chain has reached
        self.nL = 0                                                    # row the skip encoder's LSTM has reached
        self.nC = self.front                                           # row tap 4 and `z` have reached
        self.closedL, self.closedC, self.closed = [False] * B, [False] * B, [False] * B     # ended, and that stage has passed the end
        self.n2 = [self.E] * B
        self.primed = False
        self.chain_windows = self.chain_windows_batched = 0
        # the chain's window buffers, of all B items at once and of one item, each by a dry pass over its largest window; those of
        # stage 2 likewise, in `_allocate`
        self.B, self.rows = B, rows
        self.pool_cb, self.pool_c1 = (_WindowPool() if B > 1 else None), _WindowPool()
        self.tap_elu = [False] * 3
        real, model.lib = model.lib, _NoLaunch()
        try:
            n = min(rows, self.max_window + self.smargins[0] + self.smargins[1])
            for item, pool in ((None, self.pool_cb), (0, self.pool_c1)):
                if pool is not None:
                    taps, _ = self._chain_pass(0, n, item)
                    self.tap_elu = [t.elu for t in taps]
                    pool.frozen = True
        finally:
            model.lib = real
        self._allocate(B, rows, self.pl0, self.max_new)

    @property
    def tap_bytes(self) -> int:
        """Bytes of the three whole-utterance tap buffers, all items"""
        return sum(t.numel() * 4 for t in self.taps)

    # ------------------------------------------------------------------ the pieces
    def _chain_pass(self, lo: int, hi: int, item: Optional[int]) -> Tuple[List[TM], TM]:
        """`WMDecodeStream._chain_pass` over the track's rows [lo, hi) of every item (`item` None) or of one."""
        m, hop = self.m, self.hop
        who = slice(None) if item is None else slice(item, item + 1)
        with m._stream_pass(self.pool_cb if item is None else self.pool_c1, False):
            x = m._input_tm(self.track[who, lo * hop: hi * hop].unsqueeze(1), self.ch_head[0])
            z = m._run(self.ch_head, x, after=self.ch_cuts[0][0])
            taps = []
            for i, part in enumerate(self.ch_cuts):
                z = m._run(part, z, after=(self.ch_cuts[i + 1][0] if i + 1 < len(self.ch_cuts) else self.ch_last))
                taps.append(z)
            return taps, m._run([self.ch_last], z, after=self.sk_lstm_node)

    def _chain(self):
        """Chain windows as far as every item allows: the items whose windows agree in ONE batched pass, the others alone (a window cut
        at an item's first frame, an ended item's last windows)."""
        B, ops = self.B, self.ops
        while True:
            wins = [chain_window_item(self.off[u], self.nA[u], self.top[u], self.ended[u], self.smargins, self.max_window) for u in range(B)]
            skipped = False
            for u, w in enumerate(wins):
                if w is not None and w[0] == "skip":                  # the whole core lies in front of the item's first frame
                    self.nA[u], wins[u], skipped = w[1], None, True
            key, members, alone = batch_window_groups(wins)
            if key is None and not alone:
                if skipped:
                    continue
                return
            for win, item, who in ([(key, None, members)] if key is not None else []) + [(wins[u], u, [u]) for u in alone]:
                c0, c1, lo, hi = win
                taps, rows = self._chain_pass(lo, hi, item)
                pairs = [(u, u if item is None else 0) for u in who]
                for buf, t, rep in zip(self.taps + [self.p], taps + [rows], self.reps + [1]):
                    ops.add(rows_core_copy(pairs, c0, c1, lo, rep, t.C, buf.stride(0), t.bstride, t.padL), buf, t.data)
                ops.launch()                                           # before the next window takes the pool's buffers
                for u in who:
                    self.nA[u] = c1
                self.chain_windows += 1
                self.chain_windows_batched += int(item is None)

    def _lstm_rows(self, L: _Lstm, src: torch.Tensor, gins, hbufs, cbufs, hsplits, mids, out_ptr: int, out_bs: int, out_elu: bool, a: int, b: int):
        """The rows [a, b) of every item through the layers of one LSTM (+ skip): `_StreamCore._stage1_rows`' loop, with the rows in front
        of an item's first frame — the skip input `src` and every layer's `gin` — zeroed by one row-op launch ahead of each step call,
        so that the item's state stays exactly zero (`BatchDecodeStream`)."""
        m, B, rows, ops = self.m, self.B, self.rows, self.ops
        bs, nl = rows * L.C, len(L.layers)
        for l in range(nl):
            x, last = (src if l == 0 else mids[l - 1]), l == nl - 1
            m._lstm_in_gemm(L, l, x.data_ptr(), bs, gins[l], B, rows, a, b)
            if l == 0:
                ops.add(rows_front_zero(self.off, a, b, rows, L.C), src)
            ops.add(rows_front_zero(self.off, a, b, rows, 4 * L.C), gins[l])
            ops.launch()
            m._lstm_steps(L, l, gins[l], hbufs[l], cbufs[l], hsplits[l], (out_ptr if last else mids[l].data_ptr()), (out_bs if last else bs),
                          (src.data_ptr() if last else 0), bs, B, rows, a, b, out_elu and last)

    def _edges(self, buf: TM, a: int, b: int, closed_in: Sequence[bool], closed_out: Sequence[bool], zero_front: bool):
        """After a batched call has written the rows [a, b) of `buf` (data row == row; halo = the consuming convolution's paddings): an
        item whose first frame lies in [a, b) gets that convolution's padding in front of it (zeros — `zero_front`, where the producer
        does not leave them — or its reflected rows), an item that has ended (`closed_in`: the producer has passed its end) and whose
        end the consumer has not passed (`closed_out`) gets it behind its end. One launch."""
        ops, rows_b, Cc = self.ops, buf.rows, buf.C
        for u in range(self.B):
            off, end = self.off[u], self.top[u]
            if self.reflect and a <= off < b:
                assert b > off + buf.padL, (u, a, b, off)             # (the prompt lengths the constructor accepts see to it)
                ops.add([rows_left_edge(u, off, buf.padL, rows_b, Cc)], buf.data, buf.data)
            if closed_in[u] and not closed_out[u]:
                ops.add([rows_right_edge(u, end, buf.padR, self.reflect, rows_b, Cc)], buf.data, buf.data)
        if zero_front and not self.reflect:
            ops.add(rows_front_zero(self.off, a, b, rows_b, Cc), buf.data)
        ops.launch()

    def _skip_lstm(self):
        done = [self.ended[u] and self.nA[u] >= self.top[u] for u in range(self.B)]
        a, b = batch_stage1_range(self.nL, [self.top[u] if done[u] else self.nA[u] for u in range(self.B)], done, self.closedL, 0)
        b = min(b, self.rows)
        if b > a:
            u_ = self.u
            self._lstm_rows(self.sk_lstm, self.p, self.sk_gins, self.sk_hbufs, self.sk_cbufs, self.sk_hsplits, self.sk_mids, u_.base, u_.bstride,
                            u_.elu, a, b)
            self.nL = b
        for u in range(self.B):
            self.closedL[u] = self.closedL[u] or (done[u] and self.top[u] <= self.nL)
        self._edges(self.u, a, b, self.closedL, self.closedC, False)  # (in front the LSTM has written the zeros its zero state gives)

    def _decoder_input(self):
        """Tap 4 and `z` over a common row range: `WMDecodeStream._decoder_input` with batch = B."""
        m, u_, c, z, B, rows = self.m, self.u, self.sk_conv, self.z, self.B, self.rows
        a, b = batch_stage1_range(self.nC, [self.top[u] if self.closedL[u] else self.nL for u in range(B)], self.closedL, self.closedC, c.pr)
        b = min(b, rows)
        if b > a:
            m._gemm(u_.base + 4 * (a - c.pl) * u_.C, c.W, c.b, self.tap4.data_ptr() + 4 * a * c.Cout, b - a, c.Cout, c.k * c.Cin, c.s * c.Cin, c.Cout,
                    act_in=m._act_in(bool(c.act_in), u_), batch=B, sA=u_.bstride, sC=rows * c.Cout)
            pj, (Wa, cls) = m.wm_proj[0], m.wm_cls[0]
            Cs, D = int(Wa.shape[1]), z.C
            assert Cs == c.Cout and pj.Cout == D
            m._gemm(self.tap4.data_ptr() + 4 * a * Cs, Wa, pj.b, z.base + 4 * a * D, b - a, D, Cs, Cs, D, act_in=_lib.ACT_ELU,
                    R=self.q.data_ptr() + 4 * a * D, ldr=D, batch=B, sA=rows * Cs, sC=z.bstride, sR=rows * D, rowcls=(cls, self.lab[:, a:b], 1))
            self.nC = b
        for u in range(B):
            self.closedC[u] = self.closedC[u] or (self.closedL[u] and self.top[u] <= self.nC)
        self._edges(z, a, b, self.closedC, self.closed, True)

    def _stage1(self):
        B, s1 = self.B, self.s1
        a, b = batch_stage1_range(self.n1, [self.top[u] if self.closedC[u] else self.nC for u in range(B)], self.closedC, self.closed, self.pr0)
        b = min(b, self.rows)
        if b > a:
            m, z, c0 = self.m, self.z, self.conv0
            ca = max(a, self.conv_row0)
            if b > ca:
                m._gemm(z.base + 4 * (ca - self.conv_row0) * z.C, c0.W, c0.b, self.y0.data_ptr() + 4 * ca * c0.Cout, b - ca, c0.Cout, c0.k * c0.Cin,
                        c0.s * c0.Cin, c0.Cout, act_in=m._act_in(bool(c0.act_in), z), batch=B, sA=z.bstride, sC=self.rows * c0.Cout)
            self._lstm_rows(self.lstm, self.y0, self.gins, self.hbufs, self.cbufs, self.hsplits, self.mids, s1.interior, self._s1_bs, s1.elu, a, b)
            self.n1 = b
        for u in range(B):
            if self.closedC[u] and not self.closed[u] and self.top[u] <= self.n1:
                # the zero row the last window's transposed convolution reads
                self.ops.add([RowOp((u * s1.rows + 1 + self.top[u]) * s1.C, 0, self.n1 - self.top[u], s1.C, s1.C, 0, 0)], s1.data)
                self.closed[u] = True
        self.ops.launch()

    def _tail_pass(self, lo: int, hi: int, item: Optional[int], few: bool = False) -> TM:
        """`WMDecodeStream._tail_pass` over the rows [lo, hi) of every item (`item` None) or of one: the stored taps' rows of the window
        and the labels from the window's first row on, read in place."""
        m, s1 = self.m, self.s1
        who = slice(None) if item is None else slice(item, item + 1)
        x = _TMView(s1.data[who, lo: hi + 2], hi - lo, s1.bstride, m.device)
        x.elu = s1.elu
        with m._stream_pass(self.pool_b if item is None else self.pool_1, few):
            y = m._run(self.dn[0], x, after=None)
            for j in (1, 2, 3):
                tap, rep = self.taps[3 - j], self.reps[3 - j]
                skip = _TMRows(tap[who, lo * rep: hi * rep], tap.stride(0), m.device)
                skip.elu = self.tap_elu[3 - j]
                y = m._run(self.dn[j], m._concat_proj(j, skip, self.lab[who, lo:hi], rep, y, self.dn[j][0]), after=None)
            return y

    def _run_window(self, win: tuple, item: Optional[int], who: Sequence[int], row0: int):
        """`_StreamCore._run_window` with the cores copied by one row-op launch."""
        (c0, c1, lo, hi, few), hop = win, self.hop
        y = self._tail_pass(lo, hi, item, few)
        assert y.C == 1 and y.padL == 0 and y.T == (hi - lo) * hop
        self.ops.add(rows_core_copy([(u, u if item is None else 0) for u in who], c0 - row0, c1 - row0, lo - row0, hop, 1, self.wav.stride(0),
                                    y.bstride), self.wav, y.data)
        self.ops.launch()
        self.windows += 1
        self.windows_batched += int(item is None)

    def _advance_all(self):
        self._chain()
        self._skip_lstm()
        self._decoder_input()
        self._stage1()
        self._stage2()

    def _dequant(self, n: int, row: int):
        q, cfg = self.q, self.m.cfg
        self.m._call("ssrhip_rvq_decode", self.codes.data_ptr(), self.m.codebooks.data_ptr(), self._item_ptr(q, 0, row), self.B, n, q.shape[2],
                     cfg.n_q, cfg.bins, q.stride(0))

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def push_prompts(self, codes: Sequence[torch.Tensor], audio: Sequence[torch.Tensor]) -> None:
        """codes[u]: [K, P_u] (or [1, K, P_u]), range-checked here; audio[u]: the ORIGINAL audio under item u's prompt, at most
        P_u * hop samples (any shape; a shorter one is zero-extended to whole frames, as the one-pass call extends it). The prompts pass
        through the skip-encoder chain, both LSTMs and the decoder's first convolution and are never returned."""
        if self.primed:
            raise RuntimeError("BatchWMDecodeStream.push_prompts called twice")
        if len(codes) != self.B or len(audio) != self.B:
            raise ValueError(f"{self.B} prompts and {self.B} audio tracks expected, got {len(codes)} / {len(audio)}")
        hop = self.hop
        for u, w in enumerate(audio):
            if w.numel() > self.prompt_lens[u] * hop:
                raise ValueError(f"item {u}: {w.numel()} samples under a prompt of {self.prompt_lens[u]} frames ({self.prompt_lens[u] * hop} samples)")
        p_max = max(self.prompt_lens)
        self._stage_codes(codes, self.prompt_lens, p_max, right=True)
        self.primed = True
        for u, w in enumerate(audio):
            self.track[u, self.off[u] * hop: self.off[u] * hop + w.numel()].copy_(w.reshape(-1))
        self._dequant(p_max, self.front)
        self.top = [self.E] * self.B
        self._advance_all()

    @torch.no_grad()
    def advance(self, new_frames: Sequence[int], ended: Sequence[bool], codes: Optional[Sequence[torch.Tensor]] = None,
                flag: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """`BatchDecodeStream.advance`: the next generated frames (silence in the kept-audio track, label 1) -> per item the watermarked
        samples that have become final, [1, 1, m * hop] views of item u's row of the one output buffer."""
        if not self.primed:
            raise RuntimeError("BatchWMDecodeStream.advance before push_prompts")
        B = self.B
        new = [int(v) for v in new_frames]
        if len(new) != B or len(ended) != B:
            raise ValueError(f"{B} items expected")
        n = max(new)
        for u in range(B):
            if self.ended[u] and new[u]:
                raise ValueError(f"item {u} has ended and gets {new[u]} more frames")
            if not self.ended[u] and not ended[u] and new[u] != n:
                raise ValueError(f"lock-step: item {u} goes on with {new[u]} new frames while another item gets {n}")
            if self.top[u] + new[u] > self.rows:
                raise ValueError(f"item {u}: more than max_new_frames = {self.max_new} generated frames")
        a = list(self.n2)
        live_top = [self.top[u] for u in range(B) if not self.ended[u]]
        if n:
            row = live_top[0]
            assert all(t == row for t in live_top)
            if codes is not None:
                self._stage_codes(codes, new, n, right=False)
            self._dequant(n, row)
        for u in range(B):
            if not self.ended[u]:
                self.top[u] += new[u]
                self.ended[u] = bool(ended[u])
        self._advance_all()
        if flag is not None and int(flag.item()):
            raise IndexError("index out of range in self")
        hop, E = self.hop, self.E
        return [self.wav[u: u + 1, :, (a[u] - E) * hop: (self.n2[u] - E) * hop] for u in range(B)]
