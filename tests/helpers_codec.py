"""Shared by the GPU codec tests: the reference's own top-1 / top-2 margin of every RVQ decision (fp32 near-ties), and the plain
float64 references of the operations in csrc/codec.hip that tests/test_gpu_codec_kernels.py compares the kernels with. The
references are pinned to oracle/codec.py by tests/test_codec_kernel_refs.py (no GPU), so that a kernel test cannot be wrong
together with its reference. Layouts are the kernels': activations time-major ([B][rows][C], C contiguous)."""
import math

import torch
import torch.nn.functional as F


def code_margins(sd, cfg, emb, codes):
    """top-1 minus top-2 score of every RVQ decision along the reference's own residual path."""
    B, D, T = emb.shape
    res = emb.clone()
    out = torch.zeros(B, cfg.n_q, T)
    for q in range(cfg.n_q):
        E = sd[f"quantizer.vq.layers.{q}._codebook.embed"]
        x = res.permute(0, 2, 1).reshape(-1, D)
        dist = -(x.pow(2).sum(1, keepdim=True) - 2 * x @ E.t() + E.t().pow(2).sum(0, keepdim=True))
        top2 = dist.topk(2, dim=-1).values
        out[:, q] = (top2[:, 0] - top2[:, 1]).view(B, T)
        res = res - torch.nn.functional.embedding(codes[:, q], E).permute(0, 2, 1)
    return out


# ----------------------------------------------------------------------------------------------- convolutions
def conv_cin1_ref(x, w, bias, T_out, stride):
    """ssrhip_conv_cin1: x [B][L] (one input channel, L >= (T_out - 1) * stride + k), w [C_out][k] -> float64 [B][T_out][C_out]."""
    k = w.shape[1]
    L = (T_out - 1) * stride + k
    y = F.conv1d(x[:, None, :L].double(), w.double()[:, None, :], bias.double(), stride=stride)
    return y.permute(0, 2, 1).contiguous()


def conv_few_out_ref(x, w, bias, act_elu):
    """ssrhip_conv_few_out: x [B][T_out + k - 1][C_in] time-major, w [C_out][k][C_in] (the GEMM layout of the layer), the ELU
    applied to the input -> float64 [B][T_out][C_out]."""
    xin = x.double()
    if act_elu:
        xin = F.elu(xin)
    y = F.conv1d(xin.permute(0, 2, 1), w.double().permute(0, 2, 1), bias.double())
    return y.permute(0, 2, 1).contiguous()


# ----------------------------------------------------------------------------------------------- padding
def pad1d_ref(x, pl, pr, reflect):
    """The reference's pad1d on the LAST axis: zeros, or reflect with the small-input rule (an input no longer than the larger pad
    is zero-extended by max_pad - n + 1, reflected, and the extension dropped again)."""
    if not reflect:
        return F.pad(x, (pl, pr))
    n = x.shape[-1]
    max_pad = max(pl, pr)
    extra = max_pad - n + 1 if n <= max_pad else 0
    if extra:
        x = F.pad(x, (0, extra))
    y = F.pad(x, (pl, pr), mode="reflect")
    return y[..., : y.shape[-1] - extra]


def pad_rows_ref(x, pl, pr, reflect):
    """The same for one time-major item x [n][C] -> [pl + n + pr][C] (n may be 0)."""
    return pad1d_ref(x.t().unsqueeze(0), pl, pr, reflect)[0].t().contiguous()


# ----------------------------------------------------------------------------------------------- RVQ
RVQ_TS = (1, 15, 16, 17, 38)                 # around the matrix-core kernel's 16-frame tile
RVQ_B = 3
RVQ_MFMA_SHAPES = [(D, bins, n_q) for D in (32, 64, 128, 256) for bins in (64, 1024, 2048) for n_q in (1, 8)]
RVQ_SCALAR_ONLY_SHAPES = [(D, bins, n_q) for (D, bins) in ((20, 50), (64, 48), (128, 2048)) for n_q in (1, 8)]
RVQ_MIN_KEPT = 0.90


def rvq_case(D, bins, n_q, T, B=RVQ_B):
    """Fixed-seed inputs of one RVQ case: unit-variance frames [B][T][D], codebooks [n_q][bins][D] with stage q scaled by 0.7^q
    (later residuals stay comparable with their codebook), and |e|^2 as the product computes it."""
    g = torch.Generator().manual_seed(7919 * D + 31 * bins + 1000003 * n_q + T)
    emb = torch.randn(B, T, D, generator=g)
    cb = torch.randn(n_q, bins, D, generator=g) * (0.7 ** torch.arange(n_q, dtype=torch.float32)).view(n_q, 1, 1)
    return emb, cb, cb.pow(2).sum(-1)


def rvq_encode_ref(emb, cb):
    """float64 nearest-row search in the kernels' stated form score = -(|x|^2 - 2 x.e + |e|^2), first index on a tie, along its own
    residual path. emb [B][T][D], cb [n_q][bins][D] -> (codes int64 [B][n_q][T], margin [B][n_q][T] = top-1 minus top-2 score,
    err = the largest |fp32 score - float64 score| over the case, the fp32 scores being the same expression in plain fp32 torch)."""
    B, T, D = emb.shape
    n_q, bins, _ = cb.shape
    res = emb.double().reshape(-1, D)
    codes, margins, err = [], [], 0.0
    for q in range(n_q):
        E = cb[q].double()
        score = -(res.pow(2).sum(1, keepdim=True) - 2 * res @ E.t() + E.pow(2).sum(1)[None])
        r32, E32 = res.float(), cb[q]
        score32 = -(r32.pow(2).sum(1, keepdim=True) - 2 * r32 @ E32.t() + E32.pow(2).sum(1)[None])
        err = max(err, float((score32.double() - score).abs().max()))
        idx = score.max(dim=-1).indices
        if bins > 1:
            top2 = score.topk(2, dim=-1).values
            margins.append((top2[:, 0] - top2[:, 1]).view(B, T))
        else:
            margins.append(torch.full((B, T), float("inf"), dtype=torch.float64))
        codes.append(idx.view(B, T))
        res = res - E[idx]
    return torch.stack(codes, 1), torch.stack(margins, 1), err


def rvq_kept_frames(margins, err):
    """Frames [B][T] on which the float64 reference alone says every stage's decision is safe in fp32: the smallest margin over the
    stages is at least 8 x the fp32 score error of the case."""
    return margins.min(dim=1).values >= 8.0 * err


def rvq_decode_ref(codes, cb):
    """The dequantiser's fp32 sum in its documented order 0.0 + q0 + q1 + ...: codes [B][n_q][T], cb [n_q][bins][D] -> fp32 [B][T][D]."""
    out = torch.zeros(codes.shape[0], codes.shape[2], cb.shape[2], dtype=torch.float32)
    for q in range(codes.shape[1]):
        out = out + cb[q][codes[:, q]]
    return out


# ----------------------------------------------------------------------------------------------- LSTM
def lstm_ref(gin, whh, skip=None, out_elu=False):
    """float64 torch.nn.LSTM cell over time (gates i f g o; h_0 = c_0 = 0): gin [B][T][4C] holds W_ih x_t + b_ih + b_hh, whh [4C][C].
    Returns [B][T][C]: h_t, plus skip[:, t] if given, through ELU if `out_elu` (the layer's store epilogue)."""
    B, T, C4 = gin.shape
    Cc = C4 // 4
    wt = whh.double().t().contiguous()
    h, c = torch.zeros(B, Cc, dtype=torch.float64), torch.zeros(B, Cc, dtype=torch.float64)
    want = []
    for t in range(T):
        gt = gin[:, t].double() + h @ wt
        i, f, gg, o = gt[:, :Cc], gt[:, Cc:2 * Cc], gt[:, 2 * Cc:3 * Cc], gt[:, 3 * Cc:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        y = h + skip[:, t].double() if skip is not None else h
        want.append(F.elu(y) if out_elu else y)
    return torch.stack(want, 1)


def pack_whh(whh):
    """ssrhip_lstm_args.w_packed: W_hh [4C][C] as 16 x 16 blocks in the order the matrix-core lanes read them:
    [C/4 unit groups][C/16 k-steps][4 k-slots][4 units][4 gates][4 floats]."""
    Cc = whh.shape[1]
    return whh.view(4, Cc // 4, 4, Cc // 16, 4, 4).permute(1, 3, 4, 2, 0, 5).contiguous()


def lstm_weights(Cc, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4 * Cc, Cc, generator=g) / math.sqrt(Cc)
