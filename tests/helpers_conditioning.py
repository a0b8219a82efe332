"""Ill-conditioned inputs and fp64 references for the two pieces of arithmetic every decode and prefill path repeats by hand: the
LayerNorm prologue (two-pass statistics per slice, merged exactly) and the split-KV softmax merge / online-softmax rescale.
No GPU here: tests/test_conditioning_inputs.py shows on the CPU that these inputs tell a right form from a wrong one,
tests/test_gpu_conditioning.py feeds them to the kernels.

The tolerance rule, used everywhere: tol = max(floor, M * err_ref32), where err_ref32 = max |fp32 torch CPU - fp64| of the same
operation on the same inputs (the reference's own error, never the kernel's), floor is the project's bound for that kernel family
(3e-5 GEMV, 2e-5 attention) and M is the one constant below (profiles/numerics_conditioning.md has the measured ratios behind it)."""
import math

import torch
import torch.nn.functional as F

PAGE = 128
FLOOR_GEMV = 3e-5
FLOOR_ATTN = 2e-5
M = 32                       # smallest power of two >= 2 x the largest err_kernel / err_ref32 measured on the MI355X (8.2, one launch: the
#                              folded row-per-wave LayerNorm on one `offset` row, where torch's own error came out 5x below its usual
#                              size; the next largest are 5.0, attention with both errors under the floor, and 3.1 —
#                              profiles/numerics_conditioning.md explains the 8.2 from the order of the sums)
LN_EPS = 1e-5

LN_CASES = ("offset", "step", "outlier", "tiny", "const")
ML_CASES = ("wide", "ascending", "descending", "late_peak", "two_peaks")
LOGIT_CASES = ("wide", "ascending", "late_peak", "early_peak", "two_peaks")


def tol(floor, err_ref32, m=None):
    return max(floor, (M if m is None else m) * err_ref32)


def max_err(got, want64):
    """max |got - want| in fp64; a non-finite entry in `got` is an infinite error (so a NaN never passes a `<=`)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - want64).abs().max())


# ---------------------------------------------------------------------------------------------- LayerNorm rows
def ln_rows(B, K, seed):
    """name -> [B, K] fp32 rows. `outlier` is left out for K <= 8 (feature 7 would be most of the row)."""
    g = torch.Generator().manual_seed(seed)
    z = lambda: torch.randn(B, K, generator=g)
    rows = {"offset": 50.0 + 0.05 * z()}
    step = 0.05 * z()
    step[:, :K // 3] += 30.0
    step[:, K // 3:] -= 10.0
    rows["step"] = step
    if K > 8:
        out = z()
        out[:, 7] = 3000.0
        rows["outlier"] = out
    rows["tiny"] = 1e-4 * z()
    rows["const"] = torch.full((B, K), 3.25)
    return {k: v.contiguous() for k, v in rows.items()}


def act_fn(y, act):
    return F.relu(y) if act == 1 else (F.gelu(y) if act == 2 else y)


def ln_normalize(x, eps=LN_EPS, form="two_pass", slices=4):
    """x' = (x - mean) * rstd in x's dtype. The wrong forms are the regressions the new inputs must expose:
    one_pass      var = E[x^2] - E[x]^2
    within_slice  the slice merge without its between-slice term: var = sum_s M2_s / K
    eps_outside   rstd = 1 / (sqrt(var) + eps)"""
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if form == "one_pass":
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    elif form == "within_slice":
        xs = x.view(*x.shape[:-1], slices, K // slices)
        ms = xs.mean(-1, keepdim=True)
        var = ((xs - ms) ** 2).sum((-1, -2)).unsqueeze(-1) / K
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var.sqrt() + eps) if form == "eps_outside" else 1.0 / (var + eps).sqrt()
    return (x - mean) * rstd


def ln_linear_ref(x, W, bias, act=0, y0=None, ln_w=None, ln_b=None, eps=LN_EPS, dtype=torch.float64, form="two_pass"):
    """LN -> linear -> act -> (+ y0) in `dtype`. W [N, K] or grouped [G, N, K] with x [B, G, K]."""
    x, W, bias = x.to(dtype), W.to(dtype), bias.to(dtype)
    if form == "two_pass" and dtype == torch.float32:
        xn = F.layer_norm(x, (x.shape[-1],), None, None, eps)          # torch's own fp32 LayerNorm is the fp32 reference
    else:
        xn = ln_normalize(x, eps, form)
    if ln_w is not None:
        xn = xn * ln_w.to(dtype) + ln_b.to(dtype)
    y = act_fn(F.linear(xn, W, bias), act)
    return y if y0 is None else y0.to(dtype) + y


def layernorm_ref(x, w, b, eps=LN_EPS, dtype=torch.float64):
    x = x.to(dtype)
    xn = F.layer_norm(x, (x.shape[-1],), None, None, eps) if dtype == torch.float32 else ln_normalize(x, eps)
    return xn * w.to(dtype) + b.to(dtype)


# ---------------------------------------------------------------------------------------------- split-KV merge partials
def n_pages(length):
    return (length + PAGE - 1) // PAGE


def ml_cases(B, H, MS, lens, seed):
    """name -> part_ml [B, H, MS, 2] fp32 ((m, l) per page), l in [1, 128] (a real page's l is >= 1: its max key contributes exp(0)),
    NaN on the pages beyond a row's length."""
    g = torch.Generator().manual_seed(seed)
    page = torch.arange(MS, dtype=torch.float32).expand(B, H, MS)
    last = torch.tensor([n_pages(v) - 1 for v in lens])
    m = {"wide": 60.0 * torch.randn(B, H, MS, generator=g), "ascending": 40.0 * page, "descending": -40.0 * page,
         "late_peak": torch.zeros(B, H, MS), "two_peaks": torch.zeros(B, H, MS)}
    for b in range(B):
        m["late_peak"][b, :, last[b]] = 150.0
        m["two_peaks"][b, :, last[b]] = 99.5
        m["two_peaks"][b, :, 0] = 100.0                                 # a one-page row keeps the 100
    out = {}
    for name in ML_CASES:
        l_ = 1.0 + 127.0 * torch.rand(B, H, MS, generator=g)
        ml = torch.stack([m[name].clone(), l_], dim=-1).contiguous()
        for b in range(B):
            ml[b, :, last[b] + 1:] = float("nan")
        out[name] = ml
    return out


def merge_ref(part_o, part_ml, lens, dtype=torch.float64, subtract_max=True):
    """[B, H*hd]: sum_p w_p * o_p with w = e / sum(e * l), e = exp(m - max m), over each row's live pages.
    subtract_max=False is the wrong form (e = exp(m))."""
    B, H, MS, hd = part_o.shape
    out = torch.zeros(B, H * hd, dtype=dtype)
    for b in range(B):
        n = n_pages(lens[b])
        m, l_ = part_ml[b, :, :n, 0].to(dtype), part_ml[b, :, :n, 1].to(dtype)
        e = torch.exp(m - m.max(dim=1, keepdim=True).values) if subtract_max else torch.exp(m)
        w = e / (e * l_).sum(dim=1, keepdim=True)
        out[b] = (w.unsqueeze(-1) * part_o[b, :, :n].to(dtype)).sum(dim=1).reshape(-1)
    return out


def merge_part_o(B, H, MS, hd, lens, seed):
    g = torch.Generator().manual_seed(seed)
    part_o = torch.randn(B, H, MS, hd, generator=g)
    for b in range(B):
        part_o[b, :, n_pages(lens[b]):] = float("nan")
    return part_o


def gemv_chain_ref(W, bias, act, y0, dtype, x=None, ln=False, part_o=None, part_ml=None, lens=None):
    """[B, G*N]: (LayerNorm | split-KV merge | nothing) -> grouped linear -> act -> (+ y0) in `dtype`, as the "bit-identical to the fp32
    launch" harnesses of the weight streams compute it; W [G, N, K], bias [G, N], x [B, G*K] or the partials of a merge launch."""
    G, N, K = W.shape
    if part_ml is not None:
        xin = merge_ref(part_o, part_ml, lens, dtype).unsqueeze(1)
    else:
        xin = x.reshape(-1, G, K).to(dtype)
        if ln:
            xin = F.layer_norm(xin, (K,), None, None, LN_EPS) if dtype == torch.float32 else ln_normalize(xin)
    y = torch.stack([F.linear(xin[:, k], W[k].to(dtype), bias[k].to(dtype)) for k in range(G)], 1)
    y = act_fn(y, act).reshape(xin.shape[0], G * N)
    return y if y0 is None else y + y0.to(dtype)


def gemv_chain_tol(floor, W, bias, act, y0, **kw):
    """the tolerance rule for one launch of such a harness, everything on the CPU"""
    cpu = lambda t: None if t is None else t.detach().cpu()
    kw = {k: (cpu(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    want = gemv_chain_ref(cpu(W), cpu(bias), act, cpu(y0), torch.float64, **kw)
    return tol(floor, max_err(gemv_chain_ref(cpu(W), cpu(bias), act, cpu(y0), torch.float32, **kw), want))


# ---------------------------------------------------------------------------------------------- attention keys with chosen logits
def logit_targets(name, length, g):
    """t[length] fp64: the logits scale * q . k_j the keys are built to give."""
    j = torch.arange(length, dtype=torch.float64)
    if name == "wide":
        return 60.0 * torch.randn(length, generator=g, dtype=torch.float64)
    if name == "ascending":
        return 1.25 * j - 100.0                                        # the running max moves at every key
    t = torch.zeros(length, dtype=torch.float64)
    if name == "late_peak":
        t[length - 1] = 120.0
    elif name == "early_peak":
        t[0] = 120.0
    elif name == "two_peaks":
        t[length - 1] = 119.5
        if length > 5:
            t[5] = 120.0
    else:
        raise KeyError(name)
    return t


def keys_for(q, t, g):
    """k [len, hd] fp32 with (1/sqrt(hd)) * q . k_j ~= t_j: k_j = 0.1 * randn + t_j * q * sqrt(hd) / |q|^2."""
    hd = q.numel()
    qd = q.double()
    k = 0.1 * torch.randn(t.numel(), hd, generator=g, dtype=torch.float64) + t[:, None] * qd[None, :] * (math.sqrt(hd) / float(qd @ qd))
    return k.float()


def attn_ref(q, k, v, scale, dtype=torch.float64, causal=False, subtract_max=True):
    """softmax(scale * q k^T) v in `dtype`; q [nq, hd], k / v [len, hd]. causal: query i (of nq == len) sees keys 0..i."""
    s = scale * (q.to(dtype) @ k.to(dtype).T)
    if causal:
        s = s.masked_fill(torch.ones_like(s, dtype=torch.bool).triu(1), float("-inf"))
    if subtract_max:
        p = torch.softmax(s, dim=-1)
    else:
        e = torch.exp(s)
        p = e / e.sum(-1, keepdim=True)
    return p @ v.to(dtype)


def attn_problem(case, H, hd, lens, seed, max_pages=4, n_layer=2, layer=1, gains=False, share=()):
    """A paged K/V pool (shuffled table) whose row r / head h logits follow `case`, its q, and per (row, head) the dense k, v.
    gains=True (prefill): every position i of a sequence gets q_i = gain_i * q0, gain in [0.5, 1]: `q` is then [sum(lens), H*hd].
    share: (head row, member row) pairs — the member's q is 0.9 x the head's and its first table entry names the head's first page."""
    g = torch.Generator().manual_seed(seed)
    R = len(lens)
    n_pg = R * max_pages
    pool = torch.randn(n_pg, n_layer, 2, H, PAGE, hd, generator=g)
    table = torch.randperm(n_pg, generator=g).to(torch.int32).view(R, max_pages)
    q0 = torch.randn(R, H * hd, generator=g)
    for head, member in share:
        q0[member] = 0.9 * q0[head]
    dense = {}
    for r, ln in enumerate(lens):
        for h in range(H):
            t = logit_targets(case, ln, g)
            k = keys_for(q0[r, h * hd:(h + 1) * hd], t, g)
            v = torch.randn(ln, hd, generator=g)
            dense[(r, h)] = (k, v)
            for p in range(n_pages(ln)):
                n = min(PAGE, ln - p * PAGE)
                pool[table[r, p], layer, 0, h, :n] = k[p * PAGE:p * PAGE + n]
                pool[table[r, p], layer, 1, h, :n] = v[p * PAGE:p * PAGE + n]
    for head, member in share:
        table[member, 0] = table[head, 0]
    if gains:
        q = torch.cat([(0.5 + 0.5 * torch.rand(ln, 1, generator=g)) * q0[r][None, :] for r, ln in enumerate(lens)], 0)
    else:
        q = q0
    return dict(pool=pool.contiguous(), table=table, q=q.contiguous(), dense=dense, lens=list(lens), H=H, hd=hd, layer=layer,
                max_pages=max_pages, n_layer=n_layer)


def attn_problem_ref(pb, dtype=torch.float64, causal=False, subtract_max=True, pool=None):
    """[R or sum(lens), H*hd] reference of attn_problem; `pool` (e.g. the bf16-rounded one) replaces the dense k / v when given."""
    H, hd, lens = pb["H"], pb["hd"], pb["lens"]
    scale = 1.0 / math.sqrt(hd)
    out = torch.zeros(pb["q"].shape[0], H * hd, dtype=dtype)
    row = 0
    for r, ln in enumerate(lens):
        for h in range(H):
            if pool is None:
                k, v = pb["dense"][(r, h)]
            else:
                k = torch.cat([pool[pb["table"][r, p], pb["layer"], 0, h] for p in range(n_pages(ln))], 0)[:ln]
                v = torch.cat([pool[pb["table"][r, p], pb["layer"], 1, h] for p in range(n_pages(ln))], 0)[:ln]
            if causal:
                out[row:row + ln, h * hd:(h + 1) * hd] = attn_ref(pb["q"][row:row + ln, h * hd:(h + 1) * hd], k, v, scale, dtype, True, subtract_max)
            else:
                out[r, h * hd:(h + 1) * hd] = attn_ref(pb["q"][r:r + 1, h * hd:(h + 1) * hd], k, v, scale, dtype, False, subtract_max)[0]
        row += ln if causal else 0
    return out


def attn_logits64(pb, r, h):
    k, _ = pb["dense"][(r, h)]
    hd = pb["hd"]
    return (pb["q"][r, h * hd:(h + 1) * hd].double() @ k.double().T) / math.sqrt(hd)
