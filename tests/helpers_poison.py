"""What a dead page of the split-KV partials is filled with, and the rule every consumer of those partials is held to.

`part_ml[B][H][MS][2]` / `part_o[B][H][MS][hd]` have one (m, l) pair / one partial output per page; a row of n = ceil(len / PAGE) pages
wrote pages 0..n-1 in this step, the pages n..MS-1 hold what an earlier, longer decode left (zeros on a new engine). A merge must not
let them into its result. NaN alone does not show that: `fmaxf(x, NaN) == x`, a maximum swallows it. So every dead page is filled with
each of DEAD_FILLS in turn, and the kernel's whole output buffer (guard tails included) must keep the same BITS under all of them
(`same_bits`: compared as int32, no tolerance). `above` is the last-bit detector: per (row, head) the live maximum of m plus 8 with
l = 1, finite and harmless where it is ignored, but a maximum it reaches moves every rounding behind it.

No GPU here; tests/test_gpu_dead_pages.py applies the rule to the kernels."""
import math

import torch

PAGE = 128
NAN = float("nan")
DEAD_FILLS = (NAN, 0.0, float("inf"), float("-inf"), 3.0e38, -3.0e38, "above")


def fill_name(dead):
    return dead if isinstance(dead, str) else ("nan" if math.isnan(dead) else f"{dead:g}")


def n_pages(length):
    return (length + PAGE - 1) // PAGE


def fill_dead(part_o, part_ml, lens, dead=NAN):
    """In place, on the CPU: the pages >= n_pages(lens[b]) of row b of part_o [B, H, MS, hd] and part_ml [B, H, MS, 2] take `dead`
    (m, l and every partial output alike; `above`: m and the outputs take the (row, head)'s live maximum of m plus 8, l takes 1)."""
    for b, length in enumerate(lens):
        n = n_pages(length)
        if n >= part_ml.shape[2]:
            continue
        if dead == "above":
            top = part_ml[b, :, :n, 0].max(dim=1).values + 8.0                           # [H]
            part_ml[b, :, n:, 0] = top[:, None]
            part_ml[b, :, n:, 1] = 1.0
            part_o[b, :, n:] = top[:, None, None]
        else:
            part_ml[b, :, n:] = dead
            part_o[b, :, n:] = dead
    return part_o, part_ml


def rotations(B, MS):
    """Lists of B lengths whose page counts, over all lists, give every n in 1..MS to at least one row, each at a length that is not
    a multiple of the page except the longest (n = MS: the full buffer)."""
    counts = list(range(1, MS + 1))
    while len(counts) % B:
        counts.append(counts[len(counts) % MS])
    length = lambda n: MS * PAGE if n == MS else (n - 1) * PAGE + 1 + (37 * n) % (PAGE - 1)
    return [[length(n) for n in counts[i:i + B]] for i in range(0, len(counts), B)]


def bits(t):
    """the int32 view of an fp32 tensor or array (NaN compares equal to itself there)"""
    if torch.is_tensor(t):
        return t.detach().cpu().contiguous().view(torch.int32)
    import numpy as np
    return np.ascontiguousarray(t).view(np.int32)


def same_bits(outs, what):
    """outs: {fill: tensor / array, or a tuple of them}. Every entry equals the first one bit for bit, whole buffers."""
    names = list(outs)
    first = outs[names[0]]
    as_tuple = lambda v: v if isinstance(v, (tuple, list)) else (v,)
    bad = []
    for name in names[1:]:
        for k, (got, ref) in enumerate(zip(as_tuple(outs[name]), as_tuple(first))):
            gb, rb = bits(got), bits(ref)
            differ = (gb != rb)
            n = int(differ.sum())
            if n:
                g = torch.as_tensor(got).detach().cpu().reshape(-1).double()
                bad.append((fill_name(name), k, n, "NaN/inf output" if not bool(torch.isfinite(g).all()) else "last-bit mismatch"))
    assert not bad, (what, "against fill " + fill_name(names[0]), bad)
