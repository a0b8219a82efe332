"""CPU: the fills of tests/helpers_poison.py tell a merge that lets a dead page into its maximum from one that does not — and NaN, the
only fill the suite used before, does not. The model is the fp32 arithmetic of the merge prologues (csrc/gemv.hip `combine_finish`):
M = max m, den = sum e^(m - M) l, w = e^(m - M) / den, out = sum w o over the live pages; `leaky` takes M over the dead pages too,
with fmaxf's rule for NaN (the other operand)."""
import numpy as np
import pytest
import torch

import helpers_conditioning as hc
import helpers_poison as HP


def merge_fp32(part_o, part_ml, lens, leaky):
    B, H, MS, hd = part_o.shape
    out = torch.zeros(B, H * hd)
    for b in range(B):
        n = HP.n_pages(lens[b])
        m_all = part_ml[b, :, :, 0]
        m, l_ = m_all[:, :n], part_ml[b, :, :n, 1]
        over = m_all if leaky else m
        M = torch.where(torch.isnan(over), torch.tensor(-float("inf")), over).max(dim=1, keepdim=True).values      # fmaxf(x, NaN) == x
        e = torch.exp(m - M)
        w = e * (1.0 / (e * l_).sum(dim=1, keepdim=True))
        out[b] = (w.unsqueeze(-1) * part_o[b, :, :n]).sum(dim=1).reshape(-1)
    return out


def _partials(B=4, H=4, MS=8, hd=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, MS, hd, generator=g),
            torch.stack([torch.randn(B, H, MS, generator=g) * 2, torch.rand(B, H, MS, generator=g) + 0.5], dim=-1).contiguous())


def test_rotations_give_every_live_page_count():
    for B in (1, 2, 4):
        for MS in (1, 2, 3, 7, 8, 9):
            lists = HP.rotations(B, MS)
            assert all(len(v) == B and max(v) <= MS * HP.PAGE and min(v) >= 1 for v in lists)
            assert {HP.n_pages(x) for v in lists for x in v} == set(range(1, MS + 1))


def test_fill_dead_touches_the_dead_pages_only():
    lens = [1, 300, 1024, 129]
    for dead in HP.DEAD_FILLS:
        o0, ml0 = _partials()
        o, ml = HP.fill_dead(o0.clone(), ml0.clone(), lens, dead)
        for b, v in enumerate(lens):
            n = HP.n_pages(v)
            assert torch.equal(o[b, :, :n], o0[b, :, :n]) and torch.equal(ml[b, :, :n], ml0[b, :, :n])
            if n < 8:
                if dead == "above":
                    top = ml0[b, :, :n, 0].max(dim=1).values + 8.0
                    assert torch.equal(ml[b, :, n:, 0], top[:, None].expand(-1, 8 - n)) and bool((ml[b, :, n:, 1] == 1.0).all())
                    assert bool(torch.isfinite(o[b, :, n:]).all())
                elif dead != dead:
                    assert bool(torch.isnan(ml[b, :, n:]).all()) and bool(torch.isnan(o[b, :, n:]).all())
                else:
                    assert bool((ml[b, :, n:] == dead).all()) and bool((o[b, :, n:] == dead).all())


@pytest.mark.parametrize("leaky", [False, True])
def test_the_fills_expose_a_dead_page_in_the_maximum_and_nan_does_not(leaky):
    lens = [1, 300, 1024, 129]
    o0, ml0 = _partials()
    outs = {dead: merge_fp32(*HP.fill_dead(o0.clone(), ml0.clone(), lens, dead), lens, leaky) for dead in HP.DEAD_FILLS}
    ref = outs[HP.NAN]
    assert hc.max_err(ref, hc.merge_ref(o0, ml0, lens)) < 1e-5            # NaN passes either way: the suite's blind spot
    differ = {HP.fill_name(d): not np.array_equal(HP.bits(outs[d]), HP.bits(ref)) for d in HP.DEAD_FILLS[1:]}
    if not leaky:
        assert not any(differ.values()), differ
        HP.same_bits(outs, "guarded")
    else:
        assert differ["inf"] and differ["3e+38"] and differ["above"] and differ["0"], differ     # (0: some live maximum here is negative)
        assert not differ["-inf"] and not differ["-3e+38"], differ                               # below every live m: harmless in a max
        assert HP.DEAD_FILLS[2] == float("inf") and not bool(torch.isfinite(outs[HP.DEAD_FILLS[2]]).all())   # e^(m - inf) = 0, 1 / 0: NaN rows
        assert bool(torch.isfinite(outs["above"]).all())                                         # the last-bit detector stays finite
        with pytest.raises(AssertionError):
            HP.same_bits(outs, "leaky")
