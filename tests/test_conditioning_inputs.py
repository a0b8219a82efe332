"""CPU: the ill-conditioned inputs of helpers_conditioning.py are worth having and their tolerances can be met.

For every K the GPU tests use, fp32 torch meets tol = max(floor, M * err_ref32) by construction, while each wrong form of the
arithmetic — a one-pass variance, a slice merge without its between-slice term, eps outside the square root, a softmax without the
max subtraction — misses both 16 * err_ref32 and the tolerance the GPU tests apply (M = helpers_conditioning.M) by at least 10x on
the case built for it. So a kernel copy that regresses to one of these forms fails tests/test_gpu_conditioning.py."""
import math

import pytest
import torch

import helpers_conditioning as hc

KS = [16, 128, 1024, 2048, 4096]


def _problem(K, case, seed=0):
    g = torch.Generator().manual_seed(1000 + K + seed)
    N = 64
    x = hc.ln_rows(4, K, seed + K)[case]
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    return x, W, bias


def _errs(K, case, form):
    x, W, bias = _problem(K, case)
    y64 = hc.ln_linear_ref(x, W, bias)
    e32 = hc.max_err(hc.ln_linear_ref(x, W, bias, dtype=torch.float32), y64)
    ebad = hc.max_err(hc.ln_linear_ref(x, W, bias, dtype=torch.float32, form=form), y64)
    return e32, ebad


@pytest.mark.parametrize("K", KS)
def test_fp32_reference_is_within_its_own_tolerance(K):
    for case, x in hc.ln_rows(4, K, K).items():
        _, W, bias = _problem(K, "tiny")
        y64 = hc.ln_linear_ref(x, W, bias, act=2)
        e32 = hc.max_err(hc.ln_linear_ref(x, W, bias, act=2, dtype=torch.float32), y64)
        assert math.isfinite(e32) and e32 <= hc.tol(hc.FLOOR_GEMV, e32), (case, e32)
        assert e32 < 0.05, (case, e32)                        # and the tolerance it leads to still means something: outputs are O(1)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case,form", [("offset", "one_pass"), ("step", "within_slice"), ("tiny", "eps_outside")])
def test_wrong_layernorm_forms_miss_the_widest_tolerance_tenfold(K, case, form):
    e32, ebad = _errs(K, case, form)
    bound = hc.tol(hc.FLOOR_GEMV, e32, m=16)
    print(f"K={K} {case}/{form}: err_ref32 {e32:.3g}  wrong form {ebad:.3g}  ratio to the bound {ebad / bound:.3g}")
    assert ebad >= 10 * bound, (e32, ebad)                    # inf (a negative one-pass variance -> NaN) counts as a miss
    assert ebad >= 10 * hc.tol(hc.FLOOR_GEMV, e32), (e32, ebad)   # ... and so does the bound the GPU tests apply (M = hc.M)


@pytest.mark.parametrize("K", KS)
def test_wrong_forms_pass_on_the_old_operating_point(K):
    """The gap this closes: on randn * 1.5 + 0.3 the one-pass variance is as good as the two-pass one."""
    g = torch.Generator().manual_seed(K)
    x = torch.randn(4, K, generator=g) * 1.5 + 0.3
    _, W, bias = _problem(K, "tiny")
    y64 = hc.ln_linear_ref(x, W, bias)
    assert hc.max_err(hc.ln_linear_ref(x, W, bias, dtype=torch.float32, form="one_pass"), y64) < hc.FLOOR_GEMV


@pytest.mark.parametrize("K", KS)
def test_const_rows_have_an_exact_mean_and_normalise_to_zero(K):
    x = hc.ln_rows(4, K, 3)["const"]
    assert float(torch.tensor(3.25 * K, dtype=torch.float32)) == 3.25 * K             # 13 * K / 4 < 2^24: every partial sum is exact
    assert torch.equal(x.sum(-1), torch.full((4,), 3.25 * K)) and torch.equal(x.mean(-1), torch.full((4,), 3.25))
    assert torch.equal(hc.ln_normalize(x), torch.zeros(4, K))
    _, W, bias = _problem(K, "tiny")
    assert torch.equal(hc.ln_linear_ref(x, W, bias, dtype=torch.float32), bias.expand(4, -1))


def test_outlier_is_left_out_of_rows_it_would_dominate():
    assert "outlier" not in hc.ln_rows(2, 8, 0) and "outlier" in hc.ln_rows(2, 16, 0)
    assert set(hc.ln_rows(2, 16, 0)) == set(hc.LN_CASES)


# ---------------------------------------------------------------------------------------------- merge
LENS = [8 * hc.PAGE, 1, 300, 7 * hc.PAGE + 1]


@pytest.fixture(scope="module")
def merge_inputs():
    B, H, MS, hd = 4, 4, 8, 64
    return hc.merge_part_o(B, H, MS, hd, LENS, 5), hc.ml_cases(B, H, MS, LENS, 6)


@pytest.mark.parametrize("case", hc.ML_CASES)
def test_merge_partials_are_well_formed_and_fp32_meets_the_tolerance(merge_inputs, case):
    part_o, mls = merge_inputs
    ml = mls[case]
    for b, ln in enumerate(LENS):
        n = hc.n_pages(ln)
        assert torch.isnan(ml[b, :, n:]).all() and torch.isnan(part_o[b, :, n:]).all()
        assert torch.isfinite(ml[b, :, :n]).all()
        assert float(ml[b, :, :n, 1].min()) >= 1.0 and float(ml[b, :, :n, 1].max()) <= 128.0
    want = hc.merge_ref(part_o, ml, LENS)
    e32 = hc.max_err(hc.merge_ref(part_o, ml, LENS, dtype=torch.float32), want)
    assert e32 <= hc.tol(hc.FLOOR_GEMV, e32) and e32 < 1e-3, e32
    spread = float(ml[0, :, :, 0].max() - ml[0, :, :, 0].min())
    assert spread > 88.0 or case == "two_peaks", spread        # beyond what exp() holds in fp32 without the max subtraction
    if case == "two_peaks":                                     # both peak pages carry weight: neither may be dropped
        m, l_ = ml[0, :, :, 0].double(), ml[0, :, :, 1].double()
        e = torch.exp(m - m.max(1, keepdim=True).values)
        share = e * l_ / (e * l_).sum(1, keepdim=True)
        assert float(share[:, 0].min()) > 1e-3 and float(share[:, 7].min()) > 1e-3


@pytest.mark.parametrize("case", ["wide", "ascending", "late_peak", "two_peaks"])
def test_merge_without_the_max_subtraction_is_not_finite(merge_inputs, case):
    part_o, mls = merge_inputs
    bad = hc.merge_ref(part_o, mls[case], LENS, dtype=torch.float32, subtract_max=False)
    assert not torch.isfinite(bad[0]).all()                     # the 8-page row


# ---------------------------------------------------------------------------------------------- attention logits
ALENS = [1, 129, 257, 385]


@pytest.fixture(scope="module", params=[64, 128])
def attn_problems(request):
    return {case: hc.attn_problem(case, 2, request.param, ALENS, 50 + i) for i, case in enumerate(hc.LOGIT_CASES)}


@pytest.mark.parametrize("case", hc.LOGIT_CASES)
def test_constructed_logits_reach_their_targets(attn_problems, case):
    pb = attn_problems[case]
    s = hc.attn_logits64(pb, 3, 1)                              # the 385-key row
    if case == "wide":
        assert float(s.max()) > 100.0 and float(s.min()) < -100.0
    elif case == "ascending":
        assert float(s[0]) < -95.0 and float(s[-1]) > 370.0
        assert int((s.cummax(0).values[1:] > s.cummax(0).values[:-1]).sum()) > 0.9 * (len(s) - 1)    # the running max keeps moving
    else:
        assert float(s.max()) > 115.0 and float(s.median().abs()) < 2.0
    if case == "two_peaks":
        w = torch.softmax(s, 0)
        assert float(w[5]) > 0.3 and float(w[-1]) > 0.3, (float(w[5]), float(w[-1]))
    want = hc.attn_problem_ref(pb)
    e32 = hc.max_err(hc.attn_problem_ref(pb, dtype=torch.float32), want)
    assert e32 <= hc.tol(hc.FLOOR_ATTN, e32) and e32 < 5e-3, e32


@pytest.mark.parametrize("case", ["wide", "ascending", "late_peak", "early_peak", "two_peaks"])
def test_softmax_without_the_max_subtraction_is_not_finite(attn_problems, case):
    pb = attn_problems[case]
    bad = hc.attn_problem_ref(pb, dtype=torch.float32, subtract_max=False)
    assert not torch.isfinite(bad[3]).all()


def test_prefill_problem_is_causal_and_scaled_per_query():
    pb = hc.attn_problem("late_peak", 2, 64, [5, 130], 9, gains=True)
    assert pb["q"].shape == (135, 128)
    ref = hc.attn_problem_ref(pb, causal=True)
    k, v = pb["dense"][(0, 0)]
    assert torch.allclose(ref[0, :64], v[0].double())          # the first query sees the first key only
    assert torch.isfinite(ref).all()
