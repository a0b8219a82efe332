"""CPU: the host side of the per-token log-probabilities (DESIGN.md Part I.27) — `layout.assemble_logprobs` places the value of every
generated token where `layout.assemble` places the token, `TokenLogprobs`' summary fields, and the CLI flag."""
import json
import math
import os

import numpy as np
import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W

K = 4
KEPT = -1          # what the kept frames of `y` hold in these tests: no encoded index is negative


def _case(y_len, mask_interval, new_frames):
    """-> (y [K, T] of KEPT, non_mask_intervals, span_end): spans that generate new_frames[i] frames take new_frames[i] + K steps each
    (the frames, the eog column, K - 1 steps of delay)"""
    args = W.lm_args_tiny()
    y = np.full((K, y_len), KEPT, dtype=np.int64)
    _, _, num_task, nmi = LY.build_layout(np.zeros((K, y_len), dtype=np.int64), np.asarray(mask_interval), args)
    assert num_task == len(new_frames)
    return args, y, nmi, list(np.cumsum([n + K for n in new_frames]))


@pytest.mark.parametrize("out_len", [0, 3])
@pytest.mark.parametrize("y_len,mask_interval,new_frames", [(9, [[9, 9]], [6]),                 # TTS: one span behind the prompt
                                                            (14, [[2, 5], [9, 11]], [7, 1]),    # an edit of two spans
                                                            (14, [[2, 5], [9, 11]], [0, 4])])   # ... whose first span generates no frame
def test_frames_hold_the_value_of_the_step_and_codebook_assemble_put_there(y_len, mask_interval, new_frames, out_len):
    args, y, nmi, span_end = _case(y_len, mask_interval, new_frames)
    n_steps = span_end[-1]
    idx = np.arange(n_steps * K, dtype=np.int64).reshape(n_steps, K)           # entry s * K + k
    ends = [0] + span_end
    res, marks, _, _ = LY.assemble(y, [idx[ends[i]:ends[i + 1]] for i in range(len(new_frames))], nmi, args)
    res, marks = res[:, out_len:], marks[out_len:]                             # the aug_context crop of the tokens
    lp = LY.assemble_logprobs(idx.astype(np.float32), span_end, y.shape[1], nmi, out_len)
    assert isinstance(lp, LY.TokenLogprobs)
    assert lp.steps.dtype == np.float32 and lp.steps.shape == (n_steps, K) and np.array_equal(lp.steps, idx)
    assert lp.frames.dtype == np.float32 and lp.frames.shape == (1,) + res.shape
    kept = res == KEPT
    assert np.array_equal(np.isnan(lp.frames[0]), kept)                        # NaN exactly at the kept frames
    assert np.array_equal(kept.all(0), marks == 0) and np.array_equal(kept.any(0), marks == 0)
    assert np.array_equal(lp.frames[0][~kept].astype(np.int64), res[~kept])    # the same step and codebook as the token
    if out_len == 0:
        assert (~kept).sum() == K * sum(new_frames)                            # every generated frame, all K codebooks


def test_forced_entries_stay_nan_in_the_frames_and_out_of_the_summary():
    args, y, nmi, span_end = _case(9, [[9, 9]], [5])
    n_steps = span_end[-1]
    steps = -np.arange(1, n_steps * K + 1, dtype=np.float32).reshape(n_steps, K) / 8
    forced = np.zeros((n_steps, K), dtype=bool)
    forced[0, 1:] = forced[1, 2:] = forced[2, 3:] = True                      # start-of-span delay
    forced[5, 0] = True                                                        # stop rule
    for j in range(1, K):
        forced[5 + j, : j + 1] = True                                          # eog cascade
    steps[forced] = np.nan
    lp = LY.assemble_logprobs(steps, span_end, 9, nmi)
    ok = ~forced
    assert lp.count == int(ok.sum()) and lp.count > 0
    assert lp.total == float(steps[ok].astype(np.float64).sum()) and lp.mean == lp.total / lp.count
    # every drawn entry of a frame column is in `frames`; the forced ones that fall into a frame are NaN there
    fin = lp.frames[0][~np.isnan(lp.frames[0])]
    assert sorted(fin.tolist()) == sorted(steps[ok].tolist())
    assert np.isnan(lp.frames[0][:, :9]).all() and lp.frames.shape == (1, K, 9 + 5)


def test_summary_of_an_all_forced_run_is_nan_not_an_error():
    args, y, nmi, span_end = _case(9, [[9, 9]], [0])
    lp = LY.assemble_logprobs(np.full((span_end[-1], K), np.nan, dtype=np.float32), span_end, 9, nmi)
    assert lp.count == 0 and lp.total == 0.0 and math.isnan(lp.mean)
    assert lp.frames.shape == (1, K, 9) and np.isnan(lp.frames).all()


def test_cli_takes_rank_samples_and_the_reference_flags_are_unchanged(golden_dir):
    from ssr_speech_amd import inference_v2 as CLI
    assert CLI.parse_args([]).rank_samples is False
    assert CLI.parse_args(["--rank_samples", "--sample_batch_size", "4"]).rank_samples is True
    assert "--rank_samples" in [f for f, _ in CLI.EXTRA_FLAGS] and "--rank_samples" not in [f for f, _ in CLI.REFERENCE_FLAGS]
    with open(os.path.join(golden_dir, "cli_flags.json")) as f:
        ref = json.load(f)
    assert [f for f, _ in CLI.REFERENCE_FLAGS] == [r["flag"] for r in ref]                       # order and content: the reference's


def test_write_scores_ranks_by_mean_logprob_and_puts_nan_last(tmp_path):
    from ssr_speech_amd import inference_v2 as CLI
    scores = [dict(seed=3, mean_logprob=-2.5, total_logprob=-25.0, count=10, frames=7), dict(seed=4, mean_logprob=float("nan"), total_logprob=0.0, count=0, frames=0),
              dict(seed=5, mean_logprob=-1.25, total_logprob=-10.0, count=8, frames=5)]
    path = str(tmp_path / "s_scores.json")
    assert CLI.write_scores(path, scores) is None
    with open(path) as f:
        got = json.load(f)
    assert [r["seed"] for r in got] == [5, 3, 4] and got[2]["mean_logprob"] is None and got[0] == scores[2]
