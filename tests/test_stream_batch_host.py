"""CPU: the host side of the batched stream (DESIGN.md Part I.16) — pure functions only. The alignment plan and the per-poll range and
window rules of `codec.wmencodec.BatchDecodeStream`, the frame ranges handed to `ssrhip_stream_gather` against `layout.FrameAssembler`,
the refusals, the CLI flag, and a numpy model of the gather kernel (kept here for tests/test_gpu_stream_batch.py) against the
reference's `revert_pattern_sequence` as recorded in tests/golden/layout.npz."""
import argparse
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec import wmencodec as WM
from ssr_speech_amd.engine import MAX_ROWS

K = 4
ARGS = SimpleNamespace(empty_token=64, eog=65, audio_pad_token=66, eos=67, sos=68, mts=69, max_n_spans=3)


def gather_model(generated: np.ndarray, ranges: np.ndarray, codes_out: np.ndarray, bins: int) -> bool:
    """What `ssrhip_stream_gather` computes, on `codes_out` [B][K][cap] in place: generated [n][max_steps][K], ranges [4][n] =
    step0 | f0 | f1 | col0. Returns the flag (an id outside [0, bins) was met, and stored clamped)."""
    flag = False
    for u in range(ranges.shape[1]):
        step0, f0, f1, col0 = (int(v) for v in ranges[:, u])
        for f in range(f0, f1):
            for k in range(generated.shape[2]):
                v = int(generated[u, step0 + f + k, k])
                flag |= not 0 <= v < bins
                codes_out[u, k, col0 + f] = min(max(v, 0), bins - 1)
    return flag


# ----------------------------------------------------------------------------------------------- the gather, against the reference
@pytest.mark.parametrize("name", ["tts", "mid", "start", "end", "two", "three", "insert"])
def test_gather_model_undoes_the_delay_pattern_as_the_reference_does(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "layout.npz"))
    pat, want = g[f"{name}_pattern"], g[f"{name}_reverted"]              # [K, S] -> revert_pattern_sequence -> [K, S - K + 1]
    n = want.shape[1]
    gen = np.full((2, pat.shape[1] + 3, K), -7, dtype=np.int64)
    gen[1, 3:] = pat.T                                                    # second utterance, its span starts at step 3
    out = np.full((2, K, n + 2), -1, dtype=np.int64)
    flag = gather_model(gen, np.array([[0, 3], [0, 0], [0, n], [0, 2]]), out, 64)
    assert not flag
    assert np.array_equal(out[1, :, 2:], want) and np.all(out[0] == -1) and np.all(out[1, :, :2] == -1)
    # in two pieces, into the columns a poll's block uses (col0 = -f0)
    a, b = np.full((1, K, 4), -1), np.full((1, K, n - 4), -1)
    gather_model(gen[1:], np.array([[3], [0], [4], [0]]), a, 64)
    gather_model(gen[1:], np.array([[3], [4], [n], [-4]]), b, 64)
    assert np.array_equal(np.concatenate([a[0], b[0]], 1), want)


def test_gather_model_clamps_and_flags():
    gen = np.zeros((1, 8, K), dtype=np.int64)
    gen[0, 2, 1] = 64                                                     # frame 1, codebook 1
    gen[0, 5, 3] = -3                                                     # frame 2, codebook 3
    out = np.full((1, K, 5), -1)
    assert gather_model(gen, np.array([[0], [0], [5], [0]]), out, 64)
    assert out[0, 1, 1] == 63 and out[0, 3, 2] == 0 and out.sum() == 63
    assert not gather_model(gen, np.array([[0], [3], [5], [0]]), out, 64)   # the bad ids are outside the range: no flag


# ----------------------------------------------------------------------------------------------- frame ranges vs FrameAssembler
def _one_span(frames, seed):
    g = np.random.default_rng(seed)
    y = g.integers(0, 64, size=(K, 11)).astype(np.int64)
    seg = np.concatenate([g.integers(0, 64, size=(K, frames)), np.full((K, 1), ARGS.eog)], 1).astype(np.int64)
    return y, LY.delay_pattern(seg, ARGS.empty_token).T                  # rows [frames + K, K]: the span, its eog cascade included


@pytest.mark.parametrize("chunk", [16, 7])
def test_gather_ranges_release_what_the_frame_assembler_releases(chunk):
    """three utterances in lock-step whose spans end AT a poll boundary (32 rows), one step behind it (33) and one in front (31)"""
    ends = [32, 33, 31]
    utts = [_one_span(e - K, 10 + i) for i, e in enumerate(ends)]
    n = len(utts)
    gen = np.full((n, 64, K), 99, dtype=np.int64)                          # rows the sampler has not written hold junk
    asms = []
    for u, (y, rows) in enumerate(utts):
        gen[u, : rows.shape[0]] = rows
        nmi, _ = LY.intervals(y.shape[1], np.array([[y.shape[1], y.shape[1]]]))
        asms.append(LY.FrameAssembler(y, nmi, ARGS))
        first = asms[-1].start()
        assert len(first) == 1 and first[0].kept and np.array_equal(first[0].codes, y)      # the prompt first, flagged kept
    released, fed, step, polls_with_frames = [0] * n, [0] * n, 0, [0] * n
    while any(f < e for f, e in zip(fed, ends)):
        step += chunk
        states = [(min(step, e), step >= e, e if step >= e else 0) for e in ends]          # (n_steps, span ended, span_end[0])
        table = LY.stream_gather_ranges(released, states, K)
        assert table.dtype == np.int32 and table.shape == (4, n)
        width = int((table[2] - table[1]).max())
        block = np.full((n, K, max(width, 1)), -1, dtype=np.int64)
        assert not gather_model(gen, table, block, 64)
        for u in range(n):
            n_rows, ended, end = states[u]
            incs = asms[u].feed(gen[u, fed[u]: n_rows], int(ended), [end, 0, 0])
            fed[u] = n_rows
            want = np.concatenate([i.codes for i in incs], 1) if incs else np.zeros((K, 0), dtype=np.int64)
            assert all(not i.kept for i in incs)
            step0, f0, f1, col0 = table[:, u]
            assert (step0, f0, col0) == (0, released[u], -released[u])
            assert f1 - f0 == want.shape[1], (u, step)
            assert np.array_equal(block[u, :, : f1 - f0], want) and np.all(block[u, :, f1 - f0:] == -1)
            assert f1 == LY.final_generated_frames(n_rows, ended, end, K)
            released[u] = int(f1)
            polls_with_frames[u] += int(f1 > f0)
    assert released == [e - K for e in ends] and all(a.finished for a in asms)
    assert all(p >= 2 for p in polls_with_frames)
    # a live utterance of the lock-step group releases the same number of frames as every other live one, an ending one no more
    assert LY.final_generated_frames(16, False, 0, K) == 13 and LY.final_generated_frames(16, True, 16, K) == 12
    assert LY.final_generated_frames(2, False, 0, K) == 0 and LY.final_generated_frames(4, True, 4, K) == 0


# ----------------------------------------------------------------------------------------------- the codec's alignment plan and rules
def test_alignment_plan():
    p = WM.batch_align_plan((5, 19, 40), 3)
    assert p["off"] == [38, 24, 3] and p["E"] == 43
    assert p["zero"] == [(0, 38), (0, 24), (0, 3)]                         # rows in front of each item's first frame
    assert all(o + n == p["E"] for o, n in zip(p["off"], (5, 19, 40)))   # every prompt ends at E
    assert WM.batch_align_plan((7,), 0) == dict(off=[0], E=7, zero=[(0, 0)])
    with pytest.raises(ValueError):
        WM.batch_align_plan((5, 0), 3)
    with pytest.raises(ValueError):
        WM.batch_align_plan((), 3)


def test_stage1_range_rule():
    R = WM.batch_stage1_range
    no = [False] * 3
    assert R(0, [43, 43, 43], no, no, 3) == (0, 40)                        # the prompts: up to the rows whose look-ahead exists
    assert R(40, [59, 59, 59], no, no, 3) == (40, 56)
    assert R(40, [59, 50, 59], no, no, 3) == (40, 47)                      # unequal arrivals: as far as EVERY live item allows
    assert R(40, [41, 59, 59], no, no, 3) == (40, 40)                      # ... which may be nothing
    # item 0 has ended at row 50: it limits nothing, and is closed by a call that reaches its end
    assert R(40, [50, 59, 59], [True, False, False], no, 3) == (40, 56)
    # ended at row 58, inside the look-ahead of the live items: this call stops at 56, the item stays open until a later one
    assert R(40, [58, 59, 59], [True, False, False], no, 3) == (40, 56)
    # no live item left: the call runs to the last end that is still open; closed items count for nothing
    assert R(56, [58, 61, 60], [True] * 3, no, 3) == (56, 61)
    assert R(56, [58, 61, 60], [True] * 3, [False, True, False], 3) == (56, 60)
    assert R(61, [58, 61, 60], [True] * 3, [True] * 3, 3) == (61, 61)


def test_window_rule_per_item_and_who_runs_together():
    item = lambda **kw: WM.batch_window_item(**dict(dict(off=24, E=43, n2=43, top=59, n1=56, closed=False, margins=(2, 2), max_window=16,
                                                         hop=320, few_min_t=4096, few_eligible=True), **kw))
    # what DecodeStream does for that item alone, shifted by its first row: stream_window in the item's own frames
    c0, c1, lo, hi, few = item()
    assert (c0, c1) == (43, 54) and few is True                             # limit = n1 - right margin; 35 frames x 320 >= 4096
    assert (lo - 24, hi - 24) == WM.stream_window(43 - 24, 54 - 24, 56 - 24, (2, 2))
    assert item(off=3)[:4] == (43, 54, 41, 56)                              # a longer prompt: the same rows
    # a prompt shorter than the left margin: the window would cross the item's first frame — cut there, a true edge
    short = item(off=42)
    assert short[:4] == (43, 54, 42, 56) and short[4] is True
    assert item(off=42, top=50, n1=47) is None                              # 8 frames: the last layer's kernel is not known yet -> wait
    assert item(off=42, top=50, n1=50, closed=True) == (43, 50, 42, 50, False)      # ended short: known, and its end is a true edge
    assert item(few_eligible=False)[4] is False
    assert item(n2=54) is None and item(n1=45) is None                      # nothing new behind the margin
    assert item(top=58, n1=58, closed=True)[:4] == (43, 58, 41, 58)         # an ended item runs to its end, no right margin
    assert item(max_window=4)[:2] == (43, 47)
    # who runs together: the largest set of equal windows, if it has two members; everything else alone
    a, b = item(), short
    assert WM.batch_window_groups([a, a, b]) == (a, [0, 1], [2])
    assert WM.batch_window_groups([a, None, b]) == (None, [], [0, 2])
    assert WM.batch_window_groups([None, None]) == (None, [], [])
    assert WM.batch_window_groups([b, a, b, a, a]) == (a, [1, 3, 4], [0, 2])
    ended = item(top=50, n1=56, closed=True)
    assert WM.batch_window_groups([a, a, ended]) == (a, [0, 1], [2])        # an ended item's last window runs alone


# ----------------------------------------------------------------------------------------------- one window rule for both streams
class _OneUtterance:
    """The host state of a `DecodeStream`: an `emit=False` prefix, pushes, finish(). `n1` follows the stage-1 readiness rule."""

    def __init__(self, pr0):
        self.pr0, self.n_pushed, self.n1, self.n2, self.emit_from = pr0, 0, 0, 0, None

    def arrive(self, n, emit, final):
        if (emit or final) and self.emit_from is None:
            self.emit_from = self.n2 = self.n_pushed
        self.n_pushed += n
        self.n1 = max(self.n1, self.n_pushed if final else self.n_pushed - self.pr0)


def _windows_before_the_core(s, final, margins, max_window, hop, few_min_t, few_eligible, force_few_out):
    """`DecodeStream._stage2` and `._few_out` as they were before both streams took their windows from `batch_window_item`"""
    out = []
    if s.emit_from is None:
        return out
    if not few_eligible or force_few_out:
        few = False
    elif s.n_pushed * hop >= few_min_t:
        few = True
    else:
        few = False if final else None
    if few is None:
        return out
    limit = s.n_pushed if final else s.n1 - margins[1]
    while s.n2 < limit:
        c0, c1 = s.n2, min(s.n2 + max_window, limit)
        lo, hi = WM.stream_window(c0, c1, s.n1, margins)
        out.append((c0, c1, lo, hi, few))
        s.n2 = c1
    return out


def _windows_by_the_batch_rule(s, final, margins, max_window, hop, few_min_t, few_eligible, force_few_out):
    """the same decision as `DecodeStream._stage2` takes it now: the item with off = 0, E = emit_from, top = n_pushed, closed = final"""
    out = []
    while s.emit_from is not None:
        w = WM.batch_window_item(off=0, E=s.emit_from, n2=s.n2, top=s.n_pushed, n1=s.n1, closed=final, margins=margins, max_window=max_window,
                                 hop=hop, few_min_t=few_min_t, few_eligible=few_eligible and not force_few_out)
        if w is None:
            break
        out.append(w)
        s.n2 = w[1]
    return out


def _windows_by_decode_stream(s, final, margins, max_window, hop, few_min_t, few_eligible, force_few_out):
    """... and `DecodeStream._stage2` itself, on an instance that has the host state only and records the windows it would run"""
    st, out = object.__new__(WM.DecodeStream), []
    st.m = SimpleNamespace(FEW_OUT_MIN_T=few_min_t, force_few_out=force_few_out)
    st.margins, st.max_window, st.hop, st._few_eligible = margins, max_window, hop, few_eligible
    st.n_pushed, st.n1, st.n2, st.emit_from = s.n_pushed, s.n1, s.n2, s.emit_from
    st._run_window = lambda win, item, who, row0: out.append(win) if (item, who, row0) == (0, [0], 0) else out.append("not item 0")
    st._stage2(final)
    s.n2 = st.n2
    return out


@pytest.mark.parametrize("ratios", [(4, 3, 2, 2), (8, 5, 4, 2)])
def test_decode_stream_takes_the_windows_it_took_before_from_the_batch_rule(ratios):
    cfg = W.CodecConfig(dimension=64, n_filters=8, ratios=ratios, bins=64)
    margins, pr0, hop = WM.stream_margins(cfg), WM.stream_lookahead(cfg), cfg.hop
    assert margins == {(4, 3, 2, 2): (2, 2), (8, 5, 4, 2): (1, 1)}[ratios] and pr0 == 3
    cases = windows = waited = 0
    for T in (1, 2, 5, 6, 17, 61):
        for prefix in (0, 20):
            total = prefix + T
            # the last layer's kernel is known from the first frame on / from the middle on / with the very last frame / at finish() only
            for few_min_t in (1, total * hop // 2 + 1, total * hop, total * hop + 1):
                for push, max_window, eligible, force in [(p, w, e, f) for p in (1, 7, 16, 10 ** 6) for w in (1, 7, 16) for e in (False, True)
                                                          for f in (False, True)]:
                    rule = (margins, max_window, hop, few_min_t, eligible, force)
                    runs = [(_OneUtterance(pr0), fn) for fn in (_windows_before_the_core, _windows_by_the_batch_rule, _windows_by_decode_stream)]
                    events = ([(prefix, False, False)] if prefix else []) + [(min(push, T - t), True, False) for t in range(0, T, push)] + [(0, True, True)]
                    for n, emit, final in events:
                        got = []
                        for s, fn in runs:
                            s.arrive(n, emit, final)
                            got.append((fn(s, final, *rule), s.n2))
                        assert got[0] == got[1] == got[2], (T, prefix, few_min_t, push, max_window, eligible, force, (n, emit, final), got)
                        assert all(w[0] >= prefix and w[1] - w[0] <= max_window for w in got[0][0])
                        windows += len(got[0][0])
                        waited += int(not final and not got[0][0] and runs[0][0].n1 - margins[1] > runs[0][0].n2)
                    assert runs[0][0].n2 == total == runs[1][0].n2 == runs[2][0].n2
                    cases += 1
    assert cases == 6 * 2 * 4 * 4 * 3 * 2 * 2 and windows > cases and waited > 0      # (waited: polls held back for the last layer's kernel)


# ----------------------------------------------------------------------------------------------- refusals, before any library call
def _utt(T=9, mi=None, L=5):
    return {"x": torch.zeros(1, L, dtype=torch.long), "y": torch.zeros(1, T, K, dtype=torch.long),
            "mask_interval": torch.tensor([mi if mi is not None else [[T, T]]], dtype=torch.long)}


def test_refusals_come_before_any_library_call(monkeypatch):
    from ssr_speech_amd.models.ssr import SSR_Speech
    from ssr_speech_amd import inference_scale as S

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    m = SSR_Speech(W.lm_args_tiny())
    monkeypatch.setattr(m, "_get_engine", boom)
    with pytest.raises(ValueError, match="inference_batch"):                 # a speech edit: the span does not end the utterance
        m.inference_batch_stream([_utt(), _utt(mi=[[2, 5]])])
    with pytest.raises(ValueError, match="inference_batch"):                 # two spans
        m.inference_batch_stream([_utt(mi=[[1, 3], [5, 9]])])
    with pytest.raises(ValueError, match="inference_batch"):                 # more than one engine pass
        m.inference_batch_stream([_utt()] * (MAX_ROWS // 2 + 1), aug_text=True)
    with pytest.raises(ValueError, match="inference_batch"):
        m.inference_batch_stream([_utt()] * (MAX_ROWS + 1))
    with pytest.raises(ValueError):
        m.inference_batch_stream([])
    with pytest.raises(ValueError, match="render_many"):
        LY.check_stream_batch([9], [np.array([[9, 9]])], 2, MAX_ROWS, use_watermark=True)
    assert LY.check_stream_batch([9, 12], [np.array([[9, 9]]), np.array([[7, 12]])], 2, MAX_ROWS) == [9, 7]
    # a valid call is an iterator and nothing has run: not the engine lookup, not the library
    it = m.inference_batch_stream([_utt()] * (MAX_ROWS // 2), aug_text=True)
    assert it.results is None and it.polls == 0 and it.prompt_lens == [9] * (MAX_ROWS // 2)
    # the public entries: use_watermark=True (and an edit, for the samples of one utterance) before anything else is touched
    gen = S.inference_batch_stream(None, None, None, None, None, [], 1.5, 1, True, True, "cpu", {}, seed=1)
    with pytest.raises(ValueError, match="render_many"):
        next(gen)
    for tts, wm in ((True, True), (False, False)):
        gen = S.inference_samples_stream(None, None, None, None, None, None, "", "", None, 1.5, 1, True, False, wm, tts, "cpu", {}, seeds=[1, 2])
        with pytest.raises(ValueError, match="inference_samples"):
            next(gen)


def test_signatures_follow_inference_batch():
    from ssr_speech_amd.models.ssr import SSR_Speech
    from ssr_speech_amd.data.tokenizer import AudioTokenizer
    b = inspect.signature(SSR_Speech.inference_batch).parameters
    s = inspect.signature(SSR_Speech.inference_batch_stream).parameters
    shared = [p for p in b if p not in ("refill", "group", "share_prompt")]
    assert [p for p in s if p in b] == shared and all(s[p].default == b[p].default for p in shared if p != "self")
    assert not {"refill", "group", "share_prompt"} & set(s)
    assert list(inspect.signature(WM.WMEncodecModel.decode_stream_batch).parameters)[1:] == ["prompt_lens", "max_new_frames", "max_window"]
    assert inspect.signature(WM.WMEncodecModel.decode_stream_batch).parameters["max_window"].default == 16
    assert hasattr(AudioTokenizer, "decode_stream_batch")
    assert "ssrhip_stream_gather" in [n for n, _, _ in _lib.SYMBOLS]


def test_stream_dir_flag():
    from ssr_speech_amd import inference_v2 as CLI
    flags = dict(CLI.EXTRA_FLAGS)
    names = [f for f, _ in CLI.EXTRA_FLAGS]
    assert names.index("--stream_dir") == names.index("--share_prompt") + 1
    assert flags["--stream_dir"]["type"] is str and flags["--stream_dir"]["default"] is None
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream_dir", **flags["--stream_dir"])
    assert ap.parse_args([]).stream_dir is None and ap.parse_args(["--stream_dir", "out"]).stream_dir == "out"
