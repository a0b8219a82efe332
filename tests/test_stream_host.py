"""CPU: the host side of stream synthesis. `layout.FrameAssembler` (which frames of the final result are already final while the
decode loop still runs) against `layout.assemble`, and the window plan of `codec.wmencodec.DecodeStream` (`stream_margins` /
`stream_window`) against oracle/codec.py: the layers behind the LSTM run over windows with the plan's margins must reproduce the full
decode, and with one frame less they must not."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import layout as LY
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import stream_lookahead, stream_margins, stream_window
from oracle import codec as OC

K, T_Y = 4, 23
ARGS = SimpleNamespace(empty_token=64, eog=65, audio_pad_token=66, eos=67, sos=68, mts=69, max_n_spans=3)

# name -> (mask intervals, generated frames per span, out_len)
CASES = {
    "tts": ([[T_Y, T_Y]], [19], 0),                      # zero-length span at the end
    "edit_start": ([[0, 5]], [9], 0),
    "two_spans": ([[3, 7], [12, 15]], [6, 21], 0),
    "three_spans": ([[2, 4], [9, 9], [17, 22]], [5, 1, 18], 0),
    "empty_span": ([[3, 7], [12, 15]], [0, 8], 0),       # a span that generates 0 frames: its K rows are the eog cascade alone
    "aug_context": ([[8, 13]], [11], 5),                 # out_len frames dropped in front
}


def _case(name):
    mi, n_gen, out_len = CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    y = g.integers(0, 64, size=(K, T_Y)).astype(np.int64)
    nmi, _ = LY.intervals(T_Y, np.asarray(mi))
    spans = []
    for f in n_gen:                                      # what the sampler writes: the delayed frames, then the eog cascade
        seg = np.concatenate([g.integers(0, 64, size=(K, f)), np.full((K, 1), ARGS.eog)], 1).astype(np.int64)
        spans.append(LY.delay_pattern(seg, ARGS.empty_token).T)
    return y, nmi, spans, out_len


def _want(y, nmi, spans, out_len):
    res, marks, masks, nmi_out = LY.assemble(y, spans, nmi, ARGS)
    o = out_len                                          # the aug_context crop of SSR_Speech.inference
    return res[:, o:], marks[o:], [(a - o, b - o) for a, b in masks], [(a - o, b - o) for a, b in nmi_out]


def _rows_needed(nmi, spans, out_len):
    """for every frame of the final result (after the crop): how many generated rows must exist before it may be released"""
    need, start = [], 0
    for (s, e), sp in zip(nmi, spans):
        need += [start] * (e - s)                        # a kept segment: the span in front of it has ended (0 rows for the first)
        n_frames = sp.shape[0] - K
        need += [start + t + K for t in range(n_frames)]          # frame t: its last codebook sits in local row t + K - 1
        start += sp.shape[0]
    need += [start] * (nmi[-1][1] - nmi[-1][0])
    return need[out_len:]


@pytest.mark.parametrize("piece", [1, 5, 16, 10 ** 6])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_assembler_releases_final_frames_only_and_ends_equal_to_assemble(name, piece):
    y, nmi, spans, out_len = _case(name)
    res, marks, masks, nmi_out = _want(y, nmi, spans, out_len)
    need = _rows_needed(nmi, spans, out_len)
    assert len(need) == res.shape[1]
    rows = np.concatenate(spans, 0)
    ends = np.cumsum([sp.shape[0] for sp in spans]).tolist()
    asm = LY.FrameAssembler(y, nmi, ARGS, out_len)
    got_c, got_m = [np.zeros((K, 0), dtype=np.int64)], [np.zeros(0, dtype=np.int64)]

    def take(incs, n_rows):
        for inc in incs:
            assert inc.codes.shape == (K, inc.marks.shape[0]) and inc.codes.shape[1] > 0
            assert np.all(inc.marks == (0 if inc.kept else 1))
            got_c.append(inc.codes)
            got_m.append(inc.marks)
        n = sum(c.shape[1] for c in got_c)
        assert n == asm.n_released
        # every release extends the prefix that was out before (nothing is retracted), and holds final values only
        assert np.array_equal(np.concatenate(got_c, 1), res[:, :n]) and np.array_equal(np.concatenate(got_m), marks[:n])
        assert all(r <= n_rows for r in need[:n]), "a frame left before the row of its last codebook existed"
        return n

    n_first = take(asm.start(), 0)
    first_kept = nmi[0][1] - nmi[0][0]
    assert n_first >= max(first_kept - out_len, 0)       # the first kept segment is final at once
    fed = 0
    while fed < rows.shape[0]:
        nxt = min(fed + piece, rows.shape[0])
        span = sum(e <= nxt for e in ends)
        span_end = [e if e <= nxt else 0 for e in ends] + [0] * (ARGS.max_n_spans - len(ends))
        take(asm.feed(rows[fed:nxt], span, span_end), nxt)
        fed = nxt
    assert asm.finished
    r2, m2, k2, n2 = asm.result()
    assert np.array_equal(r2, res) and np.array_equal(m2, marks) and k2 == masks and n2 == nmi_out
    assert np.array_equal(np.concatenate(got_c, 1), res) and np.array_equal(np.concatenate(got_m), marks)
    assert np.array_equal(asm.rows, rows)


def test_frame_assembler_never_releases_the_eog_column():
    y, nmi, spans, _ = _case("tts")
    asm = LY.FrameAssembler(y, nmi, ARGS)
    asm.start()
    rows = spans[0]
    incs = asm.feed(rows[:-1], 0, [0, 0, 0])             # every row but the last of the cascade: the span has not ended
    assert sum(i.codes.shape[1] for i in incs) == rows.shape[0] - K
    assert all(ARGS.eog not in i.codes for i in incs)
    with pytest.raises(RuntimeError):
        asm.result()
    assert asm.feed(rows[-1:], 1, [rows.shape[0], 0, 0]) == [] and asm.finished      # TTS: the closing kept segment is empty


# ----------------------------------------------------------------------------------------------- the codec's window plan
def _codec_cfg(name):
    if name == "r8542":
        cfg = W.CodecConfig(dimension=64, n_filters=8, ratios=(8, 5, 4, 2), bins=64)
        return cfg, W.codec_state_dict(cfg, seed=7)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"codec_{name}.npz"))
    c = [int(v) for v in g["cfg"]]
    cfg = W.CodecConfig(dimension=c[0], n_filters=c[1], bins=c[2], n_q=c[3], ratios=tuple(c[4:]), pad_mode=str(g["pad_mode"]))
    return cfg, W.codec_state_dict(cfg, seed=int(g["weight_seed"]))


@functools.lru_cache(maxsize=None)
def _stages(name, T):
    """(cfg, sd, stage-1 output [1, C, T], the full decode [1, 1, T * hop]) — computed once per shape, never modified"""
    cfg, sd = _codec_cfg(name)
    codes = torch.randint(0, cfg.bins, (1, cfg.n_q, T), generator=torch.Generator().manual_seed(100 + T))
    layout = OC.decoder_layout(cfg)
    with torch.no_grad():
        s1 = OC.run_layers(sd, "decoder.", layout, OC.rvq_decode(sd, codes, cfg), cfg, 0, 2)      # first convolution + LSTM
        full = OC.run_layers(sd, "decoder.", layout, s1, cfg, 2, None)
        assert torch.equal(full, OC.decode(sd, codes, cfg))
    return cfg, sd, s1, full


def _windowed(name, T, window, margins):
    cfg, sd, s1, full = _stages(name, T)
    layout, out = OC.decoder_layout(cfg), []
    with torch.no_grad():
        for c0 in range(0, T, window):
            c1 = min(c0 + window, T)
            lo, hi = stream_window(c0, c1, T, margins)
            y = OC.run_layers(sd, "decoder.", layout, s1[..., lo:hi], cfg, 2, None)
            out.append(y[..., (c0 - lo) * cfg.hop: (c1 - lo) * cfg.hop])
    return float((torch.cat(out, -1) - full).abs().max())


@pytest.mark.parametrize("window", [1, 7, 16])
@pytest.mark.parametrize("T", [1, 3, 5, 6, 17, 61])
@pytest.mark.parametrize("name", ["tiny_reflect", "tiny_const", "r8542"])
def test_windows_with_the_plans_margin_reproduce_the_full_decode(name, T, window):
    """1e-5 absolute: 10x the fp32 noise of re-running the same layers over another extent (8e-7 .. 1.1e-6 at signal scale 1.2 .. 1.8),
    three orders below what a margin one frame short costs (the test below)."""
    cfg, _ = _codec_cfg(name)
    assert _windowed(name, T, window, stream_margins(cfg)) <= 1e-5


@pytest.mark.parametrize("name", ["tiny_reflect", "tiny_const"])
def test_a_margin_one_frame_short_is_seen(name):
    """the tiny ratios (4, 3, 2, 2) are the shapes whose receptive field needs both frames"""
    cfg, _ = _codec_cfg(name)
    ml, mr = stream_margins(cfg)
    assert (ml, mr) == (2, 2)
    assert _windowed(name, 61, 16, (ml - 1, mr)) > 1e-5
    assert _windowed(name, 61, 16, (ml, mr - 1)) > 1e-5
    assert _windowed(name, 61, 16, (ml - 1, mr - 1)) > 1e-5


def test_the_plan_follows_the_configuration():
    assert stream_lookahead(W.CodecConfig()) == 3 and stream_lookahead(W.CodecConfig(kernel_size=5)) == 2
    assert stream_margins(W.CodecConfig()) == (1, 1)                       # (8, 5, 4, 2): one frame covers the field
    assert stream_margins(W.CodecConfig(ratios=(2, 2), last_kernel_size=15)) > stream_margins(W.CodecConfig(ratios=(2, 2)))
    assert stream_window(0, 16, 61, (2, 2)) == (0, 18) and stream_window(48, 61, 61, (2, 2)) == (46, 61)
    assert stream_window(16, 32, 33, (2, 2)) == (14, 33)
