"""GPU: the HIP codec (`ssr_speech_amd.codec.wmencodec.WMEncodecModel`, all arithmetic through the C-ABI) against the
REFERENCE's golden vectors (tests/golden/codec_*.npz). Bars: fp32 activations within 2e-4 absolute of the reference
(values are O(1); conv/LSTM chains of ~40 layers, different summation order); RVQ codes identical except where the
reference's own top-1/top-2 distance margin is below 1e-4 (an fp32 tie)."""
import glob
import os

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import weights as W
from ssr_speech_amd.codec.wmencodec import WMEncodecModel
from oracle import codec as OC
from helpers_codec import code_margins

pytestmark = pytest.mark.gpu
ATOL = 2e-4
CASES = sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "codec_*.npz")))


def load_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"codec_{name}.npz"))
    c = [int(v) for v in g["cfg"]]
    cfg = W.CodecConfig(dimension=c[0], n_filters=c[1], bins=c[2], n_q=c[3], ratios=tuple(c[4:]), pad_mode=str(g["pad_mode"]))
    sd = W.codec_state_dict(cfg, seed=int(g["weight_seed"]))
    return g, cfg, sd


@pytest.mark.parametrize("name", CASES)
def test_codec_matches_reference(golden_dir, name):
    g, cfg, sd = load_case(golden_dir, name)
    m = WMEncodecModel(cfg, sd, "cuda")
    wav = torch.from_numpy(g["wav"])
    codes, scale, emb = m.encode(wav.cuda())
    assert scale is None and codes.dtype == torch.int64 and tuple(codes.shape) == g["codes"].shape
    np.testing.assert_allclose(emb.cpu().numpy(), g["emb"], rtol=0, atol=ATOL)
    ref_codes = torch.from_numpy(g["codes"])
    diff = codes.cpu() != ref_codes
    if diff.any():
        marg = code_margins(sd, cfg, torch.from_numpy(g["emb"]), ref_codes)
        # a flipped code changes the residual of the later codebooks of that frame: only the FIRST flip per frame is judged
        first = diff.float().cumsum(1) == 1
        assert (marg[diff & first] < 1e-4).all(), (int(diff.sum()), marg[diff & first])
    dec = m.decode(ref_codes.cuda())
    np.testing.assert_allclose(dec.cpu().numpy(), g["decoded"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(m.decode_latent(ref_codes.cuda()).cpu().numpy(), OC.rvq_decode(sd, ref_codes, cfg).numpy(), rtol=0, atol=1e-6)
    out, mark = m.wmdecode(ref_codes.cuda(), torch.from_numpy(g["labels"]).cuda(), torch.from_numpy(g["wav_pad"]).cuda())
    np.testing.assert_allclose(out.cpu().numpy(), g["wmdecoded"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(mark.cpu().numpy(), g["mark"], rtol=0, atol=ATOL)
    out2, none = m.wmdecode(ref_codes.cuda(), torch.from_numpy(g["labels"]).cuda(), torch.from_numpy(g["wav_pad"]).cuda(), with_mark=False)
    assert none is None and torch.equal(out2, out)
    # detect_watermark (wmencodec.py:377-382) argmaxes the detector output [B,2,T'] over TIME (its squeeze(-1) is a no-op): values
    # must equal the reference's, except where the reference's own two largest entries along time are an fp32 near-tie
    det = m.detect_watermark(torch.from_numpy(g["wmdecoded"]).cuda())
    assert tuple(det.shape) == g["detect"].shape and det.dtype == torch.int64
    ref_det = g["detect"]
    bad = det.cpu().numpy() != ref_det
    if bad.any():
        per_class = np.moveaxis(g["mark"], 1, 2)                     # [B, 2, T']
        top2 = np.sort(per_class, axis=-1)[..., -2:]
        assert ((top2[..., 1] - top2[..., 0])[bad] < 2 * ATOL).all(), (det.cpu().numpy(), ref_det)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("tiny")])
def test_decode_through_the_few_output_channel_kernel_matches_reference(golden_dir, name):
    """`WMEncodecModel.force_few_out`: the decoder's 1-channel last layer on `ssrhip_conv_few_out` also for short inputs (the product
    takes it from 4096 output steps on, which no tiny fixture reaches). At the tiny config that layer is (C_out, C_in, k) = (1, 8, 7):
    the LDS form of the kernel, end to end against the reference fixture at the file's bar."""
    g, cfg, sd = load_case(golden_dir, name)
    assert cfg.n_filters % 8 == 0 and cfg.n_filters != 64
    m = WMEncodecModel(cfg, sd, "cuda")

    class CountingLib:
        few_out_calls = 0

        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, attr):
            fn = getattr(self._lib, attr)
            if attr != "ssrhip_conv_few_out":
                return fn

            def counted(*a):
                CountingLib.few_out_calls += 1
                return fn(*a)
            return counted

    m.lib = CountingLib(m.lib)
    ref_codes = torch.from_numpy(g["codes"]).cuda()
    plain = m.decode(ref_codes)
    assert CountingLib.few_out_calls == 0
    m.force_few_out = True
    dec = m.decode(ref_codes)
    assert CountingLib.few_out_calls >= 1, "the hook did not route the last layer to ssrhip_conv_few_out"
    np.testing.assert_allclose(dec.cpu().numpy(), g["decoded"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(dec.cpu().numpy(), plain.cpu().numpy(), rtol=0, atol=2e-5)


def test_codec_roundtrip_shapes_and_errors():
    cfg = W.codec_config_tiny()
    sd = W.codec_state_dict(cfg, seed=3)
    m = WMEncodecModel(cfg, sd, "cuda")
    for n in (cfg.hop * 3, cfg.hop * 3 + 1, cfg.hop * 5 - 1):
        codes, _, emb = m.encode(torch.randn(1, 1, n).cuda())
        frames = -(-n // cfg.hop)
        assert tuple(emb.shape) == (1, cfg.dimension, frames) and tuple(codes.shape) == (1, cfg.n_q, frames)
        assert tuple(m.decode(codes).shape) == (1, 1, frames * cfg.hop)
    with pytest.raises(IndexError):
        m.decode(torch.full((1, cfg.n_q, 3), cfg.bins, dtype=torch.long).cuda())     # stray special token
    with pytest.raises(AssertionError):
        m.encode(torch.randn(1, 100).cuda())


def test_lstm_large_batch_path_matches_small_batch_path():
    """B > 4 switches the recurrence to the fused matrix-core step kernel (16-item batch tiles); same clips must give the
    same result either way (the B <= 4 path is the one pinned against the reference fixtures)."""
    cfg = W.codec_config_tiny()
    sd = W.codec_state_dict(cfg, seed=4)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(0)
    wav = (torch.randn(6, 1, cfg.hop * 7, generator=g) * 0.3).cuda()
    c6, _, e6 = m.encode(wav)
    c2, _, e2 = m.encode(wav[:2])
    torch.testing.assert_close(e6[:2], e2, rtol=0, atol=2e-5)
    d6 = m.decode(c6)
    d2 = m.decode(c6[:2])
    torch.testing.assert_close(d6[:2], d2, rtol=0, atol=2e-5)


def test_lstm_mfma_step_full_width_two_batch_tiles():
    """Full codec config (LSTM width 1024 -> 2 waves per workgroup), 20 clips = two 16-item batch tiles, the second one ragged."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=5)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(1)
    wav = (torch.randn(20, 1, cfg.hop * 12 + 17, generator=g) * 0.2).cuda()
    m.lanes = 1                                                     # the whole batch in one launch chain: two batch tiles
    c20, _, e20 = m.encode(wav)
    for lo in (0, 15, 18):
        c2, _, e2 = m.encode(wav[lo:lo + 2])
        torch.testing.assert_close(e20[lo:lo + 2], e2, rtol=0, atol=2e-5)
    d20 = m.decode(c20)
    d2 = m.decode(c20[16:19])
    torch.testing.assert_close(d20[16:19], d2, rtol=0, atol=2e-5)


@pytest.mark.parametrize("B", [114, 130])
def test_lstm_wide_step_kernel_large_batch(B):
    """More than 112 clips switch the recurrence to `lstm_step_wide_kernel` (16 hidden units per workgroup, W_hh slice in registers,
    batch tiles walked in sequence, groups of 4: B=114: 8 tiles with a ragged last tile, B=130: 9 tiles = a ragged last group). Items from the first, a middle and the last tile must equal the same clips run through the small-batch path
    (which is pinned against the reference fixtures)."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=15)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(6)
    wav = (torch.randn(B, 1, cfg.hop * 9 + 33, generator=g) * 0.2).cuda()
    m.lanes = 1                                                     # one lane, or the halves would fall below the wide kernel's 8 tiles
    cB, _, eB = m.encode(wav)
    dB = m.decode(cB)
    for lo in (0, 47, B - 2):
        c2, _, e2 = m.encode(wav[lo:lo + 2])
        torch.testing.assert_close(eB[lo:lo + 2], e2, rtol=0, atol=2e-5)
        torch.testing.assert_close(dB[lo:lo + 2], m.decode(cB[lo:lo + 2]), rtol=0, atol=2e-5)


@pytest.mark.parametrize("lanes,B", [(2, 20), (3, 27), (2, 17)])
def test_batch_lanes_equal_one_lane(lanes, B):
    """A batch is cut into lanes that run one after the other (a memory knob: a lane's intermediates are freed before the next
    lane allocates). Every public entry point must return what the single-lane run returns: same arithmetic per item, only the
    launch grouping (and with it the tile shape of the large GEMMs and the LSTM's batch tile) differs."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=21)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(9)
    n = cfg.hop * 70 + 11                                           # 71 frames: the two-stream LSTM layer pipeline is on (chunks of 64)
    wav = (torch.randn(B, 1, n, generator=g) * 0.2).cuda()
    labels = torch.randint(0, 2, (B, 71), generator=g).cuda()

    def run(use_codes=None):
        codes, _, emb = m.encode(wav)
        dec_in = codes if use_codes is None else use_codes          # a flipped near-tie code must not leak into the decoder checks
        dec = m.decode(dec_in)
        track = torch.nn.functional.pad(wav, (0, 71 * cfg.hop - n))
        wm, mark = m.wmdecode(dec_in, labels, track)
        det = m.detect_watermark(wm)
        torch.cuda.synchronize()
        return codes, emb, dec, wm, mark, det

    m.lanes, m.lane_min_items = 1, 8
    one = run()
    m.lanes = lanes
    assert len(m._lane_cuts(B)) == lanes
    for rep in range(2):                                            # twice: the second run reuses the lanes' cached memory blocks
        many = run(one[0])
        for a, b in zip(one, many):
            assert a.shape == b.shape and a.dtype == b.dtype
            if a.dtype.is_floating_point:
                torch.testing.assert_close(a, b, rtol=0, atol=2e-5)
            else:
                assert (a != b).float().mean() < 0.002              # near-tie RVQ picks may flip with a different LSTM batch tile
    with pytest.raises(IndexError):
        bad = one[0].clone()
        bad[B - 1, 0, 0] = cfg.bins
        m.decode(bad)


def test_rvq_encode_mfma_equals_scalar_kernel(monkeypatch):
    """The matrix-core RVQ search (16 frames per workgroup) against the per-frame scalar kernel: same codes except where
    the two best scores of a frame are closer than 1e-4 (different fp32 summation order). Full width: 128 dims, 2048 bins."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=6)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(2)
    wav = (torch.randn(3, 1, cfg.hop * 37 + 5, generator=g) * 0.2).cuda()      # 38 frames: a ragged last 16-frame tile
    c_mfma, _, emb = m.encode(wav)
    monkeypatch.setenv("SSRHIP_RVQ_SCALAR", "1")
    c_scalar, _, emb2 = m.encode(wav)
    monkeypatch.delenv("SSRHIP_RVQ_SCALAR")
    assert torch.equal(emb, emb2)
    diff = (c_mfma != c_scalar).cpu()
    assert diff.float().mean() < 0.02
    if diff.any():
        marg = code_margins(sd, cfg, emb.cpu(), c_scalar.cpu())
        first = diff.float().cumsum(1) == 1
        assert (marg[diff & first] < 1e-4).all(), (int(diff.sum()), marg[diff & first])


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_fused_resblock_equals_two_gemm_path(pad_mode):
    """csrc/resblock.hip (64-channel SEANetResnetBlock as one kernel) vs the same block as two strided-view GEMMs: encoder
    (first block) and decoder (last block) at the full config, ragged length (tail tile), 3 clips."""
    import dataclasses
    cfg = dataclasses.replace(W.codec_config_full(), pad_mode=pad_mode)
    sd = W.codec_state_dict(cfg, seed=9)
    m = WMEncodecModel(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(3)
    wav = (torch.randn(3, 1, cfg.hop * 9 + 123, generator=g) * 0.2).cuda()
    c1, _, e1 = m.encode(wav)
    d1 = m.decode(c1)
    m.fuse_resblock = False
    c0, _, e0 = m.encode(wav)
    d0 = m.decode(c1)
    torch.testing.assert_close(e1, e0, rtol=0, atol=2e-5)
    torch.testing.assert_close(d1, d0, rtol=0, atol=2e-5)
    assert (c1 != c0).float().mean() < 0.02


@pytest.mark.parametrize("split_lstm", [False, True])
@pytest.mark.parametrize("B", [6, 20])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_large_batch_kernels_match_the_oracle_directly(B, pad_mode, split_lstm):
    """The kernels only batches > 4 reach — `lstm_step_mfma` (16-item batch tiles; B=20: two tiles, the second ragged), the
    fused residual blocks and the batched strided-view GEMMs — against oracle/codec.py itself (not against this package's
    small-batch path): full config, both pad modes, ragged length. Every item of the batch is checked. `split_lstm`: the same with the
    recurrence forced onto `csrc/lstm_split.hip` (bf16 matrix cores, split operands; the default only from 128 items up), whose 64-row
    batch group is ragged at both sizes: encoder, decoder, skip-encoder and detector LSTMs all against the oracle."""
    import dataclasses
    cfg = dataclasses.replace(W.codec_config_full(), pad_mode=pad_mode)
    sd = W.codec_state_dict(cfg, seed=13)
    m = WMEncodecModel(cfg, sd, "cuda")
    m.lanes = 1                                                     # B=20 in ONE lane: two batch tiles, the second ragged
    if split_lstm:
        assert m.lstm_split, "SSRHIP_LSTM_SPLIT=0 in the environment: nothing to force"
        m.lstm_split_min_b = 1
    g = torch.Generator().manual_seed(5)
    wav = torch.randn(B, 1, cfg.hop * 11 + 129, generator=g) * 0.2
    codes, _, emb = m.encode(wav.cuda())
    o_codes, _, o_emb = OC.encode(sd, wav, cfg)
    np.testing.assert_allclose(emb.cpu().numpy(), o_emb.numpy(), rtol=0, atol=ATOL)
    diff = codes.cpu() != o_codes
    if diff.any():
        marg = code_margins(sd, cfg, o_emb, o_codes)
        first = diff.float().cumsum(1) == 1
        assert (marg[diff & first] < 1e-4).all(), (int(diff.sum()), marg[diff & first])
    dec = m.decode(o_codes.cuda())
    np.testing.assert_allclose(dec.cpu().numpy(), OC.decode(sd, o_codes, cfg).numpy(), rtol=0, atol=ATOL)
    T = o_codes.shape[-1]
    labels = (torch.arange(T).unsqueeze(0).repeat(B, 1) % 3 == 0).long()
    wav_pad = torch.nn.functional.pad(wav, (0, T * cfg.hop - wav.shape[-1]))
    out, mark = m.wmdecode(o_codes.cuda(), labels.cuda(), wav_pad.cuda())
    o_out, o_mark = OC.wmdecode(sd, o_codes, labels, wav_pad, cfg)
    np.testing.assert_allclose(out.cpu().numpy(), o_out.numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(mark.cpu().numpy(), o_mark.numpy(), rtol=0, atol=ATOL)


@pytest.mark.parametrize("B", [2, 6])
def test_lstm_two_stream_pipeline_equals_sequential_layers(B):
    """T' = 150 frames > LSTM_CHUNK: the two LSTM layers run chunk-pipelined on two streams (windows of the time axis through
    ssrhip_lstm_args.t_begin/t_end, ragged last chunk); bit-identical to running layer 1 over all steps, then layer 2."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=12)
    m = WMEncodecModel(cfg, sd, "cuda")
    m.lstm_pipe_min_b = 1                        # (the product pipelines from 8 items on: SSRHIP_LSTM_PIPE_MIN_B)
    g = torch.Generator().manual_seed(4)
    wav = (torch.randn(B, 1, cfg.hop * 150, generator=g) * 0.2).cuda()
    c1, _, e1 = m.encode(wav)
    d1 = m.decode(c1)
    m.LSTM_CHUNK = 10 ** 9                       # never pipelined
    c0, _, e0 = m.encode(wav)
    d0 = m.decode(c1)
    assert torch.equal(e1, e0) and torch.equal(c1, c0) and torch.equal(d1, d0)


@pytest.mark.parametrize("name", ["full_const", "full_reflect"])
def test_every_seanet_layer_matches_the_reference(golden_dir, name):
    """the reference's own per-module outputs (forward hooks on SEANetEncoder.model / SEANetDecoder.model at the FULL
    config, odd input length, both pad modes; tests/golden/layers_*.npz) against this package's fused nodes, one node at a time and
    each node fed with the REFERENCE's input to it — so an error cannot hide behind (or be blamed on) an earlier layer. Covers every
    distinct (C_in, C_out, k, stride) convolution, transposed convolution, residual block (64 / 128 / 256 / 512 channels) and the LSTM."""
    from ssr_speech_amd.codec.wmencodec import TM
    g = np.load(os.path.join(golden_dir, f"layers_{name}.npz"))
    cfg = W.codec_config_full()
    cfg.pad_mode = str(g["pad_mode"])
    sd = W.codec_state_dict(cfg, seed=int(g["weight_seed"]))
    m = WMEncodecModel(cfg, sd, "cuda")
    m.fuse_channels = (64, 128, 256, 512)      # every fused residual-block kernel is checked, also the ones the default leaves to two GEMMs

    def as_tm(arr, nxt):                       # reference activation [1, C, T] -> time-major buffer with the halo `nxt` wants
        t = torch.from_numpy(arr)
        buf = m._alloc_for(1, t.shape[2], t.shape[1], nxt)
        buf.data[:, buf.padL: buf.padL + buf.T] = t.permute(0, 2, 1).cuda()
        m._fill_pads(buf, structural_zero=(nxt is not None and nxt[1] == "convtr"))
        return buf

    checked = stored_through_elu = 0
    for pfx, net, first_in in (("enc_", m.encoder, None), ("dec_", m.decoder, None)):
        nodes = net.nodes
        for idx, node in enumerate(nodes):
            nxt = nodes[idx + 1] if idx + 1 < len(nodes) else None
            if idx == 0:
                if pfx == "enc_":
                    x = m._input_tm(torch.from_numpy(g["wav"]).cuda(), node)
                else:
                    x = m._dequant(m._codes32(torch.from_numpy(g["codes"])), node)
            else:
                x = as_tm(g[f"{pfx}{nodes[idx - 1][3]}"], node)          # the reference's output of the previous node
            y = m._run([node], x, after=nxt)
            want = g[f"{pfx}{node[3]}"]
            if y.elu:        # a residual block / the LSTM stores ELU(output): its only consumers read it through ELU (wmencodec._run)
                want = torch.nn.functional.elu(torch.from_numpy(want)).numpy()
                stored_through_elu += 1
            got = y.interior_view().permute(0, 2, 1).cpu().numpy()
            assert got.shape == want.shape, (pfx, node[0], node[1], got.shape, want.shape)
            np.testing.assert_allclose(got, want, rtol=0, atol=5e-5, err_msg=f"{pfx}{node[3]} ({node[1]})")
            checked += 1
    assert checked == len(m.encoder.nodes) + len(m.decoder.nodes) >= 22
    assert stored_through_elu == 10            # 4 + 4 residual blocks and the two LSTMs


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_elu_on_store_and_split_gemm_equal_the_plain_path(pad_mode, monkeypatch):
    """Round 3's two codec changes against the path they replace, end to end at the full config (encode, decode, wmdecode with the
    detector, 5 clips of odd length): (a) ELU applied once by the producer (`elu_on_store`) instead of by every consumer on load — the
    same function on the same values, so BIT-identical; (b) the GEMMs on the bf16 matrix cores with exactly split operands
    (`split_gemm`) instead of the fp32 FMA chain — fp32-accurate, so equal within the codec's tolerance, and both within it of the oracle."""
    import dataclasses
    cfg = dataclasses.replace(W.codec_config_full(), pad_mode=pad_mode)
    sd = W.codec_state_dict(cfg, seed=31)
    g = torch.Generator().manual_seed(8)
    wav = torch.randn(5, 1, cfg.hop * 13 + 57, generator=g) * 0.2

    def run(split, on_store):
        m = WMEncodecModel(cfg, sd, "cuda")
        m.split_gemm, m.elu_on_store = split, on_store
        if not split:
            m._plane_cache.clear()
        codes, _, emb = m.encode(wav.cuda())
        return m, codes, emb

    m_new, c_new, e_new = run(True, True)
    m_a, c_a, e_a = run(True, False)
    m_old, c_old, e_old = run(False, False)
    assert torch.equal(e_new, e_a) and torch.equal(c_new, c_a)                          # (a) bit-identical
    torch.testing.assert_close(e_new, e_old, rtol=0, atol=5e-5)                          # (b)
    o_codes, _, o_emb = OC.encode(sd, wav, cfg)
    np.testing.assert_allclose(e_new.cpu().numpy(), o_emb.numpy(), rtol=0, atol=ATOL)
    T = o_codes.shape[-1]
    labels = (torch.arange(T).unsqueeze(0).repeat(5, 1) % 3 == 0).long()
    wav_pad = torch.nn.functional.pad(wav, (0, T * cfg.hop - wav.shape[-1]))
    outs = [(m.decode(o_codes.cuda()),) + m.wmdecode(o_codes.cuda(), labels.cuda(), wav_pad.cuda()) for m in (m_new, m_a, m_old)]
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)
    for x, y in zip(outs[0], outs[2]):
        torch.testing.assert_close(x, y, rtol=0, atol=5e-5)
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), OC.decode(sd, o_codes, cfg).numpy(), rtol=0, atol=ATOL)
    o_w, o_m = OC.wmdecode(sd, o_codes, labels, wav_pad, cfg)
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), o_w.numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(outs[0][2].cpu().numpy(), o_m.numpy(), rtol=0, atol=ATOL)


def test_codec_calls_on_concurrent_streams_equal_the_single_stream_results():
    """Three caller streams, each with its own inputs, issue encode -> decode -> wmdecode back to back so that their kernels interleave on
    the GPU (the two-stream LSTM pipeline is on: 71 frames); 12 rounds; every result must equal the result of the same call made alone.
    History: rounds 3-5 saw this fail in the FIRST concurrent round of 1-20 % of fresh processes and could not say why. Round 6's
    per-process trials (tools/race_trials.py, profiles/r06_microbench/) named the conditions — kernels of several hardware queues in
    flight while the caching allocator maps fresh device memory — and the codec now sizes every new (entry point, stream, shape) with
    the device idle (`WMEncodecModel._sized`): the first use of a stream is a sizing pass, the overlap of the three callers is real
    from then on, and no real pass may reach the driver for memory (`mallocs_in_flight == 0`, asserted below). Every hand-over to the LSTM
    side stream is an event and the calling stream joins it before the layer returns (wmencodec._lstm)."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=21)
    m = WMEncodecModel(cfg, sd, "cuda")
    m.lstm_pipe_min_b = 1                        # the two-stream LSTM pipeline for every caller (the product: from 8 items on)
    g = torch.Generator().manual_seed(19)
    n = cfg.hop * 70 + 11
    Bs = (9, 7, 9)
    wavs = [(torch.randn(b, 1, n, generator=g) * 0.2).cuda() for b in Bs]
    labels = [torch.randint(0, 2, (b, 71), generator=g).cuda() for b in Bs]
    tracks = [torch.nn.functional.pad(w, (0, 71 * cfg.hop - n)) for w in wavs]

    def call(i):
        codes, _, emb = m.encode(wavs[i])
        dec = m.decode(codes)
        wm, mark = m.wmdecode(codes, labels[i], tracks[i])
        return codes, emb, dec, wm, mark

    alone = [call(i) for i in range(3)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    for rnd in range(12):
        got = [None] * 3
        for i in ((0, 1, 2) if rnd % 2 == 0 else (2, 0, 1)):
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                got[i] = call(i)
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        for i in range(3):
            for k, (a, b) in enumerate(zip(alone[i], got[i])):
                if not torch.equal(a, b):
                    bad = (a != b).nonzero()
                    raise AssertionError(f"round {rnd}, caller {i} (batch {Bs[i]}), output {k} of (codes, emb, dec, wm, mark), shape {tuple(a.shape)}: "
                                         f"{bad.shape[0]} elements differ, max |diff| {float((a.float() - b.float()).abs().max()):.3g}, "
                                         f"first at {bad[0].tolist()}, last at {bad[-1].tolist()}; codec: {m.sizing_passes} sizing passes, "
                                         f"{m.mallocs_in_flight} driver allocations in flight, {m.passes_repeated} passes repeated")
    # alone: 3 entry points on the default stream (batch 9 covers batch 7); concurrent: 3 entry points on each of 3 new streams
    assert m.mallocs_in_flight == 0, f"{m.mallocs_in_flight} driver allocations happened while sized codec passes were in flight"
    assert m.sizing_passes == 3 + 9, m.sizing_passes


def test_sized_codec_calls_never_reach_the_driver_for_memory_and_change_no_result():
    """`WMEncodecModel._sized` (round 6): a shape not yet covered on this stream runs once dry with the device idle; the real pass and
    every later call of that size or smaller must then be served from the allocator's pool (the driver-allocation counter does not move
    while codec kernels are in flight), and the outputs are bit-identical to the unsized path (SSRHIP_CODEC_PRESIZE=0)."""
    cfg = W.codec_config_full()
    sd = W.codec_state_dict(cfg, seed=5)
    g = torch.Generator().manual_seed(4)
    wav = (torch.randn(6, 1, cfg.hop * 80 + 7, generator=g) * 0.2).cuda()
    lab = torch.randint(0, 2, (6, 81), generator=g).cuda()
    m0 = WMEncodecModel(cfg, sd, "cuda")
    m0.presize = False
    c0, _, e0 = m0.encode(wav)
    d0 = m0.decode(c0)
    trk = torch.nn.functional.pad(wav, (0, 81 * cfg.hop - wav.shape[-1]))
    w0, k0 = m0.wmdecode(c0, lab, trk)
    torch.cuda.synchronize()
    del m0
    torch.cuda.empty_cache()                                              # a cold allocator for the sized model
    m = WMEncodecModel(cfg, sd, "cuda")
    assert m.presize
    n_before = torch.cuda.memory_stats()["num_device_alloc"]
    c1, _, e1 = m.encode(wav)
    assert m.sizing_passes == 1 and torch.cuda.memory_stats()["num_device_alloc"] > n_before      # the dry pass did the mapping
    d1 = m.decode(c1)
    w1, k1 = m.wmdecode(c1, lab, trk)
    assert m.sizing_passes == 3 and m.mallocs_in_flight == 0
    for a, b in ((c0, c1), (e0, e1), (d0, d1), (w0, w1), (k0, k1)):
        assert torch.equal(a, b)
    # a smaller call: covered; a larger one: one more sizing pass; still nothing mapped in flight
    n_mid = torch.cuda.memory_stats()["num_device_alloc"]
    c2, _, _ = m.encode(wav[:4, :, : cfg.hop * 40])
    assert m.sizing_passes == 3 and torch.equal(c2, m.encode(wav[:4, :, : cfg.hop * 40])[0])
    assert torch.cuda.memory_stats()["num_device_alloc"] == n_mid
    big = (torch.randn(8, 1, cfg.hop * 120, generator=g) * 0.2).cuda()
    m.encode(big)
    assert m.sizing_passes == 4 and m.mallocs_in_flight == 0


@pytest.mark.parametrize("knob", ["SSRHIP_GEMM_SPLIT_DMA=0", "SSRHIP_RESBLOCK_DMA=0", "SSRHIP_EPILOGUE_TM=0"])
def test_reference_fixtures_under_every_surviving_codec_knob(knob):
    """The codec keeps three superseded kernel generations behind switches that are read once per process (the 4-wave split GEMM — also the
    fallback for views beyond the DMA kernel's 32-bit offsets —, the round-3 residual-block kernels, the general epilogue of the
    transposed convolutions). The suite above runs the DEFAULT path; this runs the reference fixtures (end to end and per SEANet layer) and
    the large-batch oracle comparison once more in a child process per switch, so that no shipped kernel goes unexecuted."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name, val = knob.split("=")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_codec.py"), "-x", "-q", "-k",
                          "codec_matches_reference or every_seanet_layer or (large_batch_kernels and 20 and constant and False)"],
                         env=dict(os.environ, **{name: val}), cwd=root, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-2000:]
    import re as _re
    n_passed = int(_re.search(r"(\d+) passed", out.stdout).group(1))
    assert n_passed >= 8, f"the -k expression selected only {n_passed} tests: {out.stdout[-500:]}"   # (a renamed test must not shrink this silently)

