"""No GPU: the float64 references of tests/helpers_codec.py (what tests/test_gpu_codec_kernels.py compares the kernels of
csrc/codec.hip with) against oracle/codec.py, which is itself pinned to the imported reference — so that a kernel test cannot be
wrong together with its reference. Exact for the pads and the codes (codes on the frames the margin filter keeps), 1e-12 relative
for the float64 arithmetic; random inputs at the tiny config's shapes. And the design condition of the RVQ kernel test: for every
shape it runs, the filter that uses the float64 reference alone keeps at least 90 % of the frames."""
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import weights as W
from oracle import codec as OC
import helpers_codec as H


def _tiny64(seed):
    cfg = W.codec_config_tiny()
    sd = W.codec_state_dict(cfg, seed=seed)
    return cfg, sd, {k: v.double() for k, v in sd.items()}


def _close(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float64
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1.0), float((got - want).abs().max())


@pytest.mark.parametrize("reflect", [0, 1])
@pytest.mark.parametrize("pl,pr", [(3, 3), (6, 0), (0, 6), (2, 5), (0, 0)])
def test_pad_reference_equals_the_oracle_pad1d(pl, pr, reflect):
    g = torch.Generator().manual_seed(10 * pl + pr)
    for n in (1, 2, 3, 4, 7, 49, 50):
        x = torch.randn(2, 5, n, generator=g)
        want = OC.pad1d(x, (pl, pr), "reflect" if reflect else "constant")
        assert torch.equal(H.pad1d_ref(x, pl, pr, reflect), want)
        for b in range(2):
            assert torch.equal(H.pad_rows_ref(x[b].t().contiguous(), pl, pr, reflect), want[b].t())
    # an empty item (a clamped ragged length): nothing to reflect, every halo row is zero
    assert torch.equal(H.pad_rows_ref(torch.zeros(0, 5), pl, pr, reflect), torch.zeros(pl + pr, 5))


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_conv_references_equal_the_oracle_sconv1d(pad_mode):
    """The two convolutions codec.hip owns, at the tiny config: the encoder's first layer (C_in = 1, k = 7) and the decoder's last
    (C_out = 1, k = 7, fed through ELU), in float64 on both sides."""
    cfg, _, sd = _tiny64(3)
    reflect = pad_mode == "reflect"
    g = torch.Generator().manual_seed(5)
    # first layer: [B][1][n] -> [B][n_filters][n]
    pfx = "encoder.model.0."
    w = OC.wn_weight(sd, pfx)
    k = w.shape[-1]
    x = torch.randn(3, 1, 77, generator=g).double()
    want = OC.sconv1d(sd, pfx, x, 1, pad_mode)
    pr = (k - 1) // 2
    xp = H.pad1d_ref(x, k - 1 - pr, pr, reflect)
    got = H.conv_cin1_ref(xp[:, 0], w[:, 0], sd[pfx + "conv.conv.bias"], 77, 1)
    _close(got, want.permute(0, 2, 1).contiguous())
    # a strided first-layer shape (the resampler's use of the same kernel): stride 2 over the same weights
    want2 = F.conv1d(xp, w, sd[pfx + "conv.conv.bias"], stride=2)
    _close(H.conv_cin1_ref(xp[:, 0], w[:, 0], sd[pfx + "conv.conv.bias"], want2.shape[-1], 2), want2.permute(0, 2, 1).contiguous())
    # last layer: ELU, then [B][n_filters][n] -> [B][1][n]
    last = OC.decoder_layout(cfg)[-1][0]
    pfx = f"decoder.model.{last}."
    w = OC.wn_weight(sd, pfx)
    assert tuple(w.shape) == (1, cfg.n_filters, cfg.last_kernel_size)
    x = torch.randn(3, cfg.n_filters, 61, generator=g).double()
    want = OC.sconv1d(sd, pfx, F.elu(x), 1, pad_mode)
    xp = H.pad1d_ref(x, k - 1 - pr, pr, reflect)                  # padding commutes with the ELU: ELU(0) = 0, and reflect copies values
    got = H.conv_few_out_ref(xp.permute(0, 2, 1).contiguous(), w.permute(0, 2, 1).contiguous(), sd[pfx + "conv.conv.bias"], True)
    _close(got, want.permute(0, 2, 1).contiguous())


def test_lstm_reference_equals_the_oracle_lstm():
    """Two layers of `lstm_ref` (the input projection done outside, as the codec does it with a GEMM; skip add on the second) against
    the oracle's torch.nn.LSTM + skip, both in float64."""
    cfg, _, sd = _tiny64(4)
    idx = [i for (i, kind, _) in OC.encoder_layout(cfg) if kind == "lstm"][0]
    pfx = f"encoder.model.{idx}."
    Cc = sd[pfx + "lstm.weight_hh_l0"].shape[1]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, Cc, 9, generator=g).double()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                          # the oracle builds its nn.LSTM in the default dtype
    try:
        want = OC.lstm(sd, pfx, x, cfg.lstm)
    finally:
        torch.set_default_dtype(old)
    assert want.dtype == torch.float64
    xt = x.permute(0, 2, 1)
    h = xt
    for l in range(cfg.lstm):
        gin = h @ sd[pfx + f"lstm.weight_ih_l{l}"].t() + sd[pfx + f"lstm.bias_ih_l{l}"] + sd[pfx + f"lstm.bias_hh_l{l}"]
        h = H.lstm_ref(gin, sd[pfx + f"lstm.weight_hh_l{l}"], skip=xt if l == cfg.lstm - 1 else None)
    _close(h.permute(0, 2, 1).contiguous(), want.contiguous())
    # the store epilogue is a plain ELU of the same values
    gin = xt @ sd[pfx + "lstm.weight_ih_l0"].t()
    a = H.lstm_ref(gin, sd[pfx + "lstm.weight_hh_l0"], skip=xt, out_elu=True)
    assert torch.equal(a, F.elu(H.lstm_ref(gin, sd[pfx + "lstm.weight_hh_l0"], skip=xt)))


def test_pack_whh_is_the_product_packing():
    """`pack_whh` (the layout behind ssrhip_lstm_args.w_packed) addresses: block [unit group][k-step], lane (k-slot, unit, gate), 4 floats."""
    Cc = 48
    whh = torch.arange(4 * Cc * Cc, dtype=torch.float32).view(4 * Cc, Cc)
    p = H.pack_whh(whh)
    assert tuple(p.shape) == (Cc // 4, Cc // 16, 4, 4, 4, 4)
    for (jb, ks_step, ks, u, q, comp) in ((0, 0, 0, 0, 0, 0), (3, 1, 2, 1, 3, 2), (11, 2, 3, 3, 1, 3)):
        assert p[jb, ks_step, ks, u, q, comp] == whh[q * Cc + 4 * jb + u, 16 * ks_step + 4 * ks + comp]


def test_rvq_references_equal_the_oracle_rvq():
    """Codes equal the oracle's fp32 search on every frame the margin filter keeps (and the filter keeps nearly all); the dequantiser's
    fp32 sum is the oracle's bit for bit."""
    cfg, sd, _ = _tiny64(5)
    g = torch.Generator().manual_seed(7)
    cb = torch.stack([sd[f"quantizer.vq.layers.{q}._codebook.embed"] for q in range(cfg.n_q)])
    emb = torch.randn(3, cfg.dimension, 53, generator=g) * 0.5
    want = OC.rvq_encode(sd, emb, cfg)
    codes, margins, err = H.rvq_encode_ref(emb.permute(0, 2, 1).contiguous(), cb)
    keep = H.rvq_kept_frames(margins, err)
    assert keep.float().mean() >= H.RVQ_MIN_KEPT and 0 < err < 1e-3
    assert torch.equal(codes.permute(0, 2, 1)[keep], want.permute(0, 2, 1)[keep])
    dec = OC.rvq_decode(sd, want, cfg)
    assert torch.equal(H.rvq_decode_ref(want, cb), dec.permute(0, 2, 1))


def test_rvq_reference_breaks_an_exact_tie_towards_the_first_index():
    emb, cb, _ = H.rvq_case(64, 64, 1, 4)
    cb[0, 40] = cb[0, 9]
    emb[:] = cb[0, 9]
    codes, margins, _ = H.rvq_encode_ref(emb, cb)
    assert (codes == 9).all() and (margins == 0).all()


@pytest.mark.parametrize("D,bins,n_q", H.RVQ_MFMA_SHAPES + H.RVQ_SCALAR_ONLY_SHAPES)
def test_rvq_kernel_test_shapes_keep_at_least_90_percent_of_their_frames(D, bins, n_q):
    """The GPU test compares codes only on frames whose smallest float64 margin is at least 8 x the fp32 score error of the case. If a
    change of seeds or shapes let that filter discard more than 10 % of a shape's frames (all T of the shape counted together), the GPU
    test would be checking little: caught here, without a GPU."""
    kept = total = 0
    for T in H.RVQ_TS:
        emb, cb, _ = H.rvq_case(D, bins, n_q, T)
        _, margins, err = H.rvq_encode_ref(emb, cb)
        keep = H.rvq_kept_frames(margins, err)
        kept, total = kept + int(keep.sum()), total + keep.numel()
    assert total == H.RVQ_B * sum(H.RVQ_TS)
    assert kept >= H.RVQ_MIN_KEPT * total, (kept, total)
