"""One fixed `BatchDecodeStream` case and one fixed `WMDecodeStream` case, run through the public entries only: what
tests/golden/stream_bits_before_wmstream_batch.npz was recorded with on the commit before the batched watermarked stream, and what
tests/test_gpu_wmstream_batch.py runs again to show that both streams kept their bits."""
import numpy as np
import torch

GOLDEN = "stream_bits_before_wmstream_batch.npz"


def golden_streams() -> dict:
    """-> {"batch0" .. "batch2": the items of the batched stream, "wm": the watermarked stream} as float32 arrays"""
    import ssr_speech_amd  # noqa: F401
    from ssr_speech_amd import weights as W
    from ssr_speech_amd.codec.wmencodec import WMEncodecModel
    cfg = W.CodecConfig(dimension=64, n_filters=8, ratios=(8, 5, 4, 2), bins=64)
    m = WMEncodecModel(cfg, W.codec_state_dict(cfg, seed=21), "cuda")
    out = {}
    # BatchDecodeStream: three items, polls of 16 frames; item 0 ends inside the first poll, item 2 in the second, item 1 in the third
    prompts, new = (5, 19, 40), (2, 37, 21)
    g = torch.Generator().manual_seed(31)
    codes = [torch.randint(0, cfg.bins, (cfg.n_q, p + n), generator=g) for p, n in zip(prompts, new)]
    st = m.decode_stream_batch(prompts, max(new) + 2)
    st.push_prompts([c[:, :p] for c, p in zip(codes, prompts)])
    done, got = [0, 0, 0], [[], [], []]
    while not all(st.ended):
        take = [min(16, new[u] - done[u]) for u in range(3)]
        ended = [not st.ended[u] and new[u] - done[u] <= 16 for u in range(3)]
        for u, o in enumerate(st.advance(take, ended, codes=[codes[u][:, prompts[u] + done[u]: prompts[u] + done[u] + take[u]] for u in range(3)])):
            got[u].append(o.clone())
            done[u] += take[u]
    for u in range(3):
        out[f"batch{u}"] = torch.cat(got[u], -1).cpu().numpy()
    # WMDecodeStream: 61 frames with random labels and a random kept-audio track, 20 of them an un-emitted prefix, pushes of 7
    T, hop = 61, cfg.hop
    g = torch.Generator().manual_seed(261)
    wc = torch.randint(0, cfg.bins, (1, cfg.n_q, T), generator=g).cuda()
    wl = torch.randint(0, 2, (1, T), generator=g).cuda()
    ww = (torch.randn(1, 1, T * hop, generator=g) * 0.3).cuda()
    ws = m.wmdecode_stream(T + 3)
    ws.push(wc[..., :20], wl[0, :20], ww[..., : 20 * hop], emit=False)
    chunks = [ws.push(wc[..., t: t + 7], wl[0, t: t + 7], ww[..., t * hop: (t + 7) * hop]).clone() for t in range(20, T, 7)] + [ws.finish().clone()]
    out["wm"] = torch.cat(chunks, -1).cpu().numpy()
    assert out["wm"].shape == (1, 1, 41 * hop) and all(out[f"batch{u}"].shape == (1, 1, new[u] * hop) for u in range(3))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
