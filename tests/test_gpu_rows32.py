"""GPU: the 17..32-row decode step (16 utterances x CFG in one lock-step engine pass).

  * the two-panel GEMV (csrc/gemv_mfma32.hip) against torch, and bit for bit against 16-row launches of the same rows;
  * the attention kernels' paneled tiled output bit for bit against two 16-row calls;
  * whole generations on a model wide enough for the fused attention (d_model 1024, 16 heads): every utterance equals its batch-1 run;
  * the 830M shape: a 32-row engine equals two 16-row engines bit for bit (logits and tokens), and the oracle on the second panel.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import weights as W
from ssr_speech_amd.models.ssr import SSR_Speech
from oracle import lm as O

pytestmark = pytest.mark.gpu

PAGE = _lib.PAGE


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev(t):
    return t.to("cuda").contiguous()


def sync():
    torch.cuda.synchronize()


def _to_panels(t):
    """[B <= 32, Kw] -> the paneled tiled layout of include/ssrhip.h (SSRHIP_TILED_P): ceil(B/16) panels of [Kw/4][16][4]."""
    B, Kw = t.shape
    P = (B + 15) // 16
    out = torch.zeros(P, Kw // 4, 16, 4)
    for p in range(P):
        rows = t[16 * p:min(B, 16 * p + 16)]
        out[p, :, :rows.shape[0], :] = rows.reshape(rows.shape[0], Kw // 4, 4).permute(1, 0, 2)
    return out.reshape(-1)


def _from_panels(buf, B, Kw):
    P = (B + 15) // 16
    t = buf[:P * 16 * Kw].reshape(P, Kw // 4, 16, 4).permute(0, 2, 1, 3).reshape(P * 16, Kw)
    return t[:B]


# G, N, K, pro, act, epi, tiled: which 16-row kernel each shape reaches (w_tiled = 1 adds the k-step-pair forms where every workgroup owns
# one 8-row unit)
GEMV_CASES = [
    (1, 512, 2048, 1, 1, 0, 1),      # LayerNorm + ReLU, x in registers
    (1, 8192, 2048, 1, 1, 0, 1),     # FFN1 shape: two 16-row tiles per workgroup (cross-tile refills)
    (1, 4096, 2048, 1, 2, 0, 1),     # LayerNorm + GELU (head MLP 1)
    (1, 2048, 2048, 0, 0, 1, 1),     # out-projection + residual (k-step pairs with w_tiled)
    (1, 2048, 8192, 0, 0, 1, 1),     # FFN2 + residual: x streamed beside W (k-step pairs with w_tiled)
    (4, 72, 1024, 0, 0, 0, 1),       # grouped (head MLP 2)
    (1, 100, 1024, 0, 0, 0, 0),      # row-major x / y, N not a multiple of 8
    (1, 96, 8192, 0, 0, 1, 0),       # row-major, streamed x
    (1, 77, 128, 1, 1, 0, 0),        # row-major LayerNorm, one wave
    (1, 3072, 1024, 1, 0, 2, 1),     # LayerNorm + QKV with the KV append (shuffled page table)
]


class _Gemv:
    """One GEMV problem for B rows; `launch(rows)` runs ssrhip_gemv on a contiguous subset of the rows (padded to 16 for a 16-row
    launch of the second panel) and returns its outputs: y as [rows, G*N] and, for the QKV append, the whole KV pool."""

    def __init__(self, B, G, N, K, pro, act, epi, tiled, wt, seed):
        from ssr_speech_amd.engine import to_streaming_order
        g = torch.Generator().manual_seed(seed)
        self.B, self.G, self.N, self.K, self.pro, self.act, self.epi, self.tiled, self.wt = B, G, N, K, pro, act, epi, tiled, wt
        self.Wt = torch.randn(G, N, K, generator=g) / math.sqrt(K)
        self.bias = torch.randn(G, N, generator=g)
        self.x = torch.randn(B, G, K, generator=g) * 1.3 + 0.2
        self.y0 = torch.randn(B, G, N, generator=g)
        self.dW = dev(to_streaming_order(self.Wt if G > 1 else self.Wt[0]) if wt else (self.Wt if G > 1 else self.Wt[0]))
        self.db = dev(self.bias)
        if epi == 2:                                   # KV cache: 32 table rows x 2 pages, shuffled, + one spare page for padding rows
            self.hd, self.H = 64, K // 64
            self.max_pages = 2
            n_pages = 32 * self.max_pages
            self.spare = n_pages
            self.table = torch.randperm(n_pages, generator=g).to(torch.int32).view(32, self.max_pages)
            self.kv_pos = torch.randint(0, self.max_pages * PAGE, (32,), generator=g).to(torch.int32)
            self.pool0 = torch.randn(n_pages + 1, 1, 2, self.H, PAGE, self.hd, generator=g)

    def reference(self):
        xin = F.layer_norm(self.x, (self.K,), None, None, 1e-5) if self.pro == 1 else self.x
        ref = torch.stack([F.linear(xin[:, k], self.Wt[k], self.bias[k]) for k in range(self.G)], 1)
        ref = F.relu(ref) if self.act == 1 else (F.gelu(ref) if self.act == 2 else ref)
        return self.y0 + ref if self.epi == 1 else ref

    def launch(self, L, r0, n, pad16):
        G, N, K = self.G, self.N, self.K
        rows = 16 if pad16 else n
        x = torch.zeros(rows, G * K)
        x[:n] = self.x[r0:r0 + n].reshape(n, G * K)
        y0 = torch.zeros(rows, G * N)
        y0[:n] = self.y0[r0:r0 + n].reshape(n, G * N)
        a = _lib.GemvArgs()
        keep = []
        if self.tiled:
            dx = dev(_to_panels(x))
            a.x_stride = 0
        else:
            dx = dev(x)
            a.x_stride = G * K
        ytiled = self.tiled and self.epi != 2
        if self.epi == 2:
            dy = torch.zeros(rows, K, device="cuda")
            a.y_stride = K
            table = torch.full((rows, self.max_pages), self.spare, dtype=torch.int32)
            table[:n] = self.table[r0:r0 + n]
            kv_pos = torch.zeros(rows, dtype=torch.int32)
            kv_pos[:n] = self.kv_pos[r0:r0 + n]
            dpool, dtable, dpos = dev(self.pool0.clone()), dev(table), dev(kv_pos)
            keep += [dtable, dpos]
            a.kv = _lib.KV(dpool.data_ptr(), dtable.data_ptr(), self.max_pages, 1, self.H, self.hd)
            a.layer, a.kv_pos = 0, dpos.data_ptr()
        else:
            dy = dev(_to_panels(y0)) if ytiled else dev(y0)
            a.y_stride = 0 if ytiled else G * N
            dpool = None
        a.W, a.bias, a.x, a.y = self.dW.data_ptr(), self.db.data_ptr(), dx.data_ptr(), dy.data_ptr()
        a.B, a.N, a.K, a.groups = rows, N, K, G
        a.pro, a.act, a.epi, a.ln_eps = self.pro, self.act, self.epi, 1e-5
        a.x_tiled, a.y_tiled, a.w_tiled = self.tiled, int(ytiled), self.wt
        _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
        sync()
        y = _from_panels(dy.cpu().reshape(-1), rows, G * N) if ytiled else dy.cpu().reshape(rows, -1)
        return y[:n], (dpool.cpu() if dpool is not None else None)


@pytest.mark.parametrize("B", [17, 24, 32])
@pytest.mark.parametrize("G,N,K,pro,act,epi,tiled", GEMV_CASES)
@pytest.mark.parametrize("wt", [0, 1])
def test_gemv_32_rows_matches_torch_and_16_row_launches_bitwise(L, B, G, N, K, pro, act, epi, tiled, wt):
    p = _Gemv(B, G, N, K, pro, act, epi, tiled, wt, seed=B * 7 + N + K + 3 * pro + act + 11 * epi + wt)
    y32, pool32 = p.launch(L, 0, B, pad16=False)
    ya, pool_a = p.launch(L, 0, 16, pad16=False)
    yb, pool_b = p.launch(L, 16, B - 16, pad16=True)
    ref = p.reference()
    if epi == 2:
        qkv = ref[:, 0]
        torch.testing.assert_close(y32, qkv[:, :K], rtol=3e-5, atol=3e-5)
        for b in range(B):
            page, off = int(p.table[b, int(p.kv_pos[b]) // PAGE]), int(p.kv_pos[b]) % PAGE
            for which in (0, 1):
                got = pool32[page, 0, which, :, off, :].reshape(-1)
                torch.testing.assert_close(got, qkv[b, K * (1 + which):K * (2 + which)], rtol=3e-5, atol=3e-5)
        # every page but the spare one: the 32-row launch wrote exactly what the two 16-row launches wrote, and nothing else
        merged = pool_a.clone()
        for b in range(16, B):
            page, off = int(p.table[b, int(p.kv_pos[b]) // PAGE]), int(p.kv_pos[b]) % PAGE
            merged[page, :, :, :, off] = pool_b[page, :, :, :, off]
        assert torch.equal(pool32[:p.spare], merged[:p.spare])
    else:
        torch.testing.assert_close(y32, ref.reshape(B, G * N), rtol=3e-5, atol=3e-5)
    assert torch.equal(y32[:16], ya), "rows 0..15 differ from a 16-row launch"
    assert torch.equal(y32[16:], yb), "rows 16.. differ from a 16-row launch of those rows"


def test_gemv_32_rows_contract(L):
    p = _Gemv(32, 1, 512, 4096, 0, 0, 0, 1, 0, seed=1)
    a = _lib.GemvArgs()
    d = torch.zeros(32 * 4096, device="cuda")
    a.W, a.x, a.y = p.dW.data_ptr(), d.data_ptr(), d.data_ptr()
    a.B, a.N, a.K, a.groups, a.x_tiled, a.y_tiled = 32, 512, 4096, 1, 1, 1
    a.pro = 1
    assert L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()) != 0                 # LayerNorm on this path: K <= 2048
    assert b"2048" in L.ssrhip_last_error()
    a.pro, a.B = 0, 33
    assert L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()) != 0
    assert b"B=33" in L.ssrhip_last_error()


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_32_rows_tiled_equals_two_16_row_calls(L, hd):
    g = torch.Generator().manual_seed(320 + hd)
    H, n_layer, layer, R, max_pages = 2048 // hd, 2, 1, 32, 4
    D = H * hd
    n_pages = R * max_pages
    pool = dev(torch.randn(n_pages, n_layer, 2, H, PAGE, hd, generator=g))
    table = dev(torch.randperm(n_pages, generator=g).to(torch.int32).view(R, max_pages))
    lens = dev(torch.randint(1, max_pages * PAGE + 1, (R,), generator=g).to(torch.int32))
    q = dev(torch.randn(R, D, generator=g))
    part_o = torch.zeros(R * H * max_pages * hd, device="cuda")
    part_ml = torch.zeros(R * H * max_pages * 2, device="cuda")

    def args(r0, n):
        a = _lib.AttnArgs()
        a.q, a.q_stride = q.data_ptr() + 4 * r0 * D, 0
        a.kv = _lib.KV(pool.data_ptr(), table.data_ptr() + 4 * r0 * max_pages, max_pages, n_layer, H, hd)
        a.layer, a.row_seq, a.row_len, a.R, a.max_splits = layer, 0, lens.data_ptr() + 4 * r0, n, max_pages
        a.scale = 1.0 / math.sqrt(hd)
        a.part_o, a.part_ml = part_o.data_ptr() + 4 * r0 * H * max_pages * hd, part_ml.data_ptr() + 4 * r0 * H * max_pages * 2
        a.out_tiled = 1
        return a

    for entry in ("rows", "combine"):
        out32 = torch.full((R * D,), float("nan"), device="cuda")
        out16 = [torch.full((16 * D,), float("nan"), device="cuda") for _ in range(2)]
        if entry == "combine":
            _lib.check(L.ssrhip_attn_decode(C.byref(args(0, R)), _lib.stream_ptr()))
        fn = L.ssrhip_attn_rows if entry == "rows" else L.ssrhip_attn_combine
        _lib.check(fn(C.byref(args(0, R)), out32.data_ptr(), _lib.stream_ptr()))
        for p in range(2):
            _lib.check(fn(C.byref(args(16 * p, 16)), out16[p].data_ptr(), _lib.stream_ptr()))
        sync()
        assert torch.equal(out32[:16 * D], out16[0]), entry
        assert torch.equal(out32[16 * D:], out16[1]), entry
        # and the panels hold the right rows: row 20 of the 32-row output is the attention of query 20
        r, h = 20, 1
        ln = int(lens[r])
        ks = torch.cat([pool[table[r, i], layer, 0, h] for i in range((ln + PAGE - 1) // PAGE)])[:ln]
        vs = torch.cat([pool[table[r, i], layer, 1, h] for i in range((ln + PAGE - 1) // PAGE)])[:ln]
        ref = torch.softmax((ks @ q[r, h * hd:(h + 1) * hd]) / math.sqrt(hd), 0) @ vs
        got = _from_panels(out32.cpu(), R, D)[r, h * hd:(h + 1) * hd]
        torch.testing.assert_close(got, ref.cpu(), rtol=2e-5, atol=2e-5)
    a = args(0, 33)
    assert L.ssrhip_attn_rows(C.byref(a), out32.data_ptr(), _lib.stream_ptr()) != 0    # tiled output: R <= 32


# ------------------------------------------------------------------------------------------ whole generations
def _model(args, seed):
    m = SSR_Speech(args)
    m.load_state_dict(W.lm_state_dict(args, seed=seed))
    return m.to("cuda").eval()


def _utts(g, n, lens=None):
    out = []
    for i in range(n):
        L, T = lens[i] if lens else (8 + i % 7, 20 + (37 * i) % 120)
        out.append(dict(x=torch.randint(0, 30, (1, L), generator=g), y=torch.randint(0, 64, (1, T, 4), generator=g),
                        mask_interval=torch.LongTensor([[[T, T]]])))
    return out


def _batch1(m, u, seed, kw):
    torch.manual_seed(seed)
    L = u["x"].shape[1]
    return m.inference(u["x"].cuda(), torch.LongTensor([L]), u["x"].cuda(), torch.LongTensor([L]), u["y"].cuda(), u["y"].cuda(),
                       u["mask_interval"].cuda(), kvcache=1, **kw)


def _wide_model(seed):
    args = W.lm_args_tiny(d_model=1024, nhead=16, layers=2, vocab=64)
    return args, _model(args, seed)


def _kw(greedy, cfg=True):
    kw = dict(top_k=1, top_p=1.0) if greedy else dict(top_k=12, top_p=0.9)
    kw.update(temperature=1.0, stop_repetition=2, silence_tokens=[3, 7, 11], cfg_coef=1.5 if cfg else 1.0, cfg_stride=2, aug_text=cfg)
    return kw


@pytest.mark.parametrize("greedy", [True, False])
def test_sixteen_utterances_cfg_32_rows_full_generation_equals_batch1(greedy):
    """16 utterances of different lengths x CFG = 32 rows in one engine (two GEMV panels, 32 x 16 (row, head) pairs of the fused
    attention), run to completion; every utterance equals its batch-1 run seeded seed + i."""
    args, m = _wide_model(53)
    g = torch.Generator().manual_seed(22)
    utts = _utts(g, 16)
    utts[5]["mask_interval"] = torch.LongTensor([[[10, 19]]])
    kw = _kw(greedy)
    batch = m.inference_batch(utts, seed=400, group=16, **kw)
    eng = next(e for e in m._engines.values())
    assert eng.B == 32 and eng.x.shape[0] == 32
    for i, u in enumerate(utts):
        one = _batch1(m, u, 400 + i, kw)
        assert torch.equal(batch[i][0], one[0]) and torch.equal(batch[i][1], one[1]) and batch[i][2] == one[2], i


def test_twenty_utterances_group16_with_refill_equals_group8():
    args, m = _wide_model(54)
    g = torch.Generator().manual_seed(23)
    utts = _utts(g, 20)
    kw = _kw(True)
    r16 = m.inference_batch(utts, seed=500, group=16, **kw)
    assert any(e.B == 32 and e.n_refills == 4 for e in m._engines.values())
    r8 = m.inference_batch(utts, seed=500, group=8, **kw)
    for i in range(20):
        assert torch.equal(r16[i][0], r8[i][0]) and torch.equal(r16[i][1], r8[i][1]) and r16[i][2] == r8[i][2], i


def test_dp_generate_group16_equals_inference_batch_group8():
    from ssr_speech_amd import dp
    args, m = _wide_model(55)
    g = torch.Generator().manual_seed(24)
    utts = _utts(g, 18)
    kw = _kw(True)
    toks, (mine, outs) = dp.generate(m, utts, seed=11, group=16, **kw)
    ref = m.inference_batch(utts, seed=11, group=8, **kw)
    assert mine == list(range(18)) and len(toks) == 18
    for i in range(18):
        assert torch.equal(toks[i], ref[i][0][0]), i


@pytest.mark.parametrize("n_utt,cfg", [(9, True), (17, False)])
def test_odd_row_counts_equal_batch1(n_utt, cfg):
    """18 rows (9 utterances x CFG) and 17 rows (17 utterances, no CFG): a partly filled second panel."""
    args, m = _wide_model(56)
    g = torch.Generator().manual_seed(25 + n_utt)
    utts = _utts(g, n_utt)
    kw = _kw(True, cfg)
    batch = m.inference_batch(utts, seed=600, group=n_utt, **kw)
    eng = next(e for e in m._engines.values())
    assert eng.B == n_utt * (2 if cfg else 1)
    for i, u in enumerate(utts):
        one = _batch1(m, u, 600 + i, kw)
        assert torch.equal(batch[i][0], one[0]) and batch[i][2] == one[2], i


def test_config4_830m_32_rows_equal_two_16_row_engines_and_the_oracle():
    """16 utterances x CFG at the 830M shape, 5 greedy steps: per-step post-edit logits and tokens of the 32-row engine are bit-identical
    to the same utterances in two 8-utterance engines; utterances 8..15 (the second panel) also match the oracle run on the CPU."""
    from ssr_speech_amd import layout as LY
    from ssr_speech_amd.engine import DecodeEngine, DecodeKnobs, LMWeightsArena
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    args = W.lm_args_830m()
    sd_gpu = W.lm_state_dict(args, seed=0, device="cuda")
    arena = LMWeightsArena(args, sd_gpu, torch.device("cuda"))
    sd_cpu = O.reference_params({k: v.cpu() for k, v in sd_gpu.items()})
    gen = torch.Generator().manual_seed(79)
    n_utt, steps = 16, 5
    rows, cols, knobs, utts = [], [], [], []
    for u in range(n_utt):
        L, N = 18 + 2 * u, 150 + 5 * u
        x = torch.randint(0, 100, (1, L), generator=gen)
        y = torch.randint(0, 2048, (1, N, 4), generator=gen)
        unc = torch.randint(0, 101, (1, L), generator=gen)
        mi = torch.LongTensor([[[N, N]]])
        cated, _, num_task, _ = LY.build_layout(y[0].T.numpy(), mi[0].numpy(), args)
        rows += [x[0].numpy(), unc[0].numpy()]
        cols.append(cated)
        knobs.append(DecodeKnobs(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2, cfg_coef=1.5, cfg_stride=2, use_cfg=True,
                                 text_len=L, n_spans=num_task, seed=u))
        utts.append((x, y, unc, mi))

    def run(lo, hi):
        eng = DecodeEngine(arena, hi - lo, True, 512, 64, debug_logits=True)
        eng.start(rows[2 * lo:2 * hi], cols[lo:hi], knobs[lo:hi])
        logits = []
        for _ in range(steps):
            eng.decode(1, use_graph=True)
            logits.append(eng.dbg_logits.clone())
        torch.cuda.synchronize()
        out = (torch.stack(logits, 1).cpu(), eng.generated[:, :steps].cpu())
        assert eng.B == 2 * (hi - lo)
        eng.close()
        return out

    lg32, tok32 = run(0, 16)
    lga, toka = run(0, 8)
    lgb, tokb = run(8, 16)
    assert torch.equal(tok32[:8], toka) and torch.equal(tok32[8:], tokb)
    assert torch.equal(lg32[:8], lga), "panel 0 logits differ from a 16-row engine"
    assert torch.equal(lg32[8:], lgb), "panel 1 logits differ from a 16-row engine"
    worst = 0.0
    for u in range(8, 16):
        x, y, unc, mi = utts[u]
        trace = {}
        O.inference(sd_cpu, args, x, y, mi, uncond_x=unc, max_steps=steps, trace=trace, top_k=1, top_p=1.0, temperature=1.0, stop_repetition=2,
                    kvcache=1, cfg_coef=1.5, cfg_stride=2, aug_text=True)
        assert np.array_equal(tok32[u].numpy(), torch.stack(trace["samples"]).numpy()), u
        err = float(np.abs(lg32[u, steps - 1].numpy() - torch.stack(trace["edited_logits"]).numpy()[steps - 1]).max())
        worst = max(worst, err)
        assert err < 5e-4, (u, err)
    print(f"830M x 32 rows: max |logit diff| vs oracle at step {steps} (panel 1): {worst:.2e}")
