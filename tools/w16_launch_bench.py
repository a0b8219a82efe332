"""Per-launch time of the decode step's GEMV shapes, fp32 weights (`ssrhip_gemv`) against packed bf16 weights (`ssrhip_gemv_w16`), the
way the step runs them: CHAIN launches of one shape are captured into one graph on one stream (so they follow each other like the
dependent launches of a step), the graph is replayed and the elapsed time divided by the launches. Every launch of a chain streams its own
matrix (the chain's weights exceed the 256 MB of last-level cache several times over), activations stay in L2 as in the step.
Beside each figure: the project's chain floor `2.6 us + bytes / 7.3 TB/s` (DESIGN.md Part I.5) for that launch's weight bytes.

    python tools/w16_launch_bench.py [--rows 2] [--chain 16] [--replays 30] [--out FILE]
    SSRHIP_GEMV_W16_DEPTH=4 python tools/w16_launch_bench.py        (the ring-of-4 form of the straight-line kernel)
`--rows 5..16` measures the matrix-core step's launches instead (DESIGN.md Part I.11): the fp32 streaming-order copy (`ssrhip_gemv`,
w_tiled) against the packed bf16 streaming-order copy (`ssrhip_gemv_wt16`) with 8 loads in flight per wave (the default) and with 16
(`SSRHIP_GEMVM_W16_DEPTH=16`, set by the tool for that arm), activations in the tiled layout as the step keeps them.
    python tools/w16_launch_bench.py --rows 16 --out profiles/wt16_launch_bench_rows16.json
At these rows the masters are e4m3-valued (codes * scale, bf16-representable), and a fourth arm streams the 1-byte codes in
SSRHIP_WT8_INDEX order with their scales (`ssrhip_gemv_wt8`, DESIGN.md Part I.22). Beside it: its chain floor
`2.6 us + (codes + scales) / 7.3 TB/s`, the matrix-core time of the launch `2 * 16 * N * K flop / 157.3 TFLOP/s` (the panel is multiplied
whole), and which of the two is larger (`wt8_bound_by`: "bytes" or "matrix").
    python tools/w16_launch_bench.py --rows 16 --out profiles/wt8_launch_bench_rows16.json
`--rows 17..32` measures the two-panel step's launches (DESIGN.md Part I.12): the fp32 streaming-order copy against the same packed copy
through `ssrhip_gemv_wt32`, two panels of tiled activations; beside the byte floors it prints the matrix-core time of the launch,
`2 * rows_padded * N * K flop / 157.3 TFLOP/s` (rows_padded = 32: both panels are multiplied whole).
    python tools/w16_launch_bench.py --rows 32 --out profiles/wt32_launch_bench_rows32.json
`--stream w8` (1, 2 or 4 rows; DESIGN.md Part I.18) measures the e4m3 weight stream (`ssrhip_gemv_w8`: 1-byte codes and a power-of-two
scale per row) in the same process: the fp32 launch on the masters codes * scale, the bf16 stream on the same (bf16-representable)
masters, and the e4m3 stream with the straight-line form's ring at 2, 4 and every unit (`SSRHIP_GEMV_W8_DEPTH` = 2 | 4 | 8, set by the
tool per arm) and with the generic form only (0); floor of the 1-byte launch = 2.6 us + (codes + scales) / 7.3 TB/s.
    python tools/w16_launch_bench.py --stream w8 --rows 2 --out profiles/w8_launch_bench_rows2.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import _lib  # noqa: E402
from ssr_speech_amd.engine import PACKED_ORDERS, W16_STREAMS, e4m3_master, quantize_e4m3, to_streaming_order, to_w8_order, to_wt8_order  # noqa: E402

# name, G, N, K, prologue, activation, epilogue: the six launches of the 830M step
SHAPES = [
    ("ln1+qkv", 1, 6144, 2048, _lib.PRO_LAYERNORM, _lib.ACT_NONE, _lib.EPI_QKV_APPEND),
    ("merge+out", 1, 2048, 2048, _lib.PRO_ATTN_COMBINE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    ("ln2+ffn1", 1, 8192, 2048, _lib.PRO_LAYERNORM, _lib.ACT_RELU, _lib.EPI_STORE),
    ("ffn2", 1, 2048, 8192, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_RESIDUAL),
    ("lnf+head1", 1, 4096, 2048, _lib.PRO_LAYERNORM, _lib.ACT_GELU_ERF, _lib.EPI_STORE),
    ("head2", 4, 2056, 1024, _lib.PRO_NONE, _lib.ACT_NONE, _lib.EPI_STORE),
]
H, HD, MAX_PAGES = 16, 128, 6


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2, choices=[1, 2, 4] + list(range(5, 33)))
    ap.add_argument("--chain", type=int, default=16)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stream", default="w16", choices=["w16", "w8"], help="w16: the bf16 stream of --rows (default); w8: the e4m3 stream (<= 4 rows)")
    opt = ap.parse_args(argv)
    if opt.stream == "w8" and opt.rows > 4:
        ap.error("--stream w8 exists for 1, 2 or 4 rows")
    w8 = opt.stream == "w8"
    W8_DEPTHS = {"w8_depth2": "2", "w8_depth4": "4", "w8_depth8": "8", "w8_generic": "0"}
    L = _lib.lib()
    B, dev = opt.rows, torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    st = next(s for s in W16_STREAMS if s.lo <= B <= s.hi)        # the bf16 stream of these rows
    mc = st.order == "wt16"                                       # the matrix-core step: tiled activations, streaming-order weights
    wt8 = st.name == "wt16"                                       # 5..16 rows: the e4m3 stream of the matrix-core step is a fourth arm
    forms = ("fp32", st.name) + (("wt16_depth16", "wt8") if wt8 else ()) + (tuple(W8_DEPTHS) if w8 else ())
    to_packed, gemv_packed = PACKED_ORDERS[st.order][0], getattr(L, "ssrhip_gemv_" + st.name)
    xrows = 32 if B > 16 else 16 if mc else B                     # (tiled: 16 columns per panel, any values)
    for name, G, N, K, pro, act, epi in SHAPES:
        if mc and pro == _lib.PRO_ATTN_COMBINE:
            pro = _lib.PRO_NONE                                   # at 5..32 rows the split-KV merge is a launch of its own
        ny = K if epi == _lib.EPI_QKV_APPEND else G * N
        masters = [(torch.randn(G, N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16).float() for _ in range(opt.chain)]
        if w8 or wt8:                                             # masters = codes * scale: bf16-representable, so the bf16 arm streams the same values
            quant = [quantize_e4m3(m) for m in masters]
            masters = [e4m3_master(q, sc) for q, sc in quant]
            packed8, scales = [(to_wt8_order if wt8 else to_w8_order)(q) for q, _ in quant], [sc.contiguous() for _, sc in quant]
            del quant
        packed = [to_packed(m) for m in masters]
        if mc:
            masters = [to_streaming_order(m) for m in masters]
        bias = torch.randn(G, N, device=dev, generator=g)
        x = torch.randn(xrows, G * K, device=dev, generator=g)
        y = torch.zeros(xrows, ny, device=dev)
        pool = torch.zeros(B * MAX_PAGES + 1, 1, 2, H, _lib.PAGE, HD, device=dev)
        table = torch.arange(B * MAX_PAGES, dtype=torch.int32, device=dev).view(B, MAX_PAGES)
        pos = torch.full((B,), 600, dtype=torch.int32, device=dev)
        lens = torch.full((B,), 601, dtype=torch.int32, device=dev)
        part_o = torch.randn(B, H, MAX_PAGES, HD, device=dev, generator=g)
        part_ml = torch.rand(B, H, MAX_PAGES, 2, device=dev, generator=g) + 0.5

        def args_of(i):
            a = _lib.GemvArgs()
            a.W, a.bias, a.x, a.y = masters[i].data_ptr(), bias.data_ptr(), x.data_ptr(), y.data_ptr()
            a.B, a.N, a.K, a.groups, a.x_stride, a.y_stride = B, N, K, G, G * K, ny
            a.pro, a.act, a.epi, a.ln_eps = pro, act, epi, 1e-5
            if mc:
                a.x_tiled, a.y_tiled, a.w_tiled = 1, int(epi != _lib.EPI_QKV_APPEND), 1
            if epi == _lib.EPI_QKV_APPEND:
                a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), MAX_PAGES, 1, H, HD)
                a.layer, a.kv_pos = 0, pos.data_ptr()
            if pro == _lib.PRO_ATTN_COMBINE:
                a.x = 0
                a.part_o, a.part_ml, a.max_splits, a.row_len = part_o.data_ptr(), part_ml.data_ptr(), MAX_PAGES, lens.data_ptr()
                a.kv = _lib.KV(0, 0, MAX_PAGES, 1, H, HD)
            return a

        us = {}
        for form in forms:
            if form == "wt16_depth16":
                os.environ["SSRHIP_GEMVM_W16_DEPTH"] = "16"           # read at every launch, i.e. while the chain is captured
            else:
                os.environ.pop("SSRHIP_GEMVM_W16_DEPTH", None)
            if form in W8_DEPTHS:
                os.environ["SSRHIP_GEMV_W8_DEPTH"] = W8_DEPTHS[form]  # read at every launch too
            else:
                os.environ.pop("SSRHIP_GEMV_W8_DEPTH", None)

            def chain():
                for i in range(opt.chain):
                    a = args_of(i)
                    if form == "fp32":
                        _lib.check(L.ssrhip_gemv(C.byref(a), _lib.stream_ptr()))
                    elif form == "wt8":
                        rc = L.ssrhip_gemv_wt8(C.byref(a), packed8[i].data_ptr(), scales[i].data_ptr(), _lib.stream_ptr())
                        assert rc == 0, (name, rc, L.ssrhip_last_error())
                    elif form in W8_DEPTHS:
                        rc = L.ssrhip_gemv_w8(C.byref(a), packed8[i].data_ptr(), scales[i].data_ptr(), _lib.stream_ptr())
                        assert rc == 0, (name, rc, L.ssrhip_last_error())
                    else:
                        rc = gemv_packed(C.byref(a), packed[i].data_ptr(), _lib.stream_ptr())
                        assert rc == 0, (name, rc, L.ssrhip_last_error())
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                chain()                                           # module load, first-launch costs
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                chain()
            for _ in range(3):
                graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            best = None
            for _ in range(3):
                e0.record()
                for _ in range(opt.replays):
                    graph.replay()
                e1.record()
                e1.synchronize()
                t = 1000.0 * e0.elapsed_time(e1) / (opt.replays * opt.chain)
                best = t if best is None else min(best, t)
            us[form] = best
            del graph
        floor = lambda nbytes: 2.6 + nbytes / 7.3e6                # us: 7.3 TB/s = 7.3e6 bytes per us
        nw = G * N * K
        os.environ.pop("SSRHIP_GEMVM_W16_DEPTH", None)
        os.environ.pop("SSRHIP_GEMV_W8_DEPTH", None)
        row = dict(shape=name, G=G, N=N, K=K, rows=B, fp32_us=round(us["fp32"], 2), fp32_floor_us=round(floor(4 * nw), 2),
                   fp32_TBps=round(4 * nw / us["fp32"] / 1e6, 2), w16_floor_us=round(floor(2 * nw), 2))
        if w8:
            row["w8_floor_us"] = round(floor(nw + 4 * G * N), 2)
        for form in forms[1:]:
            row[form + "_us"] = round(us[form], 2)
            row[form + "_TBps"] = round(((nw + 4 * G * N) if form in W8_DEPTHS or form == "wt8" else 2 * nw) / us[form] / 1e6, 2)
        if wt8:                                                  # one panel of fp32 MFMA work against 1-byte weights: bytes or flops?
            row["wt8_floor_us"] = round(floor(nw + 4 * G * N), 2)
            row["mfma_us"] = round(2 * 16 * nw / 157.3e6, 2)
            row["wt8_bound_by"] = "matrix" if row["mfma_us"] > (nw + 4 * G * N) / 7.3e6 else "bytes"
        if B > 16:                                               # two panels of fp32 MFMA work: is the launch bound by bytes or by flops?
            row["mfma_us"] = round(2 * 32 * nw / 157.3e6, 2)     # us at 157.3 TFLOP/s = 157.3e6 flop per us
        rows.append(row)
        print(json.dumps(rows[-1]), flush=True)
        del masters, packed
        if w8 or wt8:
            del packed8, scales
        torch.cuda.empty_cache()
    out = dict(tool="tools/w16_launch_bench.py", stream=opt.stream, chain=opt.chain, replays=opt.replays, depth_knob=os.environ.get("SSRHIP_GEMV_W16_DEPTH", "unset"), shapes=rows)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
