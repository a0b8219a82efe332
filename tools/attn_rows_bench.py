"""Per-launch time of the fused decode attention of the 5..32-row step over an fp32 KV cache (`ssrhip_attn_rows`) against the bf16 KV cache
(`ssrhip_attn_rows_kv16`, DESIGN.md Part I.14) with 2 and with 4 pages in flight (`SSRHIP_ATTN_KV16_DEPTH`, set by the tool per arm), the
way the step runs them: the 16 launches over the 16 layers of ONE 830M-shaped pool (16 heads x 128) are captured into one graph on one
stream, the graph is replayed and the elapsed time divided by the launches. Every launch reads its own layer's K / V once (a layer of 16
rows at context 520 is 136 MB in fp32: the chain exceeds the 256 MB last-level cache several times over). Cases: R = 16 and 32 rows,
context 520 and 700. The arms alternate over `--rounds`; per arm the median us per launch and the spread (max - min) over the rounds,
beside the project's chain floor `2.6 us + bytes / 7.3 TB/s` (DESIGN.md Part I.5) for that launch's K / V bytes.

    python tools/attn_rows_bench.py [--rounds 5] [--replays 20] [--out profiles/kv16_attn_rows_bench.json]

`--group` measures prompt sharing instead (DESIGN.md Part I.15): `ssrhip_attn_rows` against `ssrhip_attn_rows_group` on the SAME aliased
page table, at 32 rows, for every chunk size the kernel is built for (`SSRHIP_ATTN_GROUP_MEMBERS` = 2, 4, 8, set by the tool per arm, the
chunk arrays cut to match). Layouts: `16+16` = the even rows share their first `--shared_pages` pages and the odd rows share nothing
(16 samples under `aug_text`), `2x16` = the odd rows are a second group. The outputs of every arm are compared bit for bit first.

    python tools/attn_rows_bench.py --group [--contexts 520] [--shared_pages 3] [--out profiles/share_attn_rows_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import _lib  # noqa: E402

H, HD, N_LAYER = 16, 128, 16
ARMS = (("fp32", None), ("kv16_depth2", "2"), ("kv16_depth4", "4"))


GROUP_ARMS = (("rows", None), ("group_m2", 2), ("group_m4", 4), ("group_m8", 8))


def group_main(opt, L):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    D, R, PAGE = H * HD, 32, _lib.PAGE
    cases = []
    for ctx in (int(v) for v in opt.contexts.split(",")):
        for layout in ("16+16", "2x16"):
            max_pages = (ctx + PAGE - 1) // PAGE
            ns = min(opt.shared_pages, (ctx - 1) // PAGE)
            groups = [list(range(0, R, 2))] + ([list(range(1, R, 2))] if layout == "2x16" else [])
            own = [max_pages - ns if any(r in gr for gr in groups) else max_pages for r in range(R)]
            n_pages = sum(own) + ns * len(groups)
            perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(ctx)).tolist()
            table = torch.full((R, max_pages), n_pages, dtype=torch.int32)
            for gr in groups:
                for i in range(ns):
                    table[gr, i] = perm.pop()
            for r in range(R):
                first = max_pages - own[r]
                for i in range(own[r]):
                    table[r, first + i] = perm.pop()
            table = table.to(dev)
            pool = torch.empty((n_pages + 1) * N_LAYER * 2 * H * PAGE * HD, device=dev).normal_(generator=g)
            lens = torch.full((R,), ctx, dtype=torch.int32, device=dev)
            q = torch.randn(R, D, device=dev, generator=g)
            outs = {name: torch.zeros(32 * D, device=dev) for name, _ in GROUP_ARMS}
            arrays = {}
            for name, m in GROUP_ARMS:
                head, nsh = list(range(R)), [0] * R
                for gr in groups if m else []:
                    for c0 in range(0, len(gr), m):
                        for r in gr[c0:c0 + m]:
                            head[r] = gr[c0]
                        nsh[gr[c0]] = ns
                arrays[name] = (torch.tensor(head, dtype=torch.int32, device=dev), torch.tensor(nsh, dtype=torch.int32, device=dev))

            def chain(name, m):
                for layer in range(N_LAYER):
                    a = _lib.AttnArgs()
                    a.q, a.q_stride = q.data_ptr(), 0
                    a.kv = _lib.KV(pool.data_ptr(), table.data_ptr(), max_pages, N_LAYER, H, HD)
                    a.layer, a.row_seq, a.row_len = layer, 0, lens.data_ptr()
                    a.R, a.max_splits, a.scale, a.out_tiled = R, max_pages, 1.0 / math.sqrt(HD), 1
                    if m is None:
                        _lib.check(L.ssrhip_attn_rows(C.byref(a), outs[name].data_ptr(), _lib.stream_ptr()))
                    else:
                        _lib.check(L.ssrhip_attn_rows_group(C.byref(a), arrays[name][0].data_ptr(), arrays[name][1].data_ptr(), outs[name].data_ptr(),
                                                            _lib.stream_ptr()))

            graphs = {}
            side = torch.cuda.Stream()
            for name, m in GROUP_ARMS:
                if m is None:
                    os.environ.pop("SSRHIP_ATTN_GROUP_MEMBERS", None)
                else:
                    os.environ["SSRHIP_ATTN_GROUP_MEMBERS"] = str(m)  # read at every launch, i.e. while the chain is captured
                with torch.cuda.stream(side):
                    chain(name, m)
                side.synchronize()
                graphs[name] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[name], stream=side):
                    chain(name, m)
                for _ in range(3):
                    graphs[name].replay()
            os.environ.pop("SSRHIP_ATTN_GROUP_MEMBERS", None)
            torch.cuda.synchronize()
            same = all(torch.equal(outs["rows"], outs[name]) for name, _ in GROUP_ARMS)   # the last layer's output of every arm
            us = {name: [] for name, _ in GROUP_ARMS}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(opt.rounds):
                for name, _ in GROUP_ARMS:
                    e0.record()
                    for _ in range(opt.replays):
                        graphs[name].replay()
                    e1.record()
                    e1.synchronize()
                    us[name].append(1000.0 * e0.elapsed_time(e1) / (opt.replays * N_LAYER))
            row = dict(rows=R, context=ctx, layout=layout, shared_pages=ns, pages_per_row=max_pages, bit_identical=bool(same))
            for name, m in GROUP_ARMS:
                # K / V bytes the launch must read at least: every unshared position once per row, a shared page once per chunk
                chunks = sum((len(gr) + m - 1) // m for gr in groups) if m else sum(len(gr) for gr in groups)
                shared_rows = sum(len(gr) for gr in groups)
                nbytes = ((R * ctx - shared_rows * ns * PAGE) + chunks * ns * PAGE) * 2 * D * 4
                med = statistics.median(us[name])
                row[name] = dict(us_per_launch_median=round(med, 2), spread_us=round(max(us[name]) - min(us[name]), 2),
                                 all_us=[round(v, 2) for v in us[name]], kv_MB=round(nbytes / 1e6, 1), floor_us=round(2.6 + nbytes / 7.3e6, 2))
            cases.append(row)
            print(json.dumps(row), flush=True)
            del graphs, pool
            torch.cuda.empty_cache()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/attn_rows_bench.py --group", rounds=opt.rounds, replays=opt.replays, chain=N_LAYER, cases=cases), indent=1) + "\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", action="store_true", help="prompt sharing: ssrhip_attn_rows against ssrhip_attn_rows_group at 32 rows")
    ap.add_argument("--shared_pages", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rows", default="16,32")
    ap.add_argument("--contexts", default="520,700")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(argv)
    L = _lib.lib()
    if opt.group:
        return group_main(opt, L)
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    D = H * HD
    cases = []
    for R in (int(v) for v in opt.rows.split(",")):
        for ctx in (int(v) for v in opt.contexts.split(",")):
            max_pages = (ctx + _lib.PAGE - 1) // _lib.PAGE
            n_pages = R * max_pages
            pool16 = torch.empty((n_pages + 1) * N_LAYER * 2 * H * _lib.PAGE * HD, dtype=torch.bfloat16, device=dev)
            pool16.normal_(generator=g)
            pool32 = pool16.float()                                   # the widened pool: the same values
            table = torch.randperm(n_pages, device=dev, generator=g).to(torch.int32).view(R, max_pages)
            lens = torch.full((R,), ctx, dtype=torch.int32, device=dev)
            q = torch.randn(R, D, device=dev, generator=g)
            out = torch.zeros(32 * D, device=dev)

            def chain(kv16):
                for layer in range(N_LAYER):
                    a = _lib.AttnArgs()
                    a.q, a.q_stride = q.data_ptr(), 0
                    a.kv = _lib.KV((pool16 if kv16 else pool32).data_ptr(), table.data_ptr(), max_pages, N_LAYER, H, HD)
                    a.layer, a.row_seq, a.row_len = layer, 0, lens.data_ptr()
                    a.R, a.max_splits, a.scale, a.out_tiled = R, max_pages, 1.0 / math.sqrt(HD), 1
                    fn = L.ssrhip_attn_rows_kv16 if kv16 else L.ssrhip_attn_rows
                    _lib.check(fn(C.byref(a), out.data_ptr(), _lib.stream_ptr()))

            graphs = {}
            side = torch.cuda.Stream()
            for name, depth in ARMS:
                if depth is None:
                    os.environ.pop("SSRHIP_ATTN_KV16_DEPTH", None)
                else:
                    os.environ["SSRHIP_ATTN_KV16_DEPTH"] = depth      # read at every launch, i.e. while the chain is captured
                with torch.cuda.stream(side):
                    chain(depth is not None)                          # module load, first-launch costs
                side.synchronize()
                graphs[name] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[name], stream=side):
                    chain(depth is not None)
                for _ in range(3):
                    graphs[name].replay()
            os.environ.pop("SSRHIP_ATTN_KV16_DEPTH", None)
            torch.cuda.synchronize()
            us = {name: [] for name, _ in ARMS}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(opt.rounds):
                for name, _ in ARMS:                                  # alternating arms
                    e0.record()
                    for _ in range(opt.replays):
                        graphs[name].replay()
                    e1.record()
                    e1.synchronize()
                    us[name].append(1000.0 * e0.elapsed_time(e1) / (opt.replays * N_LAYER))
            row = dict(rows=R, context=ctx, pages_per_row=max_pages)
            for name, depth in ARMS:
                nbytes = R * ctx * 2 * D * (4 if depth is None else 2)
                med = statistics.median(us[name])
                row[name] = dict(us_per_launch_median=round(med, 2), spread_us=round(max(us[name]) - min(us[name]), 2),
                                 all_us=[round(v, 2) for v in us[name]], kv_MB=round(nbytes / 1e6, 1), floor_us=round(2.6 + nbytes / 7.3e6, 2),
                                 TBps=round(nbytes / med / 1e6, 2))
            cases.append(row)
            print(json.dumps(row), flush=True)
            del graphs, pool16, pool32
            torch.cuda.empty_cache()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/attn_rows_bench.py", rounds=opt.rounds, replays=opt.replays, chain=N_LAYER, cases=cases), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
