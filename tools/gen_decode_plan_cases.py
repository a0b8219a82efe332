"""Writes tests/golden/decode_plan_cases.json: what `engine.resolve_decode_plan` answers over a grid of engine shapes, requests and
environment switches — the plan, or the exact ValueError text. tests/test_decode_plan_host.py replays the file against the current code, so
the file is the record of the behaviour a rewrite of the resolvers must keep: run this at a commit whose answers are known to be right,
never to make a failing test pass. Needs no GPU.

  python tools/gen_decode_plan_cases.py [--out tests/golden/decode_plan_cases.json]

Layout of the file: `rows` x `weight_dtypes` is the inner grid; a group is [request index, env index, pair_mode, max_seq, layers,
outcome indices], one outcome per (rows, weight_dtype) in row-major order; `outcomes` holds each distinct answer once, either
{"plan": [the DecodePlan fields in `plan_fields` order, stream and pair by name]} or {"error": text}. `kv_default` among a request's
keys is the model's default cache type, every other key a request keyword of DecodeEngine.__init__.
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssr_speech_amd  # noqa: E402,F401
from ssr_speech_amd import engine as E  # noqa: E402

ROWS = (1, 2, 4, 5, 16, 17, 32)
PLAN_FIELDS = ("rows", "stream", "pair", "pair_mode", "kv_dtype", "kv16_small", "share_prompt", "logprobs", "max_pages")
BOOL_KEYWORDS = ("stream_w16", "stream_wt16", "stream_wt32", "stream_w8", "stream_wt8", "pair_w16", "pair_w8", "pair4", "pair4_pk", "kv16_small",
                 "share_prompt")
SWITCHES = ("SSRHIP_GEMV_W16", "SSRHIP_GEMVM_W16", "SSRHIP_GEMV_W8", "SSRHIP_GEMVM_W8", "SSRHIP_GEMV_W16_PAIR", "SSRHIP_GEMV_W8_PAIR",
            "SSRHIP_GEMV_PAIR4", "SSRHIP_GEMV_PAIR4_PK", "SSRHIP_ATTN_KV16_SMALL")
PAGE = 128


def requests():
    """None everywhere; each keyword alone at False and True (kv_dtype at both names, logprobs on, the model default at "bf16"); then the
    pairs of keywords the cross rules speak of"""
    out = [{}]
    out += [{k: v} for k in BOOL_KEYWORDS for v in (False, True)]
    out += [{"kv_dtype": "fp32"}, {"kv_dtype": "bf16"}, {"logprobs": True}, {"kv_default": "bf16"}]
    out += [dict(stream_w8=True, stream_w16=True), dict(stream_wt8=True, stream_wt16=True), dict(stream_wt8=True, stream_wt16=False),
            dict(stream_wt8=False, stream_wt16=True), dict(stream_wt8=True, stream_wt32=True),
            dict(kv16_small=True, kv_dtype="bf16"), dict(kv16_small=True, kv_default="bf16"), dict(kv16_small=True, kv_dtype="fp32", kv_default="bf16"),
            dict(kv16_small=False, kv_dtype="bf16"), dict(share_prompt=True, kv_dtype="bf16"), dict(share_prompt=True, kv_default="bf16"),
            dict(share_prompt=True, kv16_small=True, kv_dtype="bf16"),
            dict(pair_w16=True, stream_w16=False), dict(pair_w16=True, stream_w16=True), dict(pair_w8=True, stream_w8=False),
            dict(pair_w8=True, stream_w8=True), dict(pair4=True, stream_w16=False), dict(pair4=True, stream_w8=False),
            dict(pair4=True, stream_w16=True), dict(pair4=True, stream_w8=True), dict(pair4_pk=True, stream_w16=False),
            dict(pair4_pk=True, stream_w8=False), dict(pair4_pk=True, stream_w16=True), dict(pair4_pk=True, stream_w8=True),
            dict(pair4=True, pair4_pk=True), dict(pair_w16=True, pair_w8=True)]
    return out


def envs():
    """nothing set; each switch alone at "0" and "1"; all of them at "0" and at "1"; the two switches of the 5..16-row step together"""
    out = [{}]
    out += [{k: v} for k in SWITCHES for v in ("0", "1")]
    out += [{k: "0" for k in SWITCHES}, {k: "1" for k in SWITCHES}, {"SSRHIP_GEMVM_W8": "1", "SSRHIP_GEMVM_W16": "1"}]
    return out


def outcome(rows, dtype, layers, max_seq, env, pair_mode, req):
    try:
        p = E.resolve_decode_plan(rows, dtype, layers, max_seq, env, pair_mode=pair_mode, **req)
    except ValueError as err:
        return {"error": str(err)}
    name = lambda v: getattr(v, "name", v)
    return {"plan": [name(getattr(p, f)) for f in PLAN_FIELDS]}


def build():
    reqs, evs = requests(), envs()
    base = (0, 256 * PAGE, 128)
    # every request x every environment at the base shape; every request x (nothing set, everything on) at every other
    # (pair_mode, pages, layers)
    shapes = [s for s in itertools.product((0, 1, 2), (256 * PAGE, 256 * PAGE + 1), (128, 129))]
    combos = [(r, e, base) for r in range(len(reqs)) for e in range(len(evs))]
    everything_on = len(evs) - 2
    combos += [(r, e, s) for r in range(len(reqs)) for e in (0, everything_on) for s in shapes if s != base]
    outcomes, index, groups = [], {}, []
    for r, e, (pm, max_seq, layers) in combos:
        ids = []
        for rows, dtype in itertools.product(ROWS, E.WEIGHT_DTYPES):
            o = outcome(rows, dtype, layers, max_seq, evs[e], pm, reqs[r])
            key = json.dumps(o, sort_keys=True)
            if key not in index:
                index[key] = len(outcomes)
                outcomes.append(o)
            ids.append(index[key])
        groups.append([r, e, pm, max_seq, layers, ids])
    return dict(rows=list(ROWS), weight_dtypes=list(E.WEIGHT_DTYPES), plan_fields=list(PLAN_FIELDS), requests=reqs, envs=evs, outcomes=outcomes,
                groups=groups)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decode_plan_cases.json"))
    a = ap.parse_args()
    doc = build()
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: " + (json.dumps(v) if k != "groups" and k != "outcomes" else
                                                              "[\n  " + ",\n  ".join(json.dumps(x, separators=(",", ":")) for x in v) + "\n ]")
                                   for k, v in doc.items()) + "\n}\n")
    n = len(doc["groups"]) * len(doc["rows"]) * len(doc["weight_dtypes"])
    print(f"{a.out}: {n} cases in {len(doc['groups'])} groups, {len(doc['outcomes'])} distinct outcomes, {os.path.getsize(a.out)} bytes")
