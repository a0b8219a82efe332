"""CPU: `engine.resolve_decode_plan` — the one place a DecodeEngine's weight stream, pair form, KV cache type and prompt sharing are
decided — against the answers recorded in tests/golden/decode_plan_cases.json (tools/gen_decode_plan_cases.py wrote it from the
constructor's own lines, before the resolvers became tables: the file is the behaviour to keep and is not regenerated to make this pass);
that the function reads nothing but its arguments; the key `SSR_Speech._get_engine` files engines under; and the counter names."""
import itertools
import json
import os

import pytest

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E
from ssr_speech_amd.models.ssr import engine_key

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_plan_cases.json")


def _outcome(doc, rows, dtype, layers, max_seq, env, pair_mode, req):
    try:
        p = E.resolve_decode_plan(rows, dtype, layers, max_seq, env, pair_mode=pair_mode, **req)
    except ValueError as err:
        return {"error": str(err)}
    return {"plan": [getattr(getattr(p, f), "name", getattr(p, f)) for f in doc["plan_fields"]]}


def test_every_recorded_case_resolves_to_the_recorded_plan_or_message():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["rows"] == [1, 2, 4, 5, 16, 17, 32] and tuple(doc["weight_dtypes"]) == E.WEIGHT_DTYPES
    assert tuple(doc["plan_fields"]) == E.DecodePlan._fields
    n = n_err = 0
    for r, e, pair_mode, max_seq, layers, ids in doc["groups"]:
        grid = list(itertools.product(doc["rows"], doc["weight_dtypes"]))
        assert len(ids) == len(grid)
        for (rows, dtype), want in zip(grid, ids):
            got = _outcome(doc, rows, dtype, layers, max_seq, doc["envs"][e], pair_mode, doc["requests"][r])
            assert got == doc["outcomes"][want], (rows, dtype, doc["requests"][r], doc["envs"][e], pair_mode, max_seq, layers)
            n += 1
            n_err += "error" in got
    shapes = {(g[2], (g[3] + 127) // 128, g[4]) for g in doc["groups"]}
    print(f"{n} cases ({n_err} refusals, {len(doc['outcomes'])} distinct outcomes) over {len(shapes)} (pair_mode, pages, layers)")
    assert shapes == set(itertools.product((0, 1, 2), (256, 257), (128, 129))) and n > 40000 and 0 < n_err < n


def test_the_plan_is_a_hashable_record_of_table_entries():
    p = E.resolve_decode_plan(2, "bf16", 4, 1024, {"SSRHIP_GEMV_W16_PAIR": "1"})
    assert p == E.DecodePlan(2, E.STREAMS[0], E.PAIR_FORMS[0], 0, "fp32", False, False, False, 8) and hash(p) == hash(p._replace())
    assert p.stream is E.W16_STREAMS[0] and E.W16Stream is E.Stream and E.W16_STREAMS == E.STREAMS[:3]
    with pytest.raises(AttributeError):
        p.pair_mode = 1
    assert [st.name for st in E.STREAMS] == ["w16", "wt16", "wt32", "w8", "wt8"] and [st.fmt for st in E.STREAMS] == ["bf16"] * 3 + ["e4m3"] * 2
    assert [pf.name for pf in E.PAIR_FORMS] == ["pair_w16", "pair_w8", "pair4", "pair4_pk"]
    bound = {sym[0] for sym in _lib.SYMBOLS}
    assert {"ssrhip_lm_set_" + st.name for st in E.STREAMS} | {"ssrhip_lm_set_" + pf.c_name for pf in E.PAIR_FORMS} <= bound
    assert {st.order for st in E.STREAMS} == set(E.PACKED_ORDERS) | set(E.CODE_ORDERS)
    with pytest.raises(TypeError, match="stream_w4"):
        E.resolve_decode_plan(2, "bf16", 4, 1024, {}, stream_w4=True)


SWITCHES = ("SSRHIP_GEMV_W16", "SSRHIP_GEMVM_W16", "SSRHIP_GEMV_W8", "SSRHIP_GEMVM_W8", "SSRHIP_GEMV_W16_PAIR", "SSRHIP_GEMV_W8_PAIR", "SSRHIP_GEMV_PAIR4",
            "SSRHIP_GEMV_PAIR4_PK", "SSRHIP_ATTN_KV16_SMALL")


def test_the_plan_reads_its_env_argument_and_not_the_process_environment(monkeypatch):
    assert {st.switch for st in E.STREAMS} | {pf.switch for pf in E.PAIR_FORMS} | {"SSRHIP_ATTN_KV16_SMALL"} == set(SWITCHES)
    shapes = [(rows, dtype) for rows in (2, 4, 8, 32) for dtype in E.WEIGHT_DTYPES]
    plans = lambda env: [E.resolve_decode_plan(rows, dtype, 4, 1024, env, kv_default="bf16") for rows, dtype in shapes]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    base = plans({})
    for name in SWITCHES:
        default = plans({name: "0"}) == base                 # one of the two values is what unset means ...
        assert plans({name: "0"}) != plans({name: "1"}) and (default or plans({name: "1"}) == base), name
        monkeypatch.setenv(name, "1" if default else "0")    # ... and the other one, in the process environment, changes nothing
        assert plans({}) == base, name
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------ the engine cache key
def _key(env, need_seq=900, **kw):
    cap_seq = ((need_seq + 1023) // 1024) * 1024             # as _get_engine rounds it
    return engine_key(kw.pop("weight_dtype", "bf16"), 4, kw.pop("kv_default", "fp32"), kw.pop("n_utt", 1), True, cap_seq, 256, env, **kw)


@pytest.mark.parametrize("switch,weight_dtype,n_utt", [("SSRHIP_GEMV_W16", "bf16", 1), ("SSRHIP_GEMVM_W16", "bf16", 8),
                                                        ("SSRHIP_GEMV_W8", "e4m3", 1), ("SSRHIP_GEMVM_W8", "e4m3", 8)])
def test_engine_key_differs_when_a_stream_switch_flips(switch, weight_dtype, n_utt):
    k0, k1 = (_key({switch: v}, weight_dtype=weight_dtype, n_utt=n_utt) for v in ("0", "1"))
    assert k0 != k1 and k0.plan.stream is None and k1.plan.stream is not None and k1.plan.stream.switch == switch
    assert not k0.covers(k1) and not k1.covers(k0)           # an engine built under the other value is not reused
    assert k0 == _key({switch: "0"}, weight_dtype=weight_dtype, n_utt=n_utt) and hash(k0) == hash(_key({switch: "0"}, weight_dtype=weight_dtype, n_utt=n_utt))


def test_engine_key_is_equal_within_a_capacity_and_covers_smaller_requests():
    assert _key({}, need_seq=100) == _key({}, need_seq=1024) != _key({}, need_seq=1025)
    built = _key({}, need_seq=2000)
    built = built._replace(pool=built.exact_pool)            # as _get_engine files it
    assert built.covers(_key({}, need_seq=100)) and built.covers(_key({}, need_seq=2048)) and not built.covers(_key({}, need_seq=2049))
    assert not built.covers(_key({}, need_seq=100, logprobs=True)) and not built.covers(_key({}, need_seq=100, n_utt=2))
    assert not built.covers(_key({}, need_seq=100)._replace(cap_steps=512))
    # the pool rule: enough pages, or exactly the request's pool under a caller-chosen page order
    assert built.pool == 32 and built.covers(_key({}, need_seq=100, need_pages=5)) and not built._replace(pool=4).covers(_key({}, need_seq=100, need_pages=5))
    pinned = _key({}, need_seq=2000, page_order=range(64))
    pinned = pinned._replace(pool=pinned.exact_pool)
    assert pinned.covers(_key({}, need_seq=2000, page_order=range(64))) and not pinned.covers(_key({}, need_seq=100, page_order=range(64)))
    # a bf16 cache has a page cap: an engine built above it holds fp32 entries and still serves the short request, as it was built
    big, small = (_key({}, need_seq=n, n_utt=8, kv_default="bf16") for n in (257 * 128, 100))
    assert (big.plan.kv_dtype, small.plan.kv_dtype) == ("fp32", "bf16") and big._replace(pool=big.exact_pool).covers(small)
    # prompt sharing is a request the key downgrades where the engine cannot serve it
    assert _key({}, n_utt=8, share_prompt=True).plan.share_prompt and not _key({}, n_utt=2, share_prompt=True).plan.share_prompt
    assert not _key({}, n_utt=8, share_prompt=True, kv_default="bf16").plan.share_prompt
    assert not _key({}, n_utt=8, share_prompt=True, need_seq=257 * 128).plan.share_prompt


# ------------------------------------------------------------------------------------------ the counters
def test_every_counter_is_a_property_of_the_engine_and_a_bound_symbol():
    names, bound = [name for name, _ in E.COUNTERS], {sym[0] for sym in _lib.SYMBOLS}
    assert names == ["kv16", "group", "w16", "w16_pair", "w8", "w8_pair", "pair4", "pair4_pk", "wt8", "wt16", "wt32"]
    for name, doc in E.COUNTERS:
        prop = getattr(E.DecodeEngine, name + "_launches_per_step")
        assert isinstance(prop, property) and prop.__doc__ == doc and doc, name
        assert f"ssrhip_lm_{name}_launches" in bound, name
    eng = E.DecodeEngine.__new__(E.DecodeEngine)
    eng._ctx = None
    assert [getattr(eng, n + "_launches_per_step") for n in names] == [0] * len(names)       # no context: nothing stepped
    assert {st.name for st in E.STREAMS} | {pf.c_name for pf in E.PAIR_FORMS} <= set(names)      # every table entry has its counter
