"""Prompt sharing on the host (DESIGN.md Part I.15, no GPU): the page pool's reference counts, the pure planner that finds the rows with
equal prompts and cuts them into attention chunks, the pure rule that decides whether an engine shares, the CLI flag, and the contract
errors of the C side that are answered before any HIP call."""
import argparse
import ctypes as C

import numpy as np
import pytest

from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E

from helpers_share import fake_attn_args, fake_engine


# ------------------------------------------------------------------------------------------ the pool
def test_pool_reference_counts():
    pool = E.PagePool(4)
    a, b = pool.take("r0"), pool.take("r1")
    assert pool.n_free == 2 and pool.holders(a) == 1
    assert pool.share(a, "r2") == a and pool.share(a, "r4") == a
    assert pool.handed_out == [(a, "r0"), (b, "r1"), (a, "r2"), (a, "r4")]             # the record shows every holder
    assert pool.n_free == 2 and pool.holders(a) == 3                         # sharing takes nothing from the pool
    pool.give_back([a])                                                       # the first taker (the leader) lets go first
    assert pool.n_free == 2 and pool.holders(a) == 2
    pool.give_back([a, b])
    assert pool.n_free == 3 and pool.holders(a) == 1 and pool.holders(b) == 0
    pool.give_back([a])                                                       # the last holder: free at zero
    assert pool.n_free == 4 and pool.holders(a) == 0
    with pytest.raises(RuntimeError, match="returned twice"):
        pool.give_back([a])
    with pytest.raises(RuntimeError, match="nobody holds"):
        pool.share(a, "r3")
    assert pool.n_free == 4


def test_pool_share_then_followers_leave_first():
    pool = E.PagePool(3, order=[2, 0, 1])
    p = pool.take(0)
    assert p == 2
    for f in (2, 4):
        pool.share(p, f)
    pool.give_back([p])                                                       # follower 2
    pool.give_back([p])                                                       # follower 4
    assert pool.n_free == 2
    pool.give_back([p])                                                       # the leader, last
    assert pool.n_free == 3
    assert pool.take("next") == p                                             # and it is handed out again
    pool.reset()
    assert pool.n_free == 3 and pool.holders(p) == 0


# ------------------------------------------------------------------------------------------ the planner
def _seqs(texts, audios):
    return [(r, np.asarray(t), np.asarray(a)) for r, (t, a) in enumerate(zip(texts, audios))]


A0, A1 = [[1, 2, 3], [4, 5, 6]], [[1, 2, 3], [4, 5, 7]]


def test_planner_all_equal_rows():
    leader, chunks = E.plan_prompt_sharing(_seqs([[5, 6]] * 4, [A0] * 4), 8)
    assert leader == {0: 0, 1: 0, 2: 0, 3: 0} and chunks == [[0, 1, 2, 3]]


def test_planner_interleaved_equal_and_unequal_rows():
    """N samples under aug_text: rows 0, 2, 4, ... carry the text, rows 1, 3, 5, ... each its own random one"""
    texts = [[5, 6], [9, 1], [5, 6], [9, 2], [5, 6], [9, 3]]
    leader, chunks = E.plan_prompt_sharing(_seqs(texts, [A0] * 6), 8)
    assert leader == {0: 0, 1: 1, 2: 0, 3: 3, 4: 0, 5: 5}
    assert chunks == [[0, 2, 4], [1], [3], [5]]


def test_planner_two_distinct_groups():
    texts = [[5, 6], [7], [5, 6], [7], [5, 6], [7]]                           # equal unconditional rows: a second group
    leader, chunks = E.plan_prompt_sharing(_seqs(texts, [A0] * 6), 8)
    assert leader == {0: 0, 1: 1, 2: 0, 3: 1, 4: 0, 5: 1}
    assert chunks == [[0, 2, 4], [1, 3, 5]]


@pytest.mark.parametrize("members", [2, 4, 8])
def test_planner_members_plus_one_rows_are_two_chunks(members):
    n = members + 1
    leader, chunks = E.plan_prompt_sharing(_seqs([[3]] * n, [A0] * n), members)
    assert set(leader.values()) == {0}
    assert chunks == [list(range(members)), [members]]
    assert all(len(c) <= members for c in chunks)


def test_planner_equal_text_but_other_audio_is_not_shared():
    leader, chunks = E.plan_prompt_sharing(_seqs([[5, 6]] * 3, [A0, A1, A0]), 8)
    assert leader == {0: 0, 1: 1, 2: 0} and chunks == [[0, 2], [1]]
    # ... nor a text that is a prefix of another, nor audio of another shape with the same values
    leader, _ = E.plan_prompt_sharing(_seqs([[5, 6], [5, 6, 0]], [A0, A0]), 8)
    assert leader == {0: 0, 1: 1}
    leader, _ = E.plan_prompt_sharing([(0, np.arange(6), np.arange(6).reshape(2, 3)), (1, np.arange(6), np.arange(6).reshape(3, 2))], 8)
    assert leader == {0: 0, 1: 1}


def test_planner_takes_rows_in_any_order_and_any_subset():
    seqs = [(6, np.asarray([1]), np.asarray(A0)), (2, np.asarray([1]), np.asarray(A0)), (3, np.asarray([2]), np.asarray(A0))]
    leader, chunks = E.plan_prompt_sharing(seqs, 4)
    assert leader == {2: 2, 3: 3, 6: 2} and chunks == [[2, 6], [3]]
    with pytest.raises(ValueError):
        E.plan_prompt_sharing(seqs, 0)


# ------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("rows", [1, 2, 4, 5, 6, 16, 32])
def test_resolve_share_prompt(rows):
    for kv in E.KV_DTYPES:
        assert E.resolve_share_prompt(rows, None, kv) is False               # None = off, wherever
        assert E.resolve_share_prompt(rows, False, kv) is False
    if rows <= 4:
        with pytest.raises(ValueError, match="5..32 rows"):
            E.resolve_share_prompt(rows, True, "fp32")
    else:
        assert E.resolve_share_prompt(rows, True, "fp32") is True
        assert E.resolve_share_prompt(rows, True) is True
        with pytest.raises(ValueError, match="bf16"):
            E.resolve_share_prompt(rows, True, "bf16")


def test_cli_flag_parses():
    from ssr_speech_amd import inference_v2 as CLI
    flags = dict(CLI.EXTRA_FLAGS)
    assert flags["--share_prompt"]["choices"] == [0, 1] and flags["--share_prompt"]["default"] == 0
    names = [f for f, _ in CLI.EXTRA_FLAGS]
    assert names.index("--share_prompt") == names.index("--kv_dtype") + 1
    ap = argparse.ArgumentParser()
    ap.add_argument("--share_prompt", **flags["--share_prompt"])
    assert ap.parse_args([]).share_prompt == 0 and ap.parse_args(["--share_prompt", "1"]).share_prompt == 1
    with pytest.raises(SystemExit):
        ap.parse_args(["--share_prompt", "2"])


def test_public_signatures_default_to_off():
    import inspect
    from ssr_speech_amd import inference_scale as S
    from ssr_speech_amd.models.ssr import SSR_Speech
    assert inspect.signature(SSR_Speech.inference_batch).parameters["share_prompt"].default is False
    assert inspect.signature(S.inference_samples).parameters["share_prompt"].default is False
    assert inspect.signature(E.DecodeEngine.__init__).parameters["share_prompt"].default is None


# ------------------------------------------------------------------------------------------ the C side, before any HIP call
def test_abi_stays_107_and_the_new_symbols_exist():
    L = _lib.lib()
    assert L.ssrhip_version() == _lib.ABI_VERSION == 107
    for name in ("ssrhip_attn_rows_group", "ssrhip_attn_rows_group_m", "ssrhip_attn_group_members", "ssrhip_lm_set_prompt_groups",
                 "ssrhip_lm_group_launches", "ssrhip_lm_set_group_members", "ssrhip_lm_group_members"):
        assert hasattr(L, name), name
    assert L.ssrhip_attn_group_members() in (2, 4, 8)


def test_group_members_knob(monkeypatch):
    L = _lib.lib()
    default = L.ssrhip_attn_group_members()
    for v in ("2", "4", "8"):
        monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", v)
        assert L.ssrhip_attn_group_members() == int(v)
    monkeypatch.setenv("SSRHIP_ATTN_GROUP_MEMBERS", "3")
    assert L.ssrhip_attn_group_members() == default


def test_launch_contract_errors_are_answered_before_any_launch():
    """fake pointers, never dereferenced"""
    L = _lib.lib()
    ch, ns, out = 0x5000, 0x6000, 0x7000
    a = fake_attn_args(6)
    assert L.ssrhip_attn_rows_group(C.byref(a), None, ns, out, None) < 0 and b"null chunk_head" in L.ssrhip_last_error()
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, None, out, None) < 0 and b"null chunk_head" in L.ssrhip_last_error()
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, ns, None, None) < 0 and b"out is null" in L.ssrhip_last_error()
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, ns, a.q, None) < 0 and b"aliases q" in L.ssrhip_last_error()
    assert L.ssrhip_attn_rows_group(None, ch, ns, out, None) < 0
    a = fake_attn_args(6, max_pages=257)
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, ns, out, None) < 0 and b"256 pages" in L.ssrhip_last_error()
    a = fake_attn_args(33, out_tiled=1)
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, ns, out, None) < 0 and b"R <= 32" in L.ssrhip_last_error()
    a = fake_attn_args(6, hd=96)
    assert L.ssrhip_attn_rows_group(C.byref(a), ch, ns, out, None) < 0 and b"head_dim" in L.ssrhip_last_error()
    for msg in (L.ssrhip_last_error(),):
        assert b"ssrhip_attn_rows_group" in msg


def test_launch_with_an_explicit_chunk_size_takes_2_4_8_only():
    L = _lib.lib()
    a = fake_attn_args(6)
    for bad in (0, 1, 3, 16):
        assert L.ssrhip_attn_rows_group_m(C.byref(a), 0x5000, 0x6000, bad, 0x7000, None) < 0 and b"not in {2,4,8}" in L.ssrhip_last_error()
    assert L.ssrhip_attn_rows_group_m(C.byref(a), None, 0x6000, 4, 0x7000, None) < 0 and b"null chunk_head" in L.ssrhip_last_error()


def test_setter_refusals_on_engines_over_fake_records():
    """`ssrhip_lm_set_prompt_groups` answers from the engine's records alone: <= 4 rows, more than 256 pages per row, a kv16 engine, one
    array without the other — and `ssrhip_lm_set_kv16` refuses an engine that shares. (The refusal after capture needs a captured step:
    tests/test_gpu_share.py.) Nothing here is dereferenced or launched."""
    L = _lib.lib()
    ch, ns = 0x5000, 0x6000
    made = []
    mk = lambda B, mp=4: made.append(fake_engine(L, B, mp)) or made[-1]
    try:
        for B in (1, 4):
            assert L.ssrhip_lm_set_prompt_groups(mk(B), ch, ns) < 0 and b"5..32 rows" in L.ssrhip_last_error()
            assert L.ssrhip_lm_group_launches(made[-1]) == 0 and L.ssrhip_lm_group_members(made[-1]) == 0
        wide = mk(6, 257)
        assert L.ssrhip_lm_set_prompt_groups(wide, ch, ns) < 0 and b"256 pages" in L.ssrhip_last_error() and b"257" in L.ssrhip_last_error()
        assert L.ssrhip_lm_set_prompt_groups(wide, None, None) == 0                          # off is always accepted
        assert L.ssrhip_lm_set_prompt_groups(mk(6, 256), ch, ns) == 0                        # 256 pages per row: the page-id registers' capacity
        kv16 = mk(6)
        assert L.ssrhip_lm_set_kv16(kv16, 1) == 0
        assert L.ssrhip_lm_set_prompt_groups(kv16, ch, ns) < 0 and b"bf16 KV cache" in L.ssrhip_last_error()
        eng = mk(32)
        for one in ((ch, None), (None, ns)):
            assert L.ssrhip_lm_set_prompt_groups(eng, *one) < 0 and b"come together" in L.ssrhip_last_error()
        assert L.ssrhip_lm_set_group_members(eng, 4) < 0 and b"does not share" in L.ssrhip_last_error()
        assert L.ssrhip_lm_set_prompt_groups(eng, ch, ns) == 0
        assert L.ssrhip_lm_group_members(eng) == L.ssrhip_attn_group_members()               # the knob's value when the arrays were set
        assert L.ssrhip_lm_set_kv16(eng, 1) < 0 and b"shares prompts" in L.ssrhip_last_error()
        for m in (2, 4, 8):
            assert L.ssrhip_lm_set_group_members(eng, m) == 0 and L.ssrhip_lm_group_members(eng) == m
        assert L.ssrhip_lm_set_group_members(eng, 3) < 0 and b"not in {2,4,8}" in L.ssrhip_last_error()
        assert L.ssrhip_lm_group_members(eng) == 8 and L.ssrhip_lm_group_launches(eng) == 0  # nothing enqueued yet
        assert L.ssrhip_lm_set_prompt_groups(eng, None, None) == 0 and L.ssrhip_lm_group_members(eng) == 0
        assert L.ssrhip_lm_set_kv16(eng, 1) == 0                                             # ... and then the cache type is free again
        assert L.ssrhip_lm_set_group_members(None, 2) < 0
    finally:
        for e in made:
            L.ssrhip_lm_destroy(e)


def test_setter_refuses_a_null_engine():
    L = _lib.lib()
    assert L.ssrhip_lm_set_prompt_groups(None, 0x5000, 0x6000) < 0 and b"ssrhip_lm_set_prompt_groups" in L.ssrhip_last_error()
    assert L.ssrhip_lm_group_launches(None) == 0
