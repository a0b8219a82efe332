"""The opt-in bf16 KV cache of the 1/2/4-row decode step on the host (no GPU; DESIGN.md Part I.23): the pure rule, the setter's refusals and
the launcher's contract errors over fake records (nothing is dereferenced or launched), the ctypes list, a numpy model of the addresses
the landing cache is written and read at, and — as a condition on the INPUTS of tests/test_gpu_kv16_small.py — that rounding K / V moves
the oracle's logits by at least twice the bound those tests hold the engine to, so that an engine with an fp32 cache cannot pass them."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ssr_speech_amd import _lib
from ssr_speech_amd import engine as E

import helpers_kv16_small as HS
from helpers_share import fake_attn_args, fake_engine

ENV_ON, ENV_OFF = {"SSRHIP_ATTN_KV16_SMALL": "1"}, {"SSRHIP_ATTN_KV16_SMALL": "0"}
MSG_ROWS = r"kv16_small: the landing cache exists for the 1/2/4-row decode step only \(this engine has {rows} rows; engines of 5..32 rows take kv_dtype='bf16'\)"
MSG_FP32 = r"kv16_small needs the bf16 cache type \(kv_dtype='bf16' or SSR_Speech.set_kv_dtype\('bf16'\)\), not 'fp32'"


@pytest.mark.parametrize("rows", [1, 2, 4, 5, 32])
def test_rule_truth_table(rows):
    small = rows <= 4
    assert E.KV16_SMALL_DEFAULT == "0"
    for kv_requested, model_default in itertools.product((None, "fp32", "bf16"), ("fp32", "bf16")):
        wanted = model_default if kv_requested is None else kv_requested
        # requested None: rows, the wanted type and the switch — unset means KV16_SMALL_DEFAULT, a value that starts with '0' means off
        for env, on in (({}, False), (ENV_OFF, False), ({"SSRHIP_ATTN_KV16_SMALL": "01"}, False), (ENV_ON, True),
                        ({"SSRHIP_ATTN_KV16_SMALL": "yes"}, True), ({"SSRHIP_ATTN_KV16_SMALL": ""}, True)):
            assert E.resolve_kv16_small(rows, kv_requested, model_default, None, env) is (on and small and wanted == "bf16"), (kv_requested, model_default, env)
        # requested False: off, whatever else is said
        for env in ({}, ENV_ON):
            assert E.resolve_kv16_small(rows, kv_requested, model_default, False, env) is False
        # requested True: the row count is named first, then the cache type; the switch is not read
        for env in ({}, ENV_OFF, ENV_ON):
            if not small:
                with pytest.raises(ValueError, match=MSG_ROWS.format(rows=rows)):
                    E.resolve_kv16_small(rows, kv_requested, model_default, True, env)
            elif wanted != "bf16":
                with pytest.raises(ValueError, match=MSG_FP32):
                    E.resolve_kv16_small(rows, kv_requested, model_default, True, env)
            else:
                assert E.resolve_kv16_small(rows, kv_requested, model_default, True, env) is True


def test_rule_leaves_resolve_kv_dtype_alone():
    """the 5..32-row rule is what it was: bf16 at <= 4 rows is still its ValueError, and the model default still falls back to fp32 there"""
    for rows in (1, 2, 4):
        with pytest.raises(ValueError, match="5..32 rows"):
            E.resolve_kv_dtype(rows, "bf16", "fp32")
        assert E.resolve_kv_dtype(rows, None, "bf16") == "fp32"
    assert E.KV_DTYPES == ("fp32", "bf16") and E.KV16_SMALL_MAX_LAYERS == _lib.PAGE


def test_new_symbols_are_in_the_ctypes_list():
    names = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    assert names["ssrhip_attn_decode_kv16"] == (C.c_int, [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_void_p])
    assert names["ssrhip_lm_set_kv16_small"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    L = _lib.lib()
    assert hasattr(L, "ssrhip_attn_decode_kv16") and hasattr(L, "ssrhip_lm_set_kv16_small")
    assert L.ssrhip_version() == _lib.ABI_VERSION == 107                                      # additions only: the ABI did not move


def _deep_engine(L, B, n_layer):
    """`fake_engine` with a chosen layer count (its per-layer arrays are copied, never dereferenced)"""
    d = _lib.LMDims(128, 2, n_layer, 512, 4, 64, 64, 32, 4 * _lib.PAGE, 1)
    layer = (C.c_void_p * n_layer)(*([0x10000] * n_layer))
    w = _lib.LMWeights()
    for name in ("ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln2_w", "ln2_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b"):
        setattr(w, name, C.cast(layer, C.POINTER(C.c_void_p)))
    b = _lib.LMBuffers()
    b.B, b.n_utt, b.max_splits, b.pair_mode = B, max(B // 2, 1), 4, 1
    b.kv = _lib.KV(0x2000, 0x3000, 4, n_layer, 2, 64)
    ctx = C.c_void_p()
    _lib.check(L.ssrhip_lm_create(C.byref(d), C.byref(w), C.byref(b), C.byref(ctx)), "ssrhip_lm_create")
    return ctx


def test_setter_refusals_on_engines_over_fake_records(monkeypatch):
    """`ssrhip_lm_set_kv16_small` answers from the engine's records and the environment alone. (The refusal after capture needs a captured
    step: tests/test_gpu_kv16_small.py.)"""
    L = _lib.lib()
    monkeypatch.delenv("SSRHIP_PREFILL_ATTN_ROWWISE", raising=False)
    land, tab, pos = 0x5000, 0x6000, 0x7000
    made = []
    mk = lambda B: made.append(fake_engine(L, B)) or made[-1]
    try:
        assert L.ssrhip_lm_set_kv16_small(None, land, tab, pos) < 0 and b"ssrhip_lm_set_kv16_small: null engine" in L.ssrhip_last_error()
        for B in (5, 16, 32):
            assert L.ssrhip_lm_set_kv16_small(mk(B), land, tab, pos) < 0
            msg = L.ssrhip_last_error()
            assert b"<= 4-row decode step only" in msg and f"this engine has {B} rows".encode() in msg and b"ssrhip_lm_set_kv16)" in msg
            assert L.ssrhip_lm_set_kv16_small(made[-1], None, None, None) == 0                # off is always accepted
            assert L.ssrhip_lm_set_kv16(made[-1], 1) == 0                                     # ... and their own setter is what it was
        for B in (1, 2, 4):
            eng = mk(B)
            assert L.ssrhip_lm_set_kv16(eng, 1) < 0 and b"5..32 rows only" in L.ssrhip_last_error()
            for one in ((land, None, None), (None, tab, None), (None, None, pos), (land, tab, None), (land, None, pos), (None, tab, pos)):
                assert L.ssrhip_lm_set_kv16_small(eng, *one) < 0 and b"come together" in L.ssrhip_last_error()
            assert L.ssrhip_lm_set_kv16_small(eng, land, tab, pos) == 0
            assert L.ssrhip_lm_kv16_launches(eng) == 0                                        # nothing enqueued yet
            assert L.ssrhip_lm_set_kv16_small(eng, None, None, None) == 0
            monkeypatch.setenv("SSRHIP_PREFILL_ATTN_ROWWISE", "1")
            assert L.ssrhip_lm_set_kv16_small(eng, land, tab, pos) < 0 and b"SSRHIP_PREFILL_ATTN_ROWWISE" in L.ssrhip_last_error()
            assert L.ssrhip_lm_set_kv16_small(eng, None, None, None) == 0                     # switching off does not ask
            monkeypatch.delenv("SSRHIP_PREFILL_ATTN_ROWWISE")
        made.append(_deep_engine(L, 2, _lib.PAGE))
        assert L.ssrhip_lm_set_kv16_small(made[-1], land, tab, pos) == 0                      # layer 127 lands at position 127: the last one
        made.append(_deep_engine(L, 2, _lib.PAGE + 1))
        assert L.ssrhip_lm_set_kv16_small(made[-1], land, tab, pos) < 0
        assert b"129 layers" in L.ssrhip_last_error() and b"128" in L.ssrhip_last_error()
    finally:
        for e in made:
            L.ssrhip_lm_destroy(e)


def test_launch_contract_errors_are_answered_before_any_launch():
    """fake pointers, never dereferenced"""
    L = _lib.lib()
    land = 0x9000

    def args(R=2, **kw):
        a = fake_attn_args(R, **kw)
        a.part_o, a.part_ml = 0x7000, 0x8000
        return a

    assert L.ssrhip_attn_decode_kv16(None, land, None) < 0
    a = args()
    assert L.ssrhip_attn_decode_kv16(C.byref(a), None, None) < 0 and b"null landing cache" in L.ssrhip_last_error()
    a.row_seq = 0x4100
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"row_seq must be NULL" in L.ssrhip_last_error()
    a = args()
    a.part_ml = 0
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"null partial buffers" in L.ssrhip_last_error()
    a = args(hd=96)
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"head_dim" in L.ssrhip_last_error()
    a = args()
    a.kv.pool = 0
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"null argument" in L.ssrhip_last_error()
    a = args()
    a.max_splits = a.kv.max_pages + 1
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"max_splits" in L.ssrhip_last_error()
    a = args(R=65536)
    assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and b"65535 rows" in L.ssrhip_last_error()
    for layer, n_layer in ((-1, 2), (2, 2), (_lib.PAGE, 200)):                                # outside the cache's layers, or past the landing page
        a = args()
        a.kv.n_layer, a.layer = n_layer, layer
        assert L.ssrhip_attn_decode_kv16(C.byref(a), land, None) < 0 and f"layer {layer} outside".encode() in L.ssrhip_last_error()
    assert b"ssrhip_attn_decode_kv16" in L.ssrhip_last_error()


@pytest.mark.parametrize("n_layer,n_head,head_dim", [(2, 2, 64), (3, 2, 128), (24, 16, 128), (128, 2, 64)])
def test_every_writer_form_appends_where_the_reader_reads(n_layer, n_head, head_dim):
    """The QKV launch of layer l, given the landing descriptor, appends row b's K / V of head h at the element offset the attention launch
    of layer l reads for (row b, head h) — for each of the three ways the GEMV kernels compute an append address, for every
    (b < 4, layer, head, K / V) — inside the landing cache, and no two of them at the same place."""
    for B in (1, 2, 4):
        size = B * 2 * n_head * HS.PAGE * head_dim
        seen = set()
        for layer in range(n_layer):
            kv, g_layer, table, kv_pos = HS.landing_descriptor(B, n_layer, n_head, head_dim, layer)
            assert g_layer == 0 and kv["max_pages"] == 1 and kv["n_layer"] == 1 and (kv_pos < HS.PAGE).all() and (table < B).all()
            for b, which, h in itertools.product(range(B), (0, 1), range(n_head)):
                want = HS.reader_offset(n_head, head_dim, layer, b, which, h)
                for form in HS.WRITER_FORMS:
                    assert int(form(kv, g_layer, table, kv_pos, b, which, h)) == want, (form.__name__, B, layer, b, which, h)
                assert 0 <= want and want + head_dim <= size
                seen.add(want)
        assert len(seen) == n_layer * B * 2 * n_head                                          # distinct entries, head_dim floats apart at least
        assert min(np.diff(sorted(seen))) >= head_dim


def test_landing_bytes():
    """B * 2 * d_model * 128 * 4 bytes: 2 MiB per row at the 830M shape (d_model 2048)"""
    assert 1 * 2 * 2048 * _lib.PAGE * 4 == 2 << 20


@pytest.mark.parametrize("cfg", sorted(HS.CONFIGS))
def test_rounding_moves_the_oracle_by_twice_the_bound_on_the_chosen_inputs(monkeypatch, cfg):
    """For every utterance the engine-level GPU tests decode (under CFG at 2 and 4 rows, without at 1 row): the rounding oracle and the
    plain oracle differ by at least 2 x LOGIT_ATOL somewhere in the 24 steps — an fp32 cache would miss the bound — and pick the same
    greedy tokens."""
    assert HS.MIN_GAP == 2 * 2e-4
    cases = [(s, True) for s in HS.SEEDS[cfg]["cfg"]] + [(HS.SEEDS[cfg]["plain"], False)]
    assert HS.seeds_of(cfg, 4) == list(HS.SEEDS[cfg]["cfg"]) and HS.seeds_of(cfg, 2) == [HS.SEEDS[cfg]["cfg"][0]] and HS.seeds_of(cfg, 1) == [HS.SEEDS[cfg]["plain"]]
    for seed, use_cfg in cases:
        gap, same_tokens = HS.oracle_gap(monkeypatch, cfg, seed, use_cfg)
        print(f"{cfg} seed {seed} {'CFG' if use_cfg else 'no CFG'}: max |rounding oracle - plain oracle| = {gap:.2e}")
        assert gap >= HS.MIN_GAP, (cfg, seed, use_cfg, gap)
        assert same_tokens
        assert HS.oracle_trace(monkeypatch, cfg, seed, True, use_cfg)[0].shape[0] == HS.STEPS
