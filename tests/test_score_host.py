"""CPU: the host side of `SSR_Speech.score` — batch validation, the packed prefill rows and the chunk plan, the reduction of per-position
cross entropy / rank into the reference's dict (fed the fixture's own reference CE and rank), the C entries' argument checks, and a
re-pin of the fixtures against the reference when its checkout is present."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd import _lib, score as SC
from ssr_speech_amd import weights as W
from oracle import ref_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "score_*.npz")))


def fixture_args(g):
    d, h, layers, vocab = (int(v) for v in g["cfg"])
    args = W.lm_args_tiny(d_model=d, nhead=h, layers=layers, vocab=vocab)
    args.predict_mask_token = int(g["flag_predict_mask_token"])
    args.predict_all = int(g["flag_predict_all"])
    cw = str(g["flag_codebook_weight"])
    args.codebook_weight = cw if cw else None
    return args


def fixture_batch(g):
    return {k: torch.from_numpy(g[k]) for k in ("x", "x_lens", "y", "y_lens")}


def scored_from_fixture(g, items, K):
    """The fixture's per-position reference CE / rank / target at the scored rows, in the order `score` concatenates them."""
    ce, rank, y = g["ce"], g["rank"], g["y"]
    nll, rk, tg = [], [], []
    for it in items:
        n = it.n_scored
        nll.append(ce[:, it.index, :n])
        rk.append(rank[:, it.index, :n])
        tg.append(y[it.index, :, 1:n + 1])
    return (torch.from_numpy(np.concatenate(nll, 1)), torch.from_numpy(np.concatenate(rk, 1)),
            torch.from_numpy(np.concatenate(tg, 1).astype(np.int32)))


def test_fixtures_exist():
    names = {os.path.basename(p) for p in FIXTURES}
    assert {"score_ragged_b3.npz", "score_all_cw_hd128.npz", "score_pad_x.npz", "score_empty_tmp_cb3.npz"} <= names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_reducer_on_reference_ce_and_rank_reproduces_the_reference_dict(path):
    g = np.load(path)
    args = fixture_args(g)
    items = SC.validate(fixture_batch(g), args)
    work = [it for it in items if it.n_scored > 0]
    nll, rank, tgt = scored_from_fixture(g, work, args.n_codebooks)
    idx = SC.scored_index(work)
    out = SC.reduce(nll, rank, tgt, torch.from_numpy(idx["item"]), torch.from_numpy(idx["pos"]), len(items), args)
    assert set(out) == {"loss", "top10acc", "top10acc_by_codebook", "effective_ntoken", "nll_by_item", "ntoken_by_item"}
    assert out["loss"].dtype == torch.float32 and out["top10acc"].dtype == torch.float32
    assert out["effective_ntoken"].dtype == torch.int64 and int(out["effective_ntoken"]) == int(g["effective_ntoken"])
    ref_loss = float(g["loss"])
    if np.isnan(ref_loss):
        assert torch.isnan(out["loss"])
    else:
        assert abs(float(out["loss"]) - ref_loss) <= 1e-6 * abs(ref_loss), (float(out["loss"]), ref_loss)
    ref_cb = g["top10acc_by_codebook"]
    for k, v in enumerate(out["top10acc_by_codebook"]):
        if ref_cb[k] == 0:
            assert float(v) == 0.0
        else:
            assert abs(float(v) - float(ref_cb[k])) <= 1e-6 * abs(float(ref_cb[k])), (k, float(v), ref_cb[k])
    assert abs(float(out["top10acc"]) - float(g["top10acc"])) <= 1e-6 * max(abs(float(g["top10acc"])), 1e-30)
    # per-item sums restate the same positions: their total is the unweighted CE sum over every codebook's tmp_mask
    assert int(out["ntoken_by_item"].sum()) > 0
    assert out["nll_by_item"].shape == (len(items),) and out["ntoken_by_item"].dtype == torch.int64


def test_empty_tmp_mask_gives_nan_loss_and_zero_accuracy():
    g = np.load(os.path.join(GOLD, "score_empty_tmp_cb3.npz"))
    assert np.isnan(g["loss"]) and g["top10acc_by_codebook"][-1] == 0


def test_pack_items_rows_match_the_prefill_format():
    args = W.lm_args_tiny()
    K = args.n_codebooks
    items = [SC.Item(0, np.array([3, 4, 5]), np.arange(8).reshape(K, 2)), SC.Item(2, np.array([7]), np.arange(12).reshape(K, 3) + 1)]
    pk = SC.pack_items(items, K)
    R = 3 + 2 + 1 + 3
    assert pk["tok"].shape == (R, 4) and pk["tok"].dtype == np.int32
    assert pk["tok"][:3, 0].tolist() == [3, 4, 5] and (pk["tok"][:3, 1:] == 0).all()
    assert pk["tok"][3:5, :K].tolist() == np.arange(8).reshape(K, 2).T.tolist()
    assert pk["pos"].tolist() == [0, 1, 2, 0, 1, 0, 0, 1, 2]
    assert pk["kind"].tolist() == [0, 0, 0, 1, 1, 0, 1, 1, 1]
    assert pk["row_seq"].tolist() == [0] * 5 + [1] * 4
    assert pk["row_pos"].tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3] and (pk["row_len"] == pk["row_pos"] + 1).all()
    assert pk["seq_start"].tolist() == [0, 5, 9]
    assert pk["score_first"].tolist() == [3, 6] and pk["score_count"].tolist() == [1, 2]
    assert pk["target"].shape == (K, 3)
    assert pk["target"][:, 0].tolist() == np.arange(8).reshape(K, 2)[:, 1].tolist()
    assert pk["target"][:, 1:].tolist() == (np.arange(12).reshape(K, 3) + 1)[:, 1:].tolist()
    assert int(pk["n_pages"]) == 2 and pk["table"].tolist() == [[0], [1]] and int(pk["max_len"]) == 5


def test_pack_items_pages_of_long_items():
    K = 4
    items = [SC.Item(0, np.zeros(100, int), np.zeros((K, 200), int)), SC.Item(1, np.zeros(5, int), np.zeros((K, 10), int))]
    pk = SC.pack_items(items, K)
    assert int(pk["n_pages"]) == 3 + 1 and pk["table"].shape == (2, 3)
    assert pk["table"][0].tolist() == [0, 1, 2] and pk["table"][1, 0] == 3 and (pk["table"] < 4).all()


def test_chunk_plans():
    assert SC.plan_chunks([5, 5, 5], 10) == [[0, 1], [2]]
    assert SC.plan_chunks([5, 5, 5], 15) == [[0, 1, 2]]
    assert SC.plan_chunks([30, 4, 4, 40, 3], 10) == [[0], [1, 2], [3], [4]]      # longer than max_rows: a chunk of its own
    assert SC.plan_chunks([], 10) == []
    with pytest.raises(ValueError):
        SC.plan_chunks([1], 0)


def test_validate_ragged_pad_x_and_errors():
    args = W.lm_args_tiny()
    g = np.load(os.path.join(GOLD, "score_pad_x.npz"))
    b = fixture_batch(g)
    items = SC.validate(b, args)
    assert [it.text.shape[0] for it in items] == g["x_lens"].tolist() and g["x"].shape[1] == 20 > g["x_lens"].max()
    assert [it.audio.shape[1] for it in items] == g["y_lens"].tolist()
    assert SC.validate(dict(x=torch.zeros(0, 3, dtype=torch.long), x_lens=torch.zeros(0), y=torch.zeros(0, 4, 2), y_lens=torch.zeros(0)), args) is None
    bad = dict(b, x=b["x"].clone())
    bad["x"][0, 0] = args.text_vocab_size + 1
    with pytest.raises(ValueError, match="text ids"):
        SC.validate(bad, args)
    bad = dict(b, y=b["y"].clone())
    bad["y"][1, 2, 0] = 10 ** 6
    with pytest.raises(ValueError, match="audio ids"):
        SC.validate(bad, args)
    bad = dict(b, y=b["y"].clone())
    bad["y"][1, 0, int(g["y_lens"][1])] = 0                          # a real-looking token in the padding
    with pytest.raises(ValueError, match="audio_pad_token"):
        SC.validate(bad, args)
    with pytest.raises(ValueError, match="x_lens"):
        SC.validate(dict(b, x_lens=b["x_lens"] + 100), args)
    with pytest.raises(ValueError, match="y_lens"):
        SC.validate(dict(b, y_lens=-b["y_lens"]), args)
    with pytest.raises(ValueError):
        SC.validate(dict(b, y=b["y"][:, :3]), args)                 # 3 codebooks
    with pytest.raises(ValueError):
        SC.validate({"x": b["x"]}, args)


def test_score_entries_refuse_null_arguments_without_a_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.ssrhip_sizeof(14) == __import__("ctypes").sizeof(_lib.ScoreArgs)
    assert L.ssrhip_lm_score(None, None, None, None) != 0
    assert b"null" in L.ssrhip_last_error()
    assert L.ssrhip_xent_rank(None, 8, 8, None, 4, None, None, None) != 0
    assert b"null" in L.ssrhip_last_error()
    # a complete-looking argument block with no scored-row arrays is refused before any launch
    d, w, a = _lib.LMDims(), _lib.LMWeights(), _lib.ScoreArgs()
    assert L.ssrhip_lm_score(d, w, a, None) != 0 and b"null" in L.ssrhip_last_error()


def test_forward_still_raises_and_points_to_score():
    from ssr_speech_amd.models.ssr import SSR_Speech
    m = SSR_Speech(W.lm_args_tiny())
    with pytest.raises(NotImplementedError, match="score"):
        m.forward({})
    g = np.load(os.path.join(GOLD, "score_ragged_b3.npz"))
    with pytest.raises(RuntimeError, match="GPU"):
        m.score(fixture_batch(g))                                     # CPU-resident model


@pytest.mark.skipif(not ref_import.available(), reason="the reference checkout is not present")
def test_regenerated_fixtures_are_bit_identical(tmp_path):
    from oracle import numerics
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_score.py"), "--out", str(tmp_path)], cwd=ROOT,
                       env=dict(os.environ, **numerics.ENV), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for path in FIXTURES:
        a, b = np.load(path), np.load(os.path.join(tmp_path, os.path.basename(path)))
        assert sorted(a.files) == sorted(b.files), path
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (path, k)
