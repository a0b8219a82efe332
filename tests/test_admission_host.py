"""CPU: the host side of `DecodeEngine` admission that needs no device — the one packer of the prefill's rows
(`layout.pack_prefill_rows`, shared by the engine's admissions and `score.pack_items`) and the size / offset arithmetic of the one-copy
staging of an admission's integer arrays (`engine.IntStaging`)."""
import numpy as np
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd.engine import IntStaging
from ssr_speech_amd.layout import pack_prefill_rows


def test_packer_cfg_utterances_refilled_into_used_slots():
    """Two CFG utterances refilled into slots 3 and 5 of a CFG engine: four sequences with engine rows 6, 7, 10, 11 as ids; the two text
    rows of the first differ in length (the packer does not require them to match), the audio prompt is shared by an utterance's rows."""
    K = 4
    au_a = np.array([[10, 11], [20, 21], [30, 31], [40, 41]])          # [K, T = 2]
    au_b = np.array([[50], [60], [70], [80]])                          # [K, T = 1]
    pk = pack_prefill_rows([(6, [7, 8, 9], au_a), (7, [5], au_a), (10, [1, 2], au_b), (11, [3, 4], au_b)], K)
    assert pk["tok"].tolist() == [[7, 0, 0, 0], [8, 0, 0, 0], [9, 0, 0, 0], [10, 20, 30, 40], [11, 21, 31, 41],
                                  [5, 0, 0, 0], [10, 20, 30, 40], [11, 21, 31, 41],
                                  [1, 0, 0, 0], [2, 0, 0, 0], [50, 60, 70, 80],
                                  [3, 0, 0, 0], [4, 0, 0, 0], [50, 60, 70, 80]]
    assert pk["pos"].tolist() == [0, 1, 2, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    assert pk["kind"].tolist() == [0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 1]
    assert pk["row_seq"].tolist() == [6] * 5 + [7] * 3 + [10] * 3 + [11] * 3
    assert pk["row_pos"].tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 2, 0, 1, 2]
    assert pk["row_len"].tolist() == [1, 2, 3, 4, 5, 1, 2, 3, 1, 2, 3, 1, 2, 3]
    assert pk["seq_start"].tolist() == [0, 5, 8, 11, 14]
    assert pk["lens"].tolist() == [5, 3, 3, 3]
    assert set(pk) == {"tok", "pos", "kind", "row_seq", "row_pos", "row_len", "seq_start", "lens"}
    assert all(v.dtype == np.int32 for v in pk.values())


def test_packer_with_fewer_than_four_codebooks_leaves_the_other_columns_zero():
    pk = pack_prefill_rows([(2, np.array([9, 8]), np.array([[1, 2, 3], [4, 5, 6]]))], 2)
    assert pk["tok"].tolist() == [[9, 0, 0, 0], [8, 0, 0, 0], [1, 4, 0, 0], [2, 5, 0, 0], [3, 6, 0, 0]]
    assert pk["kind"].tolist() == [0, 0, 1, 1, 1] and pk["row_seq"].tolist() == [2] * 5 and pk["seq_start"].tolist() == [0, 5]


def test_staging_layout_of_an_admission():
    """tok | pos | kind | seq | rpos | rlen | seq_start | next_tok | t0 | kv0 | row index: R = 14 rows, n = 4 sequences = 4 engine rows."""
    R, n = 14, 4
    sizes = [4 * R, R, R, R, R, R, n + 1, 4 * n, n, n, n]
    offs, total = IntStaging.offsets(sizes)
    assert offs == [0, 56, 70, 84, 98, 112, 126, 131, 147, 151, 155] and total == 159
    # packing into a (here: unpinned) host buffer puts every part, flattened, at its offset; the device views are the same slices
    parts = [(np.arange(s, dtype=np.int64).reshape(-1, 4) if i in (0, 7) else np.arange(s, dtype=np.int32)) + 1000 * i
             for i, s in enumerate(sizes)]
    st = IntStaging()
    assert st.capacity == 0 and st.pinned is None and st.dev is None                 # nothing is allocated before the first grow
    st.pinned = torch.full((IntStaging.grown(total, 0),), -1, dtype=torch.int32)
    assert st.pack(parts) == (offs, total)
    host = st.pinned.numpy()
    for o, s, p in zip(offs, sizes, parts):
        assert host[o:o + s].tolist() == p.reshape(-1).tolist()
    assert (host[total:] == -1).all()


def test_staging_grow_rule():
    assert IntStaging.grown(159, 0) == 4096                   # never below 4096 words
    assert IntStaging.grown(5000, 4096) == 8192               # at least doubles
    assert IntStaging.grown(20000, 4096) == 20000             # or takes what the admission needs
    assert IntStaging.offsets([]) == ([], 0)
