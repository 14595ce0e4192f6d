"""CPU-side checks of the full-corpus top-K retrieval (csrc/topk.hip, evaluate.topk_news / recommend /
recall_metrics): the header's limits against their Python mirrors, the host-side workspace query, the
test oracle's own ordering on a hand-written case, and recall_metrics on CPU tensors."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import topk_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newsrec_hip.h")


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, open(HEADER).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_limits_match_the_binding():
    from newsrec_amd import _lib
    assert _define("NR_TOPK_MAX_K") == _lib.TOPK_MAX_K == 128
    assert _define("NR_TOPK_MAX_EXCLUDE") == _lib.TOPK_MAX_EXCLUDE == 256
    m = re.search(r"enum nr_topk_flags \{ NR_TOPK_NONFINITE = (\d+) \}", open(HEADER).read())
    assert m and int(m.group(1)) == _lib.TOPK_NONFINITE
    assert _lib._RESTYPES["nr_topk_workspace"] is _lib.c_i64


def test_workspace_query():
    from newsrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    f = ctypes.CDLL(_lib.LIB_PATH).nr_topk_workspace
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    # bad arguments
    assert f(-1, 1000, 10, 2) == 0 and f(65, -1, 10, 2) == 0
    assert f(65, 1000, 0, 2) == 0 and f(65, 1000, 129, 2) == 0
    assert f(65, 1000, 10, -1) == 0 and f(65, 1000, 10, 65) == 0
    assert f(65, 2 ** 31, 10, 2) == 0
    # one 8-byte entry per (user, slice, slot); grows with the slice count
    sizes = [f(65, 1000, 100, s) for s in (1, 2, 7, 64)]
    assert sizes == [65 * s * 100 * 8 for s in (1, 2, 7, 64)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # the automatic count is one of the admitted ones, and never more slices than 128-row tiles
    auto = f(1024, 72024, 100, 0)
    assert auto % (1024 * 100 * 8) == 0 and 1 <= auto // (1024 * 100 * 8) <= 64
    assert f(65, 100, 10, 0) == 65 * 1 * 10 * 8
    assert f(0, 1000, 10, 2) == 0                      # no users: nothing to hold


def test_oracle_ordering_on_a_hand_case():
    """2 users x 6 rows, H = 1 (scale 1): ties go to the smaller id, row 0 is skipped by first_row = 1."""
    table = np.array([[9.0], [1.0], [3.0], [3.0], [-2.0], [1.0]], np.float32)
    user = np.array([[1.0], [-1.0]], np.float32)
    ids, sc = TU.expected(table, user, 4)
    assert ids.tolist() == [[2, 3, 1, 5], [4, 1, 5, 2]]
    assert sc.tolist() == [[3.0, 3.0, 1.0, 1.0], [2.0, -1.0, -1.0, -3.0]]
    ids, sc = TU.expected(table, user, 4, first_row=0)
    assert ids.tolist() == [[0, 2, 3, 1], [4, 1, 5, 2]]
    # mask and exclude: user 0 loses row 2 and (padding ignored) nothing else; rows 4, 5 are masked out
    mask = np.array([1, 1, 1, 1, 0, 0], np.uint8)
    ex = np.array([[2, -1, 6], [1, 1, 3]], np.int64)
    ids, sc = TU.expected(table, user, 4, first_row=1, row_mask=mask, exclude=ex)
    assert ids.tolist() == [[3, 1, -1, -1], [2, -1, -1, -1]]
    assert sc[0].tolist() == [3.0, 1.0, -np.inf, -np.inf] and sc[1].tolist() == [-3.0] + [-np.inf] * 3
    TU.check_properties(table, user, ids, sc, 4, 1, mask, ex)
    # the scale is fp32 1 / sqrt(H)
    assert TU.scale32(4) == np.float32(0.5) and TU.scale32(150).dtype == np.float32


def test_property_check_rejects_wrong_answers():
    rng = np.random.default_rng(0)
    table = rng.standard_normal((40, 8)).astype(np.float32)
    user = rng.standard_normal((3, 8)).astype(np.float32)
    ids, sc = TU.expected(table, user, 5)
    TU.check_properties(table, user, ids, sc, 5)
    bad = ids.copy()
    bad[1, [0, 1]] = bad[1, [1, 0]]                     # scores no longer belong to their ids
    with pytest.raises(AssertionError):
        TU.check_properties(table, user, bad, sc, 5)
    ids9, sc9 = TU.expected(table, user, 9)
    with pytest.raises(AssertionError):                 # rows 1.. of the true order: the best row is left out
        TU.check_properties(table, user, ids9[:, 1:6], sc9[:, 1:6], 5)


def _store(cand_ids, labels, grp_off):
    return types.SimpleNamespace(cand_ids=torch.tensor(cand_ids, dtype=torch.int64),
                                 cand_labels=torch.tensor(labels, dtype=torch.int32),
                                 grp_off=torch.tensor(grp_off, dtype=torch.int64))


def test_recall_metrics_hand_case():
    from newsrec_amd.evaluate import recall_metrics
    # impression 0: no click (skipped); 1: clicks {7, 9, 4}, 9 listed twice; 2: clicks {5, 6}
    st = _store([3, 8, 7, 9, 9, 4, 2, 5, 6, 1], [0, 0, 1, 1, 1, 1, 0, 1, 1, 0], [0, 2, 7, 10])
    top = torch.tensor([[3, 8, 1, 2],
                        [1, 9, 2, 7],
                        [6, 5, 3, -1]], dtype=torch.int64)
    m = recall_metrics(top, st, ks=(1, 2, 4))
    assert m["n_impr_scored"] == 2
    # k=1: impression 1 finds nothing (0/3), impression 2 finds 6 (1/2)
    assert m["recall@1"] == round((0 + 0.5) / 2, 4) and m["hit@1"] == 0.5
    # k=2: {9} of 3, {6, 5} of 2
    assert m["recall@2"] == round((1 / 3 + 1.0) / 2, 4) and m["hit@2"] == 1.0
    # k=4: {9, 7} of 3 (partial hit), full hit
    assert m["recall@4"] == round((2 / 3 + 1.0) / 2, 4) and m["hit@4"] == 1.0
    assert sorted(m) == ["hit@1", "hit@2", "hit@4", "n_impr_scored", "recall@1", "recall@2", "recall@4"]
    with pytest.raises(ValueError):
        recall_metrics(top[:2], st)
    with pytest.raises(ValueError):
        recall_metrics(top, st, ks=(5,))
    # the default cutoffs need 10 columns
    wide = torch.cat([top, torch.full((3, 6), -1, dtype=torch.int64)], 1)
    d = recall_metrics(wide, st)
    assert d["recall@5"] == d["recall@10"] == m["recall@4"]


def test_recommend_rejects_a_train_store():
    from newsrec_amd.evaluate import recommend
    with pytest.raises(ValueError):
        recommend(None, types.SimpleNamespace(mode="train"))
