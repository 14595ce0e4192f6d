"""CPU-side checks of sparse (BM25) recall (csrc/bm25.hip, evaluate.build_bm25_index / sparse_topk_news /
merge_recall / recommend): the restatement in bm25_util against the index the reference's own code built
(tests/golden/bm25_index.npz: ids, score bits, idf bits), merge_recall on hand cases, the header's limits
against the binding, the host-side workspace queries and the wrappers' argument checks."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import bm25_util as BU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newsrec_hip.h")


@pytest.fixture(scope="module")
def golden():
    g = BU.load_golden()
    return g, BU.build(g["tok"], g["V"], g["P"], g["k"])


def test_restatement_reproduces_the_reference_index(golden):
    g, ix = golden
    R = g["tok"].shape[0]
    assert (g["V"], g["P"], g["k"]) == (30522, 100, 2) and g["tok"].shape == (401, 12)
    has = np.flatnonzero((ix.post_ids != R).any(1))
    np.testing.assert_array_equal(has, g["tokens"])
    np.testing.assert_array_equal(ix.post_ids[g["tokens"]], g["post_ids"])
    np.testing.assert_array_equal(BU.bits64(ix.post_scores[g["tokens"]]), BU.bits64(g["post_scores"]))
    np.testing.assert_array_equal(BU.bits64(ix.idf[g["tokens"]]), BU.bits64(g["idf"]))
    assert not ix.bad
    # the fixture holds what it is there for: a pruned list, negative and signed-zero scores
    sc = g["post_scores"]
    assert (ix.n_post > 3 * g["P"]).any() and (ix.n_post == g["P"]).any() and (ix.n_post == g["P"] + 1).any()
    assert (sc < 0).any() and ((sc == 0) & np.signbit(sc)).sum() == 4 and (ix.df > R).any()
    dense = BU.dense_from_golden(g)
    assert dense.shape == (30522, 100, 2) and (dense[0, :, 0] == R).all() and (dense[101] == dense[0]).all()


def test_view_of_the_golden_index(golden):
    g, ix = golden
    tok, R = g["tok"], g["tok"].shape[0]
    kept = 0
    for n in range(R):
        for col in range(tok.shape[1]):
            t = int(tok[n, col])
            bit = bool((int(ix.keep[n]) >> col) & 1)
            want = (t not in BU.SPECIAL and t not in tok[n, :col] and n in ix.post_ids[t])
            assert bit == want, (n, col)
            if bit:
                p = int(np.flatnonzero(ix.post_ids[t] == n)[0])
                assert BU.bits32(ix.fwd[n, col]) == BU.bits32(np.float32(ix.post_scores[t, p]))
            else:
                assert ix.fwd[n, col] == 0 and not np.signbit(ix.fwd[n, col])
            kept += bit
    assert kept == int((ix.post_ids != R).sum())
    # a query of one token returns that token's list: scores rounded to fp32, equal ones by id
    t = int(g["tokens"][np.argmax(ix.n_post[g["tokens"]] == g["P"] + 1)])
    ids, sc = BU.expected_topk(tok, ix.fwd, ix.keep, [[t, 0, 101, -5, 40000, t]], g["V"], 128, first_row=0)
    assert (ids[0, :100] >= 0).all() and (ids[0, 100:] == -1).all() and np.isneginf(sc[0, 100:]).all()
    assert sorted(ids[0, :100].tolist()) == sorted(ix.post_ids[t].tolist())
    assert (np.diff(sc[0, :100]) <= 0).all()


def test_merge_recall_hand_cases():
    from newsrec_amd.evaluate import merge_recall
    a = torch.tensor([[5, 7, 9], [1, -1, -1], [-1, -1, -1], [4, 4, 2]])
    b = torch.tensor([[7, 5, 3], [1, 2, 3], [-1, -1, -1], [2, 8, 4]])
    want = [[5, 7, 9, 3, -1, -1], [1, 2, 3, -1, -1, -1], [-1] * 6, [4, 2, 8, -1, -1, -1]]
    got = merge_recall(a, b)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert BU.merge_recall(a.numpy(), b.numpy()).tolist() == want
    # unequal widths: the longer list goes on alone
    a2, b2 = torch.tensor([[6]]), torch.tensor([[1, 6, 2, -1, 3]])
    assert merge_recall(a2, b2).tolist() == [[6, 1, 2, 3, -1, -1]] == BU.merge_recall(a2.numpy(), b2.numpy()).tolist()
    assert merge_recall(b2, a2).tolist() == [[1, 6, 2, 3, -1, -1]]
    rng = np.random.default_rng(4)
    x, y = rng.integers(-1, 12, (40, 10)), rng.integers(-1, 12, (40, 7))
    assert merge_recall(torch.from_numpy(x), torch.from_numpy(y)).tolist() == BU.merge_recall(x, y).tolist()
    assert merge_recall(torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64)).shape == (0, 5)
    with pytest.raises(ValueError):
        merge_recall(a, b[:2])


def test_header_limits_match_the_binding():
    from newsrec_amd import _lib
    txt = open(HEADER).read()
    for name, val in (("NR_BM25_MAX_L", _lib.BM25_MAX_L), ("NR_BM25_MAX_POSTINGS", _lib.BM25_MAX_POSTINGS)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, txt, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.BM25_MAX_L == 64 and _lib.BM25_MAX_POSTINGS >= 128
    m = re.search(r"enum nr_bm25_flags \{ NR_BM25_BAD_TOKEN = (\d+) \}", txt)
    assert m and int(m.group(1)) == _lib.BM25_BAD_TOKEN
    for name in ("nr_bm25_build_workspace", "nr_bm25_topk_workspace"):
        assert _lib._RESTYPES[name] is _lib.c_i64
    for name in ("nr_bm25_count", "nr_bm25_build", "nr_bm25_forward", "nr_bm25_topk"):
        assert name in _lib.declared_symbols()


def test_workspace_queries():
    from newsrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.nr_bm25_build_workspace
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert f(-1, 30, 100) == 0 and f(10, 0, 100) == 0 and f(10, 65, 100) == 0 and f(10, 30, 0) == 0
    assert f(2 ** 31, 30, 100) == 0
    # offsets [V + 1] and one 8-byte key per (row, column), then the cursors [V] rounded to 8 bytes
    assert f(401, 12, 30522) == 30523 * 8 + 401 * 12 * 8 + 30522 * 4
    assert f(0, 1, 1) == 2 * 8 + 8 and f(7, 64, 3) == 4 * 8 + 7 * 64 * 8 + 16
    q = lib.nr_bm25_topk_workspace
    q.restype, q.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert q(-1, 1000, 10, 2) == 0 and q(65, -1, 10, 2) == 0 and q(65, 2 ** 31, 10, 2) == 0
    assert q(65, 1000, 0, 2) == 0 and q(65, 1000, 129, 2) == 0 and q(65, 1000, 10, -1) == 0 and q(65, 1000, 10, 65) == 0
    assert [q(65, 1000, 100, s) for s in (1, 2, 7, 64)] == [65 * s * 100 * 8 for s in (1, 2, 7, 64)]
    auto = q(1024, 72024, 100, 0)
    assert auto % (1024 * 100 * 8) == 0 and 1 <= auto // (1024 * 100 * 8) <= 64
    assert q(65, 60, 10, 0) == 65 * 1 * 10 * 8           # never more slices than 64-row tiles
    assert q(0, 1000, 10, 2) == 0


def test_wrappers_reject_bad_arguments_before_any_launch():
    from newsrec_amd import _lib as L
    from newsrec_amd import evaluate as EV
    tok = torch.zeros(5, 4, dtype=torch.int32)
    with pytest.raises(L.HipError):                      # CPU tensors: the kernels run on the GPU only
        EV.build_bm25_index(tok)
    ix = EV.BM25Index(tok, torch.zeros(9, 3, dtype=torch.int32), torch.zeros(9, 3, dtype=torch.float64),
                      torch.zeros(9, dtype=torch.int64), torch.zeros(9, dtype=torch.float64),
                      torch.zeros(5, 4), torch.zeros(5, dtype=torch.int64), 2, (0, 101, 102))
    assert (ix.n_rows, ix.vocab, ix.postings) == (5, 9, 3)
    with pytest.raises(L.HipError):
        EV.sparse_topk_news(ix, torch.zeros(2, 3, dtype=torch.int32), 5)
    ref = ix.to_reference()
    assert ref.shape == (9, 3, 2) and ref.dtype == torch.float64


def test_index_save_load_roundtrip(tmp_path):
    from newsrec_amd import evaluate as EV
    rng = np.random.default_rng(2)
    ix = EV.BM25Index(torch.from_numpy(rng.integers(0, 9, (5, 4)).astype(np.int32)),
                      torch.from_numpy(rng.integers(0, 6, (9, 3)).astype(np.int32)),
                      torch.from_numpy(rng.standard_normal((9, 3))), torch.arange(9), torch.from_numpy(rng.random(9)),
                      torch.from_numpy(rng.random((5, 4)).astype(np.float32)), torch.arange(5) - 2 ** 62, 3,
                      (1, 2, 3), True)
    path = ix.save(str(tmp_path / "index"))
    assert path.endswith("index.npz")
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(EV.BM25Index._ARRAYS + ("meta",))
    back = EV.BM25Index.load(path, device="cpu")
    for n in EV.BM25Index._ARRAYS:
        assert torch.equal(getattr(back, n), getattr(ix, n)) and getattr(back, n).dtype == getattr(ix, n).dtype, n
    assert (back.k, back.special, back.bad_tokens) == (3, (1, 2, 3), True)


def test_recommend_rejects_an_unknown_recall_type():
    from newsrec_amd.evaluate import recommend
    st = types.SimpleNamespace(mode="dev")
    for bad in ("x", "ds", "", "dense"):
        with pytest.raises(ValueError, match="recall_type"):
            recommend(None, st, recall_type=bad)
    with pytest.raises(ValueError):
        recommend(None, types.SimpleNamespace(mode="train"), recall_type="s")
