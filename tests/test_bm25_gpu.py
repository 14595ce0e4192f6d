"""Sparse (BM25) recall on the device (csrc/bm25.hip, evaluate.build_bm25_index / sparse_topk_news /
recommend) against the reference's own index (tests/golden/bm25_index.npz) and the restatement in
bm25_util.  Every comparison is exact -- ids, df, keep words and the bits of every score: the definition
fixes every rounding and every order.

  golden     the device index of the golden corpus equals the reference's, to_reference() included
  build      R / L / P / V on both sides of every block and cut, posting counts around P, lists that are
             one tie, out-of-range tokens, other specials and k, a strided corpus; fwd / keep each time
  query      U / Tq / K / R on both sides of every tile, empty queries, fewer than K rows, negative and
             zero sums, heavy ties, first_row / row_mask / exclude, every n_slices
  errors     every invalid-argument code of the four entries, nothing launched
  e2e        recommend("s" / "d" / "sd") and recall_metrics on the synthetic dev split
"""
import numpy as np
import pytest
import torch

import bm25_util as BU
from mind_util import load_data

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_index(ix, want, R):
    np.testing.assert_array_equal(ix.df.cpu().numpy(), want.df)
    np.testing.assert_array_equal(BU.bits64(ix.idf.cpu().numpy()), BU.bits64(want.idf))
    np.testing.assert_array_equal(ix.post_ids.cpu().numpy(), want.post_ids)
    np.testing.assert_array_equal(BU.bits64(ix.post_scores.cpu().numpy()), BU.bits64(want.post_scores))
    np.testing.assert_array_equal(ix.keep.cpu().numpy().view(np.uint64), want.keep)
    np.testing.assert_array_equal(BU.bits32(ix.fwd.cpu().numpy()), BU.bits32(want.fwd))
    assert ix.bad_tokens == want.bad and ix.n_rows == R
    assert ix.post_ids.dtype == torch.int32 and ix.post_scores.dtype == torch.float64 and ix.df.dtype == torch.int64


def _build_and_check(tok, V, P=100, k=2, special=BU.SPECIAL, device_tok=None):
    from newsrec_amd.evaluate import build_bm25_index
    t = device_tok if device_tok is not None else _dev(tok)
    ix = build_bm25_index(t, vocab=V, postings=P, k=k, special=special)
    want = BU.build(tok, V, P, k, special)
    _check_index(ix, want, tok.shape[0])
    return ix, want


def _corpus(rng, R, L, V, n_words=40, heavy=0.3):
    """[CLS] then Zipf-distributed words (one of them heavy: several per row, so df > R), [SEP], pad; some
    rows without [CLS]; ids spread over [0, V)."""
    words = np.unique(np.concatenate([rng.integers(3, V, n_words), [3]]))
    words = words[~np.isin(words, BU.SPECIAL)]
    w = 1.0 / np.arange(1, len(words) + 1)
    w /= w.sum()
    tok = np.zeros((R, L), np.int32)
    for n in range(R):
        length = int(rng.integers(1, L + 1))
        body = np.where(rng.random(length) < heavy, words[0], rng.choice(words, length, p=w))
        tok[n, :length] = body
        if rng.random() < 0.85:
            tok[n, 0] = 101
        if length >= 2 and rng.random() < 0.9:
            tok[n, length - 1] = 102
    return tok


# ------------------------------------------------------------------------------------------------ build
def test_golden_corpus_matches_the_reference():
    g = BU.load_golden()
    ix, _ = _build_and_check(g["tok"], g["V"], g["P"], g["k"])
    R = g["tok"].shape[0]
    ids, sc = ix.post_ids.cpu().numpy(), ix.post_scores.cpu().numpy()
    np.testing.assert_array_equal(np.flatnonzero((ids != R).any(1)), g["tokens"])
    np.testing.assert_array_equal(ids[g["tokens"]], g["post_ids"])
    np.testing.assert_array_equal(BU.bits64(sc[g["tokens"]]), BU.bits64(g["post_scores"]))
    np.testing.assert_array_equal(BU.bits64(ix.idf.cpu().numpy()[g["tokens"]]), BU.bits64(g["idf"]))
    assert ((sc == 0) & np.signbit(sc)).sum() == 4                   # the -0.0 scores survive
    ref = ix.to_reference()
    assert ref.dtype == torch.float64 and not ref.is_cuda
    np.testing.assert_array_equal(BU.bits64(ref.numpy()), BU.bits64(BU.dense_from_golden(g)))


BUILD_CASES = [(1, 1, 1, 200), (1, 12, 4, 200), (2, 2, 100, 200), (63, 30, 4, 200), (64, 64, 128, 200),
               (65, 12, 1, 200), (401, 30, 100, 200), (401, 12, 4, 30522), (65, 1, 4, 200), (64, 2, 1, 200),
               (401, 64, 128, 200), (63, 12, 100, 200), (129, 30, 4, 200)]


def test_build_cases_cover_every_size():
    for col, vals in enumerate(((1, 2, 63, 64, 65, 401), (1, 2, 12, 30, 64), (1, 4, 100, 128))):
        assert {c[col] for c in BUILD_CASES} >= set(vals)
    assert sum(c[3] == 30522 for c in BUILD_CASES) == 1


@pytest.mark.parametrize("R,L,P,V", BUILD_CASES)
def test_build_family(R, L, P, V):
    rng = np.random.default_rng(100000 * R + 1000 * L + P)
    tok = _corpus(rng, R, L, V)
    ix, want = _build_and_check(tok, V, P)
    if R >= 63 and L >= 12:
        assert (want.df > R).any() and (want.idf < 0).any()          # the heavy word: negative scores
        assert (want.n_post > P).any() or P >= 100                   # rows cut by the prune
        dup = [len(set(r[r != 0].tolist())) < (r != 0).sum() for r in tok]
        assert any(dup)                                              # repeated tokens: only the first column kept


@pytest.mark.parametrize("P", [4, 100])
def test_posting_counts_around_the_cut(P):
    """Tokens with 0, 1, P - 1, P, P + 1 and 5 P + 3 postings, term frequencies 1 .. 3."""
    rng = np.random.default_rng(P)
    counts = {10: 0, 11: 1, 12: P - 1, 13: P, 14: P + 1, 15: 5 * P + 3}
    R, L, V = 5 * P + 3 + 10, 12, 200
    tok = np.zeros((R, L), np.int32)
    tok[:, 0] = 101
    fill = np.ones(R, np.int64)
    for t, c in counts.items():
        for n in rng.permutation(R)[:c]:
            for _ in range(int(rng.integers(1, 4))):
                if fill[n] < L:
                    tok[n, fill[n]] = t
                    fill[n] += 1
    ix, want = _build_and_check(tok, V, P)
    assert [int(want.n_post[t]) for t in sorted(counts)] == [0, 1, P - 1, P, P + 1, 5 * P + 3]
    ids = ix.post_ids.cpu().numpy()
    assert (ids[10] == R).all() and (ids[13] != R).all() and (ids[12] != R).sum() == P - 1


def test_the_largest_cut():
    """P = NR_BM25_MAX_POSTINGS with a list longer than that: the select's LDS buffer is full."""
    from newsrec_amd import _lib as L
    P = L.BM25_MAX_POSTINGS
    tok = _corpus(np.random.default_rng(3), 2000, 6, 200)
    _, want = _build_and_check(tok, 200, P)
    assert (want.n_post > P).any() and ((want.n_post > 0) & (want.n_post < P)).any()


@pytest.mark.parametrize("per_row", [1, 2])
def test_a_list_that_is_one_tie_is_ordered_by_row(per_row):
    """Every row holds the token per_row times: equal scores (negative idf at two per row: df = 2 R > R),
    so the P best are rows 0 .. P - 1."""
    R, L, V, P = 300, 6, 200, 100
    rng = np.random.default_rng(per_row)
    tok = rng.integers(20, 40, (R, L)).astype(np.int32)
    tok[:, 0] = 101
    for n in range(R):
        tok[n, 1 + rng.permutation(L - 1)[:per_row]] = 9
    ix, want = _build_and_check(tok, V, P)
    assert (want.idf[9] < 0) == (per_row == 2)
    assert ix.post_ids[9].cpu().tolist() == list(range(P))
    assert len(set(BU.bits64(ix.post_scores[9].cpu().numpy()).tolist())) == 1


def test_out_of_range_tokens_special_ids_k_and_strides():
    rng = np.random.default_rng(77)
    R, L, V = 130, 12, 200
    tok = _corpus(rng, R, L, V)
    clean, _ = _build_and_check(tok, V, 4)
    assert not clean.bad_tokens
    bad = tok.copy()
    bad[5, 3], bad[64, 0], bad[129, 11], bad[70, 2] = -3, V, V + 5, 2 ** 31 - 1
    ix, want = _build_and_check(bad, V, 4)
    assert ix.bad_tokens and want.bad
    # other specials and k: 101 now posts like any word, the heavy word does not
    heavy = int(np.bincount(tok[tok > 2].ravel()).argmax())
    for k in (1, 3):
        ix, want = _build_and_check(tok, V, 4, k=k, special=(0, heavy, 7))
        assert (want.post_ids[101] != R).any() and (want.post_ids[heavy] == R).all()
    # a corpus that is a column window of a wider tensor
    wide = torch.full((R, L + 5), 3, dtype=torch.int32, device=DEV)
    wide[:, 2:2 + L] = _dev(tok)
    view = wide[:, 2:2 + L]
    assert view.stride(0) == L + 5
    _build_and_check(tok, V, 4, device_tok=view)


# ------------------------------------------------------------------------------------------------ query
def _host_index(tok, V, P, special=BU.SPECIAL, k=2):
    """The restatement's index on the device: the query tests do not depend on the build kernels."""
    from newsrec_amd.evaluate import BM25Index
    w = BU.build(tok, V, P, k, special)
    ix = BM25Index(_dev(tok), _dev(w.post_ids), _dev(w.post_scores), _dev(w.df), _dev(w.idf), _dev(w.fwd),
                   _dev(w.keep.view(np.int64)), k, special)
    return ix, w


def _unused_token(tok):
    return min(set(range(3, 200)) - set(tok.ravel().tolist()) - set(BU.SPECIAL))


@pytest.fixture(scope="module")
def corpora():
    """R -> (tok, device index, restatement) at L = 12, V = 200, P = 20; built once, never modified."""
    out = {}
    for R in (63, 64, 65, 401):
        tok = _corpus(np.random.default_rng(R), R, 12, 200)
        tok[[5, 40], 0] = _unused_token(tok)                         # seen in column 0 only: tf = 0, idf = 0
        out[R] = (tok,) + _host_index(tok, 200, 20)
    return out


def _queries(rng, tok, U, Tq, V):
    """Bags of corpus words with specials, out-of-range ids and repeats mixed in; user 0 holds junk only."""
    words = np.unique(tok[tok > 2])
    words = words[~np.isin(words, BU.SPECIAL)]
    q = rng.choice(words, (U, Tq)).astype(np.int32)
    junk = np.array([0, 101, 102, -1, V, V + 77, -2 ** 31, 2 ** 31 - 1], np.int32)
    where = rng.random((U, Tq)) < 0.3
    q[where] = rng.choice(junk, int(where.sum()))
    if Tq:
        q[0] = rng.choice(junk, Tq)
    return q


def _same(got, want):
    ids, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
    np.testing.assert_array_equal(ids, want[0])
    np.testing.assert_array_equal(BU.bits32(sc), BU.bits32(want[1]))
    return ids, sc


def _search(ix, q, K, **kw):
    from newsrec_amd.evaluate import sparse_topk_news
    t = {n: (_dev(v) if isinstance(v, np.ndarray) else v) for n, v in kw.items()}
    got = sparse_topk_news(ix, _dev(q), K, **t)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (len(q), K)
    return got


QUERY_CASES = [(1, 0, 1, 63), (15, 1, 10, 64), (16, 7, 100, 65), (17, 1500, 128, 401), (64, 7, 10, 401),
               (65, 1500, 100, 65), (65, 7, 128, 63), (16, 1, 1, 401), (17, 0, 10, 64), (7, 7, 10, 65), (8, 40, 100, 63),
               (9, 40, 128, 401)]


def test_query_cases_cover_every_size():
    for col, vals in enumerate(((1, 15, 16, 17, 64, 65), (0, 1, 7, 1500), (1, 10, 100, 128), (63, 64, 65, 401))):
        assert {c[col] for c in QUERY_CASES} >= set(vals)


@pytest.mark.parametrize("U,Tq,K,R", QUERY_CASES)
def test_query_family(corpora, U, Tq, K, R):
    tok, ix, w = corpora[R]
    q = _queries(np.random.default_rng(1000 * U + Tq + K), tok, U, Tq, 200)
    for first_row in (0, 1):
        want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, K, first_row)
        ids, sc = _same(_search(ix, q, K, first_row=first_row), want)
    assert (ids[0] == -1).all() and np.isneginf(sc[0]).all()         # the empty query
    if Tq == 1 and K >= 10:
        assert ((ids >= 0).sum(1) < K).any()                         # fewer than K eligible rows


def test_negative_and_zero_sums_are_eligible_and_ordered(corpora):
    tok, ix, w = corpora[401]
    heavy = [int(t) for t in np.flatnonzero(w.idf < 0) if t not in BU.SPECIAL][0]
    zero = int(tok[5, 0])
    assert w.df[zero] == 0 and w.idf[zero] == 0 and w.n_post[zero] == 2
    q = np.array([[heavy, heavy], [zero, zero], [heavy, zero]], np.int32)
    want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, 128, 0)
    ids, sc = _same(_search(ix, q, 128, first_row=0), want)
    assert (sc[0][ids[0] >= 0] <= 0).all() and (sc[0] < 0).any() and (ids[0] >= 0).sum() == 20
    assert (np.diff(sc[0][ids[0] >= 0]) <= 0).all()
    assert ids[1].tolist()[:3] == [5, 40, -1] and (sc[1][:2] == 0).all()
    assert set(ids[2][ids[2] >= 0].tolist()) == set(ids[0][ids[0] >= 0].tolist()) | {5, 40}


@pytest.mark.parametrize("K", [10, 128])
def test_heavy_ties_and_every_geometry(K):
    """The second half of the corpus repeats the first: every score occurs at least twice, on both sides
    of every 64-row tile and of every slice; all n_slices give the same bits."""
    rng = np.random.default_rng(9)
    half = _corpus(rng, 300, 12, 200, n_words=12)
    tok = np.concatenate([half, half])
    ix, w = _host_index(tok, 200, 1024)
    q = _queries(rng, tok, 33, 7, 200)
    want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, K)
    with np.errstate(invalid="ignore"):                              # (-inf tails)
        assert (np.diff(want[1][1:], axis=1) == 0).mean() > 0.4
    for ns in (0, 1, 2, 7, 64):
        _same(_search(ix, q, K, n_slices=ns), want)


@pytest.mark.parametrize("E", [0, 1, 50])
def test_first_row_mask_and_exclude(corpora, E):
    tok, ix, w = corpora[401]
    rng = np.random.default_rng(50 + E)
    U, K, R = 17, 10, 401
    q = _queries(rng, tok, U, 40, 200)
    top = BU.expected_topk(tok, w.fwd, w.keep, q, 200, 128, 1)[0]
    ex = None
    if E:
        ex = np.full((U, E), -1, np.int64)
        ex[:, 0] = top[:, 0]                                         # the row that would be first
        if E > 1:
            ex[:, 1], ex[:, 2] = R, top[:, 0]                        # padding, a repeat
            ex[:, 3:E // 2] = top[:, 1:E // 2 - 2]
            ex[::2, E // 2:] = rng.integers(0, R, (len(ex[::2]), E - E // 2))
    for first_row in (0, 1, 70):
        want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, K, first_row, None, ex)
        _same(_search(ix, q, K, first_row=first_row, exclude=ex), want)
    mask = (rng.random(R) < 0.05).astype(np.uint8)
    want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, K, 1, mask, ex)
    ids, _ = _same(_search(ix, q, K, row_mask=mask, exclude=ex), want)
    assert np.isin(ids[ids >= 0], np.flatnonzero(mask)).all()


def test_user_with_every_eligible_row_excluded(corpora):
    tok, ix, w = corpora[401]
    q = _queries(np.random.default_rng(6), tok, 5, 200, 200)
    matched = BU.sparse_scores(tok, w.fwd, w.keep, q, 200)[1]
    common = np.flatnonzero(matched[1:].all(0))                      # rows that every real user matches
    keep_rows = common[[1, len(common) // 3, len(common) // 2, -2, -1]]
    assert keep_rows[0] >= 1 and keep_rows[0] < 64 < keep_rows[-1] and len(set(keep_rows.tolist())) == 5
    mask = np.zeros(401, np.uint8)
    mask[keep_rows] = 1
    ex = np.full((5, 6), -1, np.int64)
    ex[2, :5] = keep_rows
    ex[3, :2] = keep_rows[[1, 4]]
    want = BU.expected_topk(tok, w.fwd, w.keep, q, 200, 10, 1, mask, ex)
    ids, sc = _same(_search(ix, q, 10, row_mask=mask, exclude=ex), want)
    assert (ids[2] == -1).all() and np.isneginf(sc[2]).all()
    assert sorted(ids[1][ids[1] >= 0].tolist()) == keep_rows.tolist()
    assert sorted(ids[3][ids[3] >= 0].tolist()) == keep_rows[[0, 2, 3]].tolist()


# ------------------------------------------------------------------------------------------------ errors
def test_entries_reject_bad_arguments():
    from newsrec_amd import _lib as L
    lib, P = L.load(), L.ptr
    R, Ls, V, Pn, U, Tq, K = 40, 6, 50, 4, 3, 5, 5
    tok = torch.ones(R, Ls, dtype=torch.int32, device=DEV)
    df = torch.full((V,), -7, dtype=torch.int64, device=DEV)
    npost = torch.full((V,), -7, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    S = L.stream_ptr(tok)

    def count(tok=tok, ldt=Ls, R=R, Ls=Ls, V=V, df=df, npost=npost, st=st):
        return lib.nr_bm25_count(P(tok), ldt, R, Ls, V, 0, 101, 102, P(df), P(npost), P(st), S)
    assert count(R=-1) == -1000 and count(Ls=0) == -1000 and count(Ls=65) == -1000 and count(V=0) == -1000
    assert count(R=2 ** 31) == -1000
    assert count(tok=None) == -1001 and count(df=None) == -1001 and count(npost=None) == -1001 and count(st=None) == -1001
    assert count(ldt=Ls - 1) == -1004
    torch.cuda.synchronize()
    assert (df == -7).all() and (npost == -7).all()                   # nothing ran

    idf = torch.zeros(V, dtype=torch.float64, device=DEV)
    ids = torch.full((V, Pn), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((V, Pn), -7.0, dtype=torch.float64, device=DEV)
    nb = int(lib.nr_bm25_build_workspace(R, Ls, V))
    ws = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=DEV)

    def build(tok=tok, ldt=Ls, R=R, Ls=Ls, V=V, Pn=Pn, k=2, idf=idf, npost=npost, ids=ids, sc=sc, ws=ws, nb=nb):
        return lib.nr_bm25_build(P(tok), ldt, R, Ls, V, Pn, k, 0, 101, 102, P(idf), P(npost), P(ids), P(sc), P(ws), nb, S)
    assert build(R=-1) == -1000 and build(Ls=65) == -1000 and build(V=0) == -1000 and build(k=0) == -1000
    assert build(nb=-1) == -1000
    assert build(idf=None) == -1001 and build(npost=None) == -1001 and build(ids=None) == -1001
    assert build(sc=None) == -1001 and build(tok=None) == -1001
    assert build(Pn=0) == -1002 and build(Pn=L.BM25_MAX_POSTINGS + 1) == -1002
    assert build(ldt=Ls - 1) == -1004
    assert build(ws=None) == -1006 and build(nb=nb - 1) == -1006
    assert lib.nr_bm25_build(P(tok), Ls, R, Ls, V, Pn, 2, 0, 101, 102, P(idf), P(npost), P(ids), P(sc),
                             L.c_ptr(ws.data_ptr() + 4), nb, S) == -1006
    torch.cuda.synchronize()
    assert (ids == -7).all() and (sc == -7).all()

    fwd = torch.full((R, Ls), -7.0, device=DEV)
    keep = torch.full((R,), -7, dtype=torch.int64, device=DEV)

    def forward(tok=tok, ldt=Ls, R=R, Ls=Ls, V=V, Pn=Pn, ids=ids, sc=sc, fwd=fwd, ldf=Ls, keep=keep):
        return lib.nr_bm25_forward(P(tok), ldt, R, Ls, V, Pn, P(ids), P(sc), P(fwd), ldf, P(keep), S)
    assert forward(R=-1) == -1000 and forward(Ls=0) == -1000 and forward(V=0) == -1000
    assert forward(tok=None) == -1001 and forward(ids=None) == -1001 and forward(sc=None) == -1001
    assert forward(fwd=None) == -1001 and forward(keep=None) == -1001
    assert forward(Pn=0) == -1002 and forward(Pn=L.BM25_MAX_POSTINGS + 1) == -1002
    assert forward(ldt=Ls - 1) == -1004 and forward(ldf=Ls - 1) == -1004
    torch.cuda.synchronize()
    assert (fwd == -7).all() and (keep == -7).all()

    q = torch.ones(U, Tq, dtype=torch.int32, device=DEV)
    fwd.zero_()
    keep.zero_()
    top = torch.full((U, K), -77, dtype=torch.int64, device=DEV)
    ts = torch.full((U, K), 123.0, device=DEV)
    ex = torch.zeros(U, L.TOPK_MAX_EXCLUDE + 1, dtype=torch.int64, device=DEV)
    ws2 = torch.zeros(U * 2 * K, dtype=torch.int64, device=DEV)

    def topk(q=q, ldq=Tq, U=U, Tq=Tq, tok=tok, ldt=Ls, fwd=fwd, ldf=Ls, keep=keep, R=R, Ls=Ls, V=V, K=K, first_row=1,
             mask=None, ex=None, E=0, ns=1, top=top, ts=ts, ws=None, nb=0):
        return lib.nr_bm25_topk(P(q), ldq, U, Tq, P(tok), ldt, P(fwd), ldf, P(keep), R, Ls, V, 0, 101, 102, K,
                                first_row, P(mask), P(ex), E, ns, P(top), P(ts), P(ws), nb, S)
    assert topk(U=-1) == -1000 and topk(Tq=-1) == -1000 and topk(R=-1) == -1000 and topk(Ls=0) == -1000
    assert topk(Ls=65) == -1000 and topk(V=0) == -1000 and topk(E=-1) == -1000 and topk(first_row=-1) == -1000
    assert topk(ns=-1) == -1000 and topk(nb=-1) == -1000
    assert topk(q=None) == -1001 and topk(tok=None) == -1001 and topk(fwd=None) == -1001 and topk(keep=None) == -1001
    assert topk(top=None) == -1001 and topk(ts=None) == -1001
    assert topk(K=0) == -1002 and topk(K=L.TOPK_MAX_K + 1) == -1002
    assert topk(ex=ex, E=L.TOPK_MAX_EXCLUDE + 1) == -1003
    assert topk(ldt=Ls - 1) == -1004 and topk(ldf=Ls - 1) == -1004 and topk(ldq=Tq - 1) == -1004
    assert topk(ns=65) == -1005
    assert topk(ns=2, ws=ws2, nb=U * 2 * K * 8 - 1) == -1006 and topk(ns=2, ws=None, nb=U * 2 * K * 8) == -1006
    assert topk(V=3_000_000) == -1007                                 # the users' bitmaps exceed the LDS
    assert topk(U=0, q=None, top=None, ts=None) == 0                  # no users: nothing to do
    torch.cuda.synchronize()
    assert (top == -77).all() and (ts == 123.0).all()
    assert topk() == 0 and topk(ns=2, ws=ws2, nb=U * 2 * K * 8) == 0  # the valid calls: nothing is kept, all -1
    torch.cuda.synchronize()
    assert (top == -1).all() and torch.isneginf(ts).all()


def test_wrapper_argument_checks(corpora):
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import build_bm25_index, sparse_topk_news
    tok, ix, _ = corpora[63]
    t = _dev(tok)
    for bad in (t.long(), t[0], torch.zeros(4, 65, dtype=torch.int32, device=DEV), t[:, ::2]):
        with pytest.raises(L.HipError):
            build_bm25_index(bad, vocab=200)
    for kw in ({"postings": 0}, {"postings": L.BM25_MAX_POSTINGS + 1}, {"k": 0}, {"vocab": 0}, {"special": (0, 1)}):
        with pytest.raises(L.HipError):
            build_bm25_index(t, **{"vocab": 200, **kw})
    q = torch.ones(3, 4, dtype=torch.int32, device=DEV)
    for bad in (q.long(), q.cpu(), q[0]):
        with pytest.raises(L.HipError):
            sparse_topk_news(ix, bad, 5)
    for k in (0, L.TOPK_MAX_K + 1):
        with pytest.raises(L.HipError):
            sparse_topk_news(ix, q, k)
    with pytest.raises(L.HipError):
        sparse_topk_news(ix, q, 5, row_mask=torch.ones(62, dtype=torch.uint8, device=DEV))
    with pytest.raises(L.HipError):
        sparse_topk_news(ix, q, 5, row_mask=torch.ones(63, dtype=torch.bool, device=DEV))
    with pytest.raises(L.HipError):
        sparse_topk_news(ix, q, 5, exclude=torch.zeros(2, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(L.HipError):
        sparse_topk_news(ix, q, 5, exclude=torch.zeros(3, L.TOPK_MAX_EXCLUDE + 1, dtype=torch.int64, device=DEV))
    ids, sc = sparse_topk_news(ix, q[:0], 5)
    assert ids.shape == (0, 5) and sc.shape == (0, 5)


# ------------------------------------------------------------------------------------------------ e2e
def test_end_to_end_recommend(tmp_path):
    from newsrec_amd import evaluate as EV
    from newsrec_amd.manager import build_model
    from newsrec_amd.mind import MINDStore
    news, beh, opts = load_data()
    st = MINDStore(news, beh["dev"], "dev", device=DEV, **opts)
    tok = st.tok.cpu().numpy()
    n_impr = len(st.grp_off_host) - 1
    x = st.eval_batch(0, len(st))
    rows = torch.from_numpy(st.first_chunk_host).to(DEV)
    his_id = x["his_id"][rows].reshape(n_impr, -1)
    his_mask = x["his_mask"][rows].reshape(n_impr, -1)
    q = EV.history_tokens(st, x["his_id"][rows], x["his_mask"][rows])
    want_q = BU.history_tokens(tok, his_id.cpu().numpy(), his_mask.cpu().numpy())
    assert q.dtype == torch.int32 and q.shape == (n_impr, st.his_size * st.signal_length)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    assert (his_mask.cpu().numpy() == 0).any()

    index = EV.build_bm25_index(st.tok)
    w = BU.build(tok, 30522, 100, 2)
    _check_index(index, w, tok.shape[0])
    impressed = np.zeros(tok.shape[0], np.uint8)
    impressed[np.unique(st.cand_ids.cpu().numpy())] = 1
    his = his_id.cpu().numpy().astype(np.int64)
    for candidates, mask in (("impressed", impressed), ("all", None)):
        for exclude in (True, False):
            want = BU.expected_topk(tok, w.fwd, w.keep, want_q, 30522, 10, 1, mask, his if exclude else None)
            for batch, bm25 in ((len(st), index), (3, None)):
                got = EV.recommend(None, st, k=10, batch_impr=batch, candidates=candidates, exclude_history=exclude,
                                   recall_type="s", bm25=bm25)
                ids, _ = _same(got, want)
    assert (ids >= 1).any()
    m = EV.recall_metrics(got[0], st, ks=(5, 10))
    assert m["n_impr_scored"] > 0 and 0.0 <= m["recall@5"] <= m["recall@10"] <= 1.0

    # the saved index serves the same search
    back = EV.BM25Index.load(index.save(str(tmp_path / "bm25")), device=DEV)
    _same(EV.recommend(None, st, k=10, candidates="all", exclude_history=False, recall_type="s", bm25=back), want)

    # dense recall is what it was, and "sd" is the merge of the two
    torch.manual_seed(11)
    model = build_model("cnn", "attn", 150, vocab=30522, device=DEV, user_num=600, dropout_p=0.2).eval()
    table = EV.encode_news_table(model, st)
    d0 = EV.recommend(model, st, k=10, news_table=table)
    d1 = EV.recommend(model, st, k=10, news_table=table, recall_type="d")
    assert torch.equal(d0[0], d1[0]) and torch.equal(d0[1], d1[1])
    s = EV.recommend(None, st, k=10, recall_type="s", bm25=index)
    sd, none = EV.recommend(model, st, k=10, news_table=table, recall_type="sd", bm25=index)
    assert none is None and sd.shape == (n_impr, 20) and sd.dtype == torch.int64
    np.testing.assert_array_equal(sd.cpu().numpy(), BU.merge_recall(s[0].cpu().numpy(), d0[0].cpu().numpy()))
    assert torch.equal(sd, EV.merge_recall(s[0], d0[0]))
    with pytest.raises(ValueError):
        EV.recommend(model, st, recall_type="x")
    with pytest.raises(ValueError):
        EV.recommend(None, st, recall_type="s", bm25=_host_index(tok[:-1], 30522, 100)[0])
