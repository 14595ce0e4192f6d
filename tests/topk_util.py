"""The expected result of evaluate.topk_news built from its definition, and the property check for
real-valued data (no GPU, numpy only).

  score      float64 dot product of the fp32 inputs times the fp32 scale 1 / sqrt(H)
  eligible   row >= first_row, row_mask[row] != 0, row not among the user's exclude ids
  order      stable sort by (-score, id) over the eligible rows; the tail is id -1 / score -inf
"""
import numpy as np


def scale32(H):
    return np.float32(1.0) / np.sqrt(np.float32(H))


def scores64(table, user):
    """[U, N] float64 scores of fp32 inputs."""
    H = table.shape[1]
    return (user.astype(np.float64) @ table.astype(np.float64).T) * np.float64(scale32(H))


def eligible(U, N, first_row=1, row_mask=None, exclude=None):
    """bool [U, N]"""
    ok = np.zeros((U, N), bool)
    ok[:, min(first_row, N):] = True
    if row_mask is not None:
        ok &= (np.asarray(row_mask) != 0)[None, :]
    if exclude is not None:
        ex = np.asarray(exclude)
        for u in range(U):
            e = ex[u][(ex[u] >= 0) & (ex[u] < N)]
            ok[u, e] = False
    return ok


def expected(table, user, k, first_row=1, row_mask=None, exclude=None):
    """-> (ids int64 [U, k], scores float32 [U, k]); the scores are the float64 scores rounded to fp32,
    which for integer-valued inputs is the fp32 product (exact dot) * scale bit for bit."""
    U, N = user.shape[0], table.shape[0]
    s = scores64(table, user)
    ok = eligible(U, N, first_row, row_mask, exclude)
    ids = np.full((U, k), -1, np.int64)
    sc = np.full((U, k), -np.inf, np.float32)
    for u in range(U):
        rows = np.flatnonzero(ok[u])                          # ascending ids
        order = rows[np.argsort(-s[u, rows], kind="stable")][:k]
        ids[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order].astype(np.float32)
    return ids, sc


def dot_tolerance(absdot, dot, H):
    """Bound on |fp32 score - float64 score| of one H-term dot product given sum_k |u_k t_k| and
    sum_k u_k t_k in float64: the gamma_H bound of an H-term fp32 fma chain, 2 H 2^-24 sum_k |u_k t_k|,
    plus the rounding of the scale multiply, 2^-23 |s|, times the scale.  (Shared with
    score_util.score_tolerance, the scorer kernels' bound.)"""
    return (2.0 * H * 2.0 ** -24 * absdot + 2.0 ** -23 * np.abs(dot)) * np.float64(scale32(H))


def tolerances(table, user):
    """[U, N] dot_tolerance of every (user, table row) pair."""
    H = table.shape[1]
    t64, u64 = table.astype(np.float64), user.astype(np.float64)
    absdot = np.abs(u64) @ np.abs(t64).T
    dot = u64 @ t64.T
    return dot_tolerance(absdot, dot, H)


def check_properties(table, user, ids, scores, k, first_row=1, row_mask=None, exclude=None):
    """Asserts that (ids, scores) is a valid top-k of real-valued inputs up to fp32 rounding:
    ordered, every score within tol of its id's float64 score, no eligible row left out that beats the
    k-th returned score by more than the two tolerances, no duplicates, fillers only at the tail."""
    U, N = user.shape[0], table.shape[0]
    assert ids.shape == (U, k) and scores.shape == (U, k)
    s = scores64(table, user)
    tol = tolerances(table, user)
    ok = eligible(U, N, first_row, row_mask, exclude)
    for u in range(U):
        n_real = min(k, int(ok[u].sum()))
        got, sc = ids[u], scores[u]
        assert (got[n_real:] == -1).all() and np.isneginf(sc[n_real:]).all(), u
        got, sc = got[:n_real], sc[:n_real]
        assert ((got >= 0) & (got < N)).all() and ok[u, got].all(), u
        assert len(set(got.tolist())) == n_real, u
        d = np.diff(sc)
        assert (d <= 0).all(), u
        assert (np.diff(got)[d == 0] > 0).all(), u
        assert (np.abs(sc.astype(np.float64) - s[u, got]) <= tol[u, got]).all(), u
        if n_real == k:
            rest = ok[u].copy()
            rest[got] = False
            kth = got[-1]
            assert (s[u, rest] <= np.float64(sc[-1]) + tol[u, rest] + tol[u, kth]).all(), u
