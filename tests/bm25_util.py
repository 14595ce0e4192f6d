"""The token-level BM25 index, its per-news view, the sparse scores, their top-K and merge_recall,
restated from the definition in include/newsrec_hip.h (numpy and plain Python, no GPU).

  df[t], tf[n][t]  occurrences in columns 1 .. L-1 (occurrences, not documents; pad and [SEP] count)
  idf[t]           math.log((R - df + 0.5) / (df + 0.5) + 1) where df > 0, else 0.0
  posting          row n posts every non-special in-range token that occurs anywhere in it (column 0
                   included): s = ((idf * tf) * (k + 1)) / (tf + k) in float64, in that order
  list             sorted(postings in row order, key=score, reverse=True)[:P]  (stable: ties by row)
  fwd / keep       the kept postings at their token's first column of the row, rounded once to fp32
  sparse score     sequential float32 sum, from 0, in column order over the kept columns whose token the
                   user holds; eligible when at least one matched
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bm25_index.npz")
SPECIAL = (0, 101, 102)


def load_golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g["V"], g["P"], g["k"] = (int(v) for v in g.pop("meta"))
    return g


def dense_from_golden(g):
    """The reference's [V, P, 2] float64 array rebuilt from the sparse fixture."""
    R = g["tok"].shape[0]
    arr = np.zeros((g["V"], g["P"], 2))
    arr[:, :, 0] = R
    arr[g["tokens"], :, 0] = g["post_ids"]
    arr[g["tokens"], :, 1] = g["post_scores"]
    return arr


class Index:
    """df int64 [V], idf float64 [V], post_ids int32 [V, P], post_scores float64 [V, P], fwd float32 [R, L],
    keep uint64 [R], bad (a token outside [0, V) was met)."""


def build(tok, V, P=100, k=2, special=SPECIAL):
    tok = np.asarray(tok)
    R, L = tok.shape
    rows = [[int(t) for t in row] for row in tok]
    ix = Index()
    ix.bad = any(not 0 <= t < V for row in rows for t in row)
    ix.df = np.zeros(V, np.int64)
    tfs = []
    for row in rows:
        tf = {}
        for t in row[1:]:
            if 0 <= t < V:
                tf[t] = tf.get(t, 0) + 1
                ix.df[t] += 1
        tfs.append(tf)
    ix.idf = np.zeros(V, np.float64)
    for t in np.flatnonzero(ix.df):
        d = int(ix.df[t])
        ix.idf[t] = math.log((R - d + 0.5) / (d + 0.5) + 1)
    lists = {}
    for n, row in enumerate(rows):
        seen = set()
        for t in row:
            if 0 <= t < V and t not in special and t not in seen:
                seen.add(t)
                tf = tfs[n].get(t, 0)
                lists.setdefault(t, []).append((n, ((float(ix.idf[t]) * tf) * (k + 1)) / (tf + k)))
    ix.post_ids = np.full((V, P), R, np.int32)
    ix.post_scores = np.zeros((V, P), np.float64)
    ix.n_post = np.zeros(V, np.int32)
    ix.fwd = np.zeros((R, L), np.float32)
    ix.keep = np.zeros(R, np.uint64)
    for t, v in lists.items():
        ix.n_post[t] = len(v)
        v = sorted(v, key=lambda x: x[1], reverse=True)[:P]
        for p, (n, s) in enumerate(v):
            ix.post_ids[t, p] = n
            ix.post_scores[t, p] = s
            col = rows[n].index(t)
            ix.fwd[n, col] = np.float32(s)
            ix.keep[n] |= np.uint64(1 << col)
    return ix


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def sparse_scores(tok, fwd, keep, qtok, V, special=SPECIAL):
    """-> (scores float32 [U, R], matched bool [U, R])"""
    tok = np.asarray(tok)
    R, L = tok.shape
    U = len(qtok)
    kept = ((keep[:, None] >> np.arange(L, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    s = np.zeros((U, R), np.float32)
    matched = np.zeros((U, R), bool)
    for u in range(U):
        q = np.array(sorted({int(t) for t in qtok[u] if 0 <= t < V and t not in special}), np.int64)
        member = np.isin(tok, q) & kept
        for col in range(L):
            s[u] = np.where(member[:, col], s[u] + fwd[:, col], s[u])          # float32 + float32
        matched[u] = member.any(1)
    return s, matched


def expected_topk(tok, fwd, keep, qtok, V, K, first_row=1, row_mask=None, exclude=None, special=SPECIAL):
    """-> (ids int64 [U, K], scores float32 [U, K]): score descending, id ascending, tail -1 / -inf."""
    s, ok = sparse_scores(tok, fwd, keep, qtok, V, special)
    U, R = s.shape
    ok[:, :min(first_row, R)] = False
    if row_mask is not None:
        ok &= (np.asarray(row_mask) != 0)[None, :]
    if exclude is not None:
        for u in range(U):
            e = np.asarray(exclude[u])
            ok[u, e[(e >= 0) & (e < R)]] = False
    ids = np.full((U, K), -1, np.int64)
    sc = np.full((U, K), -np.inf, np.float32)
    for u in range(U):
        rows = np.flatnonzero(ok[u])
        order = rows[np.argsort(-s[u, rows].astype(np.float64), kind="stable")][:K]
        ids[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order]
    return ids, sc


def history_tokens(tok, his_id, his_mask):
    U = his_id.shape[0]
    t = np.asarray(tok)[his_id.reshape(U, -1)].copy()
    t[his_mask.reshape(U, -1) == 0] = 0
    return t.reshape(U, -1).astype(np.int32)


def merge_recall(a, b):
    a, b = np.asarray(a), np.asarray(b)
    out = np.full((a.shape[0], a.shape[1] + b.shape[1]), -1, np.int64)
    for u in range(a.shape[0]):
        taken = []
        for i in range(max(a.shape[1], b.shape[1])):
            for src in (a, b):
                if i < src.shape[1] and src[u, i] >= 0 and int(src[u, i]) not in taken:
                    taken.append(int(src[u, i]))
        out[u, :len(taken)] = taken
    return out
