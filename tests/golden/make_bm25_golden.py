"""Writes tests/golden/bm25_index.npz: a small token corpus and the inverted index that the REFERENCE's
own code builds from it,

    construct_inverted_index(corpus, BM25_token(corpus))        (utils/utils.py:219-246, :287-342)

The script imports the reference read-only and runs it in a temporary working directory that has
data/recall/ (the reference saves its .pt there).  The reference's array is [30522, 100, 2] float64;
only the tokens that have postings are stored, as ids (int32), scores (float64) and BM25_token's idf.

The corpus (401 rows of 12 columns, about 60 distinct tokens) holds the cases the index can go wrong on;
main() asserts each of them:
  an all-pad row 0; rows of every length 1 .. L; [SEP] in the last column of full rows; a token with more
  than 3 P postings, one with exactly P, one with P + 1; a token whose occurrence count exceeds the row
  count (negative idf); non-[CLS] tokens in column 0, one that occurs nowhere else (idf 0.0, score 0.0)
  and one with negative idf and no other occurrence in its row (score -0.0).

    python tests/golden/make_bm25_golden.py --ref <reference checkout>
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
R, L, V, P, K = 401, 12, 30522, 100, 2
PAD, CLS, SEP = 0, 101, 102
COMMON, EXACT_P, P_PLUS_1, ONLY_COL0 = 1000, 2000, 2001, 3000
WORDS = np.arange(1001, 1053)        # the Zipf-distributed rest


def corpus():
    rng = np.random.default_rng(2502)
    tok = np.zeros((R, L), np.int64)
    w = 1.0 / np.arange(1, len(WORDS) + 1)
    w /= w.sum()
    for n in range(1, R):
        length = n if n <= L else int(rng.integers(3, L + 1))      # rows 1 .. 12: every length
        row = [CLS]
        while len(row) < length - 1:
            u = rng.random()
            # the common token: most rows, often more than once
            row.append(COMMON if u < 0.45 else int(rng.choice(WORDS, p=w)))
        if length >= 2:
            row.append(SEP)
        tok[n, :len(row)] = row
    body = [n for n in range(20, R) if (tok[n] != PAD).sum() >= 4]
    for t, count, start in ((EXACT_P, P, 0), (P_PLUS_1, P + 1, 1)):
        for n in body[start::2][:count]:
            tok[n, 1 + (n % 2)] = t
    # column 0 without [CLS]
    for n in (30, 31, 32):
        tok[n, 0] = ONLY_COL0
    for n in (40, 41, 42, 43):
        tok[n, 0] = COMMON
        tok[n, 1:][tok[n, 1:] == COMMON] = WORDS[3]                  # ... and nowhere else in the row: tf = 0
    tok[50, 0] = int(WORDS[0])
    return tok


def main(ref, out_dir):
    sys.path.insert(0, ref)
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    tok = corpus()
    docs = [[int(t) for t in row] for row in tok]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("data/recall")
            from utils.utils import BM25_token, construct_inverted_index
            bm = BM25_token(docs, k=K)
            arr = construct_inverted_index(docs, bm).numpy()
        finally:
            os.chdir(cwd)
    assert arr.shape == (V, P, 2) and arr.dtype == np.float64
    ids, sc = arr[:, :, 0], arr[:, :, 1]
    tokens = np.flatnonzero((ids != R).any(1)).astype(np.int32)
    idf = np.array([bm.idf[int(t)] for t in tokens], np.float64)
    n_post = {int(t): int((tok == t).any(1).sum()) for t in tokens}
    df = {int(t): int((tok[:, 1:] == t).sum()) for t in tokens}

    # the cases the corpus is there for
    assert (tok[0] == PAD).all()
    lengths = (tok != PAD).sum(1)
    assert set(range(1, L + 1)) <= set(lengths.tolist())
    assert (tok[lengths == L, L - 1] == SEP).all() and (lengths == L).sum() > 10
    assert n_post[COMMON] > 3 * P and n_post[EXACT_P] == P and n_post[P_PLUS_1] == P + 1
    assert df[COMMON] > R and bm.idf[COMMON] < 0
    assert df[ONLY_COL0] == 0 and bm.idf[ONLY_COL0] == 0.0 and n_post[ONLY_COL0] == 3
    neg_zero = (sc == 0) & np.signbit(sc)
    assert neg_zero[COMMON].sum() == 4 and sorted(ids[COMMON][neg_zero[COMMON]].tolist()) == [40, 41, 42, 43]
    assert (sc[ONLY_COL0][:3] == 0).all() and not np.signbit(sc[ONLY_COL0]).any()
    assert not (set(tokens.tolist()) & {PAD, CLS, SEP}) and 50 < len(tokens) < 70
    assert (sc[tokens] < 0).sum() >= P - 4 and ((sc[tokens] == 0) & (ids[tokens] != R)).sum() >= 7

    path = os.path.join(out_dir, "bm25_index.npz")
    np.savez_compressed(path, tok=tok.astype(np.int32), meta=np.array([V, P, K], np.int64), tokens=tokens,
                        post_ids=ids[tokens].astype(np.int32), post_scores=sc[tokens], idf=idf)
    print("wrote", path, len(tokens), "tokens with postings,", int((ids[tokens] != R).sum()), "postings,",
          int(neg_zero.sum()), "scores of -0.0,", os.path.getsize(path), "bytes on disk")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("NEWSREC_REFERENCE"), required="NEWSREC_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    main(a.ref, a.out)
