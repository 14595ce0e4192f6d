"""Times sparse (BM25) recall on a synthetic corpus of MIND's size, in one process:

  build   evaluate.build_bm25_index (csrc/bm25.hip: count, host idf, scatter / select, per-news view) of
          R = 72,024 rows of L = 30 Zipf-distributed tokens over V = 30522, P = 100; wall time with the
          device-to-host copy of the counts and the host idf, median of `--builds` runs, and the device
          time of the four entries alone
  query   (a) evaluate.sparse_topk_news for U = 1,024 users whose queries are the tokens of 50 history rows
              each (Tq = 1,500), K = 10 and K = 100; the wrapper as callers use it, also with the 50
              history ids as exclude list, as recommend passes them
          (b) the torch composition on the same index: the users' distinct tokens gather their posting
              lists, index_put_(accumulate=True) adds the scores into a [U, R + 1] fp32 matrix (and marks
              the rows that matched), torch.topk selects
          The parent of this path has no sparse recall, so (b) is the baseline.  Both are warmed up, then
          timed with device events over `--rounds` alternating rounds; medians are reported.  "kernel_ms" is
          the raw nr_bm25_topk entry alone (buffers preallocated) and gives the membership tests per
          second (U x kept columns of all rows).  (b) sums with float atomics in no fixed order, so the two
          agree up to fp32 rounding: the fraction of equal ids is reported, not asserted.

Prints one JSON line for the build and one per K.

python tools/bm25_probe.py [--users 1024] [--news 72024] [--rounds 7] [--builds 3] [--seed 0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "news-recommendation-mind_amd"))

import numpy as np
import torch

from newsrec_amd import _lib as L
from newsrec_amd import evaluate as EV

V, LEN, P, HIS = 30522, 30, 100, 50


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def corpus(R, rng):
    """[CLS] words [SEP] pad..., 8 .. 30 tokens a row, word ranks Zipf(1) over ids 1000 .. V - 1; row 0 pad."""
    words = np.arange(1000, V)
    p = 1.0 / np.arange(1, len(words) + 1)
    p /= p.sum()
    tok = rng.choice(words, (R, LEN), p=p).astype(np.int32)
    length = rng.integers(8, LEN + 1, R)
    col = np.arange(LEN)[None, :]
    tok[col >= length[:, None]] = 0
    tok[np.arange(R), length - 1] = 102
    tok[:, 0] = 101
    tok[0] = 0
    return tok


def probe_build(tok, builds):
    dev = tok.device
    R = tok.shape[0]
    wall = []
    for _ in range(builds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = EV.build_bm25_index(tok, vocab=V, postings=P)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    # the four entries alone, from the index's own idf
    df = torch.empty(V, dtype=torch.int64, device=dev)
    n_post = torch.empty(V, dtype=torch.int32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = int(L.load().nr_bm25_build_workspace(R, LEN, V))
    ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
    ids, sc = torch.empty_like(index.post_ids), torch.empty_like(index.post_scores)
    fwd, keep = torch.empty_like(index.fwd), torch.empty_like(index.keep)
    S = L.stream_ptr(tok)
    steps = {
        "count_ms": lambda: L.call("nr_bm25_count", L.ptr(tok), LEN, R, LEN, V, 0, 101, 102, L.ptr(df), L.ptr(n_post),
                                   L.ptr(st), S),
        "build_ms": lambda: L.call("nr_bm25_build", L.ptr(tok), LEN, R, LEN, V, P, 2, 0, 101, 102, L.ptr(index.idf),
                                   L.ptr(n_post), L.ptr(ids), L.ptr(sc), L.ptr(ws), nb, S),
        "forward_ms": lambda: L.call("nr_bm25_forward", L.ptr(tok), LEN, R, LEN, V, P, L.ptr(ids), L.ptr(sc),
                                     L.ptr(fwd), LEN, L.ptr(keep), S),
    }
    out = {"R": R, "L": LEN, "V": V, "P": P, "build_wall_ms": round(float(np.median(wall[1:])), 3),
           "build_wall_first_ms": round(wall[0], 3)}
    for name, fn in steps.items():
        fn()
        out[name] = round(float(np.median([timed(fn, 3) for _ in range(builds)])), 4)
    assert torch.equal(ids, index.post_ids) and torch.equal(keep, index.keep)
    n_post_h = n_post.cpu().numpy()
    out.update(postings=int(np.minimum(n_post_h, P).sum()), postings_before_cut=int(n_post_h.sum()),
               longest_list=int(n_post_h.max()), tokens_with_postings=int((n_post_h > 0).sum()))
    return index, out


def probe_query(index, qtok, K, rounds, his):
    dev = qtok.device
    U, R = qtok.shape[0], index.n_rows
    scores32 = index.post_scores.to(torch.float32)
    post_ids = index.post_ids.long()

    def a():
        return EV.sparse_topk_news(index, qtok, K, first_row=1)

    def a_ex():                                                       # as recommend calls it: the history excluded
        return EV.sparse_topk_news(index, qtok, K, first_row=1, exclude=his)

    def b():
        member = torch.zeros(U, V, dtype=torch.bool, device=dev)
        member.scatter_(1, qtok.long(), True)
        member[:, [0, 101, 102]] = False
        u, t = member.nonzero(as_tuple=True)
        rows = post_ids[t]                                           # [pairs, P], padding = R
        s = torch.zeros(U, R + 1, device=dev)
        hit = torch.zeros(U, R + 1, dtype=torch.bool, device=dev)
        uu = u[:, None].expand_as(rows)
        s.index_put_((uu, rows), scores32[t], accumulate=True)
        hit[uu, rows] = True
        s.masked_fill_(~hit, float("-inf"))
        s[:, 0] = float("-inf")
        return torch.topk(s[:, :R], K)

    ids = torch.empty(U, K, dtype=torch.int64, device=dev)
    sc = torch.empty(U, K, dtype=torch.float32, device=dev)
    nb = int(L.load().nr_bm25_topk_workspace(U, R, K, 0))
    ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=dev)

    def kern():
        L.call("nr_bm25_topk", L.ptr(qtok), qtok.stride(0), U, qtok.shape[1], L.ptr(index.tok), LEN, L.ptr(index.fwd),
               LEN, L.ptr(index.keep), R, LEN, V, 0, 101, 102, K, 1, None, None, 0, 0, L.ptr(ids), L.ptr(sc), L.ptr(ws),
               nb, L.stream_ptr(qtok))

    fns = (a, b, kern, a_ex)
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    reps = {fn: max(2, min(200, int(100.0 / max(timed(fn, 2), 1e-3)))) for fn in fns}
    t = {fn: [] for fn in fns}
    for _ in range(rounds):
        for fn in fns:
            t[fn].append(timed(fn, reps[fn]))
    a_ms, b_ms, k_ms, x_ms = (float(np.median(t[fn])) for fn in fns)
    ia, sa = a()
    sb, ib = b()
    kept_cols = int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in index.keep.cpu().tolist()))
    tests = float(U) * kept_cols
    both = torch.isfinite(sa) & torch.isfinite(sb)
    return {"U": U, "R": R, "Tq": qtok.shape[1], "K": K, "slices": nb // (U * K * 8),
            "sparse_topk_news_ms": round(a_ms, 4), "torch_index_put_topk_ms": round(b_ms, 4),
            "torch_over_sparse_topk_news": round(b_ms / a_ms, 2), "kernel_ms": round(k_ms, 4),
            "sparse_topk_news_exclude%d_ms" % his.shape[1]: round(x_ms, 4),
            "membership_tests": tests, "G_tests_per_s": round(tests / (k_ms * 1e-3) / 1e9, 1),
            "sparse_topk_news_min_ms": round(min(t[a]), 4), "torch_min_ms": round(min(t[b]), 4),
            "calls_per_round": [reps[a], reps[b], reps[kern]], "rounds": rounds,
            "ids_equal_fraction": round((ia == ib).float().mean().item(), 5),
            "max_score_diff": float((sa - sb)[both].abs().max().item()) if both.any() else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--news", type=int, default=72024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bm25_probe needs the GPU")
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda", 0)
    tok = torch.from_numpy(corpus(a.news, rng)).to(dev)
    index, res = probe_build(tok, a.builds)
    print(json.dumps(res), flush=True)
    his = torch.from_numpy(rng.integers(1, a.news, (a.users, HIS))).to(dev)
    his_mask = torch.from_numpy((rng.random((a.users, HIS)) < 0.8).astype(np.float32)).to(dev)
    store = argparse.Namespace(tok=tok)
    qtok = EV.history_tokens(store, his, his_mask)
    for K in (10, 100):
        print(json.dumps(probe_query(index, qtok, K, a.rounds, his)), flush=True)


if __name__ == "__main__":
    main()
