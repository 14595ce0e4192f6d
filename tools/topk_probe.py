"""Times the full-corpus top-K search of one eval batch two ways on the same data, in the same process:

  (a) evaluate.topk_news (csrc/topk.hip: fused score / select, the [U, N] scores never reach HBM); the
      wrapper as callers use it, i.e. with its workspace allocation and its status read
  (b) the torch composition  torch.topk(user @ table.T * scale, K)  with the ineligible rows (row 0)
      set to -inf, which writes and re-reads the [U, N] fp32 score matrix

at the MIND dev shapes U = 1024, N = 72,024 with (H = 384, K = 100) and (H = 150, K = 10).  The parent
of this path has no retrieval at all, so (b) is the baseline.  Each variant is warmed up, then timed
with device events over `--rounds` alternating rounds of several calls; the medians are reported.
"kernel_ms" is the raw nr_topk_news entry alone (both launches, buffers preallocated) and gives the
achieved TF/s of the 2 U N H score FLOPs against the 157.3 TF fp32-MFMA peak.  Also reports how far the
two results agree (different summation orders: near-ties may swap).  Prints one JSON line per shape.

python tools/topk_probe.py [--users 1024] [--news 72024] [--rounds 7] [--seed 0]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "news-recommendation-mind_amd"))

import numpy as np
import torch

from newsrec_amd import _lib as L
from newsrec_amd import evaluate as EV

PEAK_TF = 157.3


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def probe(U, N, H, K, rounds, seed):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.randn(N, H, device=dev, generator=g)
    user = torch.randn(U, H, device=dev, generator=g)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(H)))

    def a():
        return EV.topk_news(table, user, K, first_row=1)

    def b():
        s = user @ table.T
        s *= scale
        s[:, 0] = float("-inf")
        return torch.topk(s, K)

    ids = torch.empty(U, K, dtype=torch.int64, device=dev)
    sc = torch.empty(U, K, dtype=torch.float32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = int(L.load().nr_topk_workspace(U, N, K, 0))
    ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=dev)

    def kern():
        L.call("nr_topk_news", L.ptr(table), table.stride(0), N, L.ptr(user), user.stride(0), U, H, K, 1, None, None, 0,
               0, L.ptr(ids), L.ptr(sc), L.ptr(ws), nb, L.ptr(st), L.stream_ptr(table))

    for fn in (a, b, kern):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # calls per round: about 0.1 s of each variant
    reps = {fn: max(3, int(100.0 / max(timed(fn, 3), 1e-3))) for fn in (a, b, kern)}
    t = {fn: [] for fn in (a, b, kern)}
    for _ in range(rounds):
        for fn in (a, b, kern):
            t[fn].append(timed(fn, reps[fn]))
    a_ms, b_ms, k_ms = (float(np.median(t[fn])) for fn in (a, b, kern))

    ia, sa = a()
    sb, ib = b()
    same = (ia == ib).float().mean().item()
    tf = 2.0 * U * N * H / (k_ms * 1e-3) / 1e12
    return {"U": U, "N": N, "H": H, "K": K, "slices": nb // (U * K * 8), "topk_news_ms": round(a_ms, 4),
            "torch_mm_topk_ms": round(b_ms, 4), "torch_over_topk_news": round(b_ms / a_ms, 2),
            "kernel_ms": round(k_ms, 4), "kernel_TFs": round(tf, 1), "peak_fraction": round(tf / PEAK_TF, 3),
            "topk_news_min_ms": round(min(t[a]), 4), "torch_min_ms": round(min(t[b]), 4),
            "calls_per_round": [reps[a], reps[b], reps[kern]], "rounds": rounds,
            "ids_equal_fraction": round(same, 5), "max_score_diff": float((sa - sb).abs().max().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--news", type=int, default=72024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_probe needs the GPU")
    for H, K in ((384, 100), (150, 10)):
        print(json.dumps(probe(a.users, a.news, H, K, a.rounds, a.seed)), flush=True)


if __name__ == "__main__":
    main()
