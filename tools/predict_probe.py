"""Times the prediction.txt text of a MIND-shaped test split two ways and checks they agree:

  (a) the device path: nr_rank_ordinal, the prefix sum of the line lengths, nr_format_prediction and
      the copy of the text to pinned host memory (warmed up, synchronised, repeated past 0.5 s)
  (b) the reference's formulation on the host (Manager.test, utils/Manager.py:842-850): the same scores
      after .tolist(), one scipy.stats.rankdata and one string join per impression (run once)

File I/O is outside both.  Also times the format kernel alone (device events) for its output rate.
Prints one JSON line.  python tools/predict_probe.py [--groups 262144] [--seed 0]"""
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


def synthetic(G, seed):
    """Group sizes with mean ~37 clipped to [1, 300] (a log-normal, as MIND's long tail); scores are
    fp32 sigmoids of N(0, 4) logits."""
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.rint(rng.lognormal(np.log(37.0) - 0.32, 0.8, G)), 1, 300).astype(np.int64)
    off = np.zeros(G + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    logits = rng.normal(0.0, 4.0, int(off[-1])).astype(np.float32)
    preds = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
    return preds, off


def device_path(preds, grp_off, host):
    rank, line_len = EV.rank_ordinal(preds, grp_off, 1)
    line_off = EV._line_offsets(line_len)
    total = int(line_off[-1].item())
    text = torch.empty(total, dtype=torch.uint8, device=preds.device)
    EV._format(rank, grp_off, line_off, 1, text, total)
    host[:total].copy_(text, non_blocking=True)
    torch.cuda.synchronize()
    return total, (rank, line_off, text)


def host_path(preds, off):
    import scipy.stats as ss
    pl = preds.tolist()
    out, index = [], 1
    for g in range(len(off) - 1):
        array = np.asarray(pl[off[g]:off[g + 1]])
        rank_list = ss.rankdata(1 - array, method="ordinal")
        out.append(str(index) + " [" + ",".join([str(i) for i in rank_list]) + "]" + "\n")
        index += 1
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=262144)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    p_np, off_np = synthetic(a.groups, a.seed)
    preds, grp_off = torch.from_numpy(p_np).to(dev), torch.from_numpy(off_np).to(dev)

    host = torch.empty(16 * len(p_np) + 32 * a.groups, dtype=torch.uint8, pin_memory=True)
    for _ in range(3):
        total, (rank, line_off, text) = device_path(preds, grp_off, host)
    reps, t_dev = 0, 0.0
    while t_dev < 0.6 or reps < 10:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_path(preds, grp_off, host)
        t_dev += time.perf_counter() - t0
        reps += 1
    a_ms = 1e3 * t_dev / reps

    # the format kernel alone
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_reps = 50
    ev[0].record()
    for _ in range(k_reps):
        EV._format(rank, grp_off, line_off, 1, text, total)
    ev[1].record()
    torch.cuda.synchronize()
    fmt_ms = ev[0].elapsed_time(ev[1]) / k_reps
    ev[0].record()
    for _ in range(k_reps):
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        L.call("nr_rank_ordinal", L.ptr(preds), L.ptr(grp_off), a.groups, 1, 300, L.ptr(rank),
               L.ptr(torch.empty(a.groups, dtype=torch.int64, device=dev)), L.ptr(st), L.stream_ptr(preds))
    ev[1].record()
    torch.cuda.synchronize()
    rank_ms = ev[0].elapsed_time(ev[1]) / k_reps

    got = bytes(host[:total].numpy().tobytes())
    t0 = time.perf_counter()
    want = host_path(p_np, off_np)
    b_ms = 1e3 * (time.perf_counter() - t0)
    assert got == want.encode("ascii"), "device text differs from the host formulation"
    print(json.dumps({"groups": a.groups, "candidates": int(len(p_np)), "text_bytes": total,
                      "device_ms": round(a_ms, 3), "device_reps": reps, "host_ms": round(b_ms, 1),
                      "host_over_device": round(b_ms / a_ms, 1), "rank_kernel_ms": round(rank_ms, 4),
                      "format_kernel_ms": round(fmt_ms, 4),
                      "format_output_GBps": round(total / fmt_ms / 1e6, 1)}))


if __name__ == "__main__":
    main()
