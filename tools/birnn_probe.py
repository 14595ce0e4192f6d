"""Times the recurrence of the bidirectional-LSTM news encoder two ways on the same data, in the same
process, at the train size nseq = 1,760 titles (B = 32 x (5 candidates + 50 history)), L = 30, H = 150:

  (new)   nr_birnn_fwd (no tokens) + nr_birnn_bwd (dnews only): 16 sequences of one direction per
          workgroup, both directions in one launch (csrc/birnn.hip)
  (base)  what the library offered before: nr_rnn_fwd + nr_rnn_bwd (one workgroup per sequence, LSTM,
          no mask) called twice, reverse = 0 and 1, over the same sequences -- the same numbers up to
          the 1/2 (-> + <-) sums

Each variant is warmed up, then timed with device events over `--rounds` interleaved rounds
(base, new, base'), several calls each; medians are reported.  The noise floor is the spread between
the two timings of the baseline itself (base vs base').  Also times one rnn + attn train step at
B = 32 (eager and as a graph replay) unless --no-step.  Prints one JSON line.

python tools/birnn_probe.py [--nseq 1760] [--len 30] [--hidden 150] [--rounds 7] [--no-step]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "news-recommendation-mind_amd"))

import numpy as np
import torch

from newsrec_amd import _lib as L
from newsrec_amd import kernels as K


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def recurrence(nseq, seq_len, H, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    T = nseq * seq_len
    gx = torch.randn(T, 8 * H, device=dev, generator=g)
    w = torch.randn(2, 4 * H, H, device=dev, generator=g) * (1.5 / H ** 0.5)
    bhh = torch.randn(2, 4 * H, device=dev, generator=g) * 0.1
    dnews = torch.randn(nseq, H, device=dev, generator=g)
    # new
    wf, wb = K.birnn_pack_whh(w[0], w[1])
    gates = torch.empty(K.birnn_gates_numel(nseq, seq_len, H), device=dev)
    hprev = torch.empty(2, T, H, device=dev)
    hlast = torch.empty(2, nseq, H, device=dev)
    news = torch.empty(nseq, H, device=dev)
    dg = torch.empty(T, 8 * H, device=dev)

    def new_fwd():
        K.birnn_fwd(gx, wf, bhh, nseq, seq_len, H, gates, hprev, hlast, news)

    def new_bwd():
        K.birnn_bwd(wb, gates, nseq, seq_len, H, dg, dnews=dnews)

    # base: per direction, its own saved state and gradient buffers
    wt = [w[d].t().contiguous() for d in range(2)]
    wd = [w[d].contiguous() for d in range(2)]
    b_g = [torch.empty(T, 4 * H, device=dev) for _ in range(2)]
    b_h = [torch.empty(T, H, device=dev) for _ in range(2)]
    b_c = [torch.empty(T, H, device=dev) for _ in range(2)]
    b_o = [torch.empty(nseq, H, device=dev) for _ in range(2)]
    b_dg = [torch.empty(T, 4 * H, device=dev) for _ in range(2)]
    half = (0.5 * dnews).contiguous()

    def base_fwd():
        for d in range(2):
            K.rnn_fwd(L.CELL_LSTM, gx[:, d * 4 * H:(d + 1) * 4 * H], wt[d], bhh[d], nseq, seq_len, H, b_g[d], b_h[d],
                      b_c[d], b_o[d], reverse=bool(d))

    def base_bwd():
        for d in range(2):
            K.rnn_bwd(L.CELL_LSTM, wd[d], b_g[d], b_h[d], b_c[d], nseq, seq_len, H, half, b_dg[d], reverse=bool(d))

    def new():
        new_fwd()
        new_bwd()

    def base():
        base_fwd()
        base_bwd()

    for fn in (new, base):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    agree = {
        "news_maxdiff": float((news - 0.5 * (b_o[0] + b_o[1])).abs().max()),
        "dg_maxdiff": float((dg - torch.cat(b_dg, 1)).abs().max()),
    }
    fns = {"base": base, "new": new, "base2": base, "new_fwd": new_fwd, "new_bwd": new_bwd, "base_fwd": base_fwd,
           "base_bwd": base_bwd}
    reps = {k: max(3, int(50.0 / max(timed(fn, 2), 1e-3))) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"nseq": nseq, "L": seq_len, "H": H, "rounds": rounds}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out["noise_ms"] = round(abs(med["base"] - med["base2"]), 4)
    out["base_over_new"] = round(0.5 * (med["base"] + med["base2"]) / med["new"], 3)
    out.update(agree)
    return out


def train_step_ms(rounds, B=32, C=5, N=50, seq_len=30, vocab=30522):
    from newsrec_amd.manager import build_model, get_optim, train_step
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = build_model("rnn", "attn", 150, vocab=vocab).train()
    opt = get_optim(model, capturable=True)
    g = torch.Generator().manual_seed(1)

    def titles(n):
        tok = torch.randint(1, vocab, (n, seq_len), generator=g)
        lens = torch.randint(5, seq_len + 1, (n,), generator=g)
        mask = (torch.arange(seq_len)[None] < lens[:, None]).long()
        return tok * mask, mask
    ct, cm = titles(B * C)
    ht, hm = titles(B * N)
    x = {"cdd_encoded_index": ct.view(B, C, seq_len), "cdd_attn_mask": cm.view(B, C, seq_len),
         "his_encoded_index": ht.view(B, N, seq_len), "his_attn_mask": hm.view(B, N, seq_len),
         "his_mask": torch.ones(B, N, 1, dtype=torch.float64), "user_id": torch.randint(1, 40, (B,), generator=g),
         "label": torch.zeros(B, dtype=torch.long)}
    x = {k: v.to(dev) for k, v in x.items()}

    def step():
        train_step(model, opt, x, check_labels=False)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    eager = float(np.median([timed(step, 5) for _ in range(rounds)]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(model, opt, x, check_labels=False).detach()
    graph.replay()
    torch.cuda.synchronize()
    replay = float(np.median([timed(graph.replay, 10) for _ in range(rounds)]))
    return {"step_eager_ms": round(eager, 3), "step_graph_ms": round(replay, 3), "step_B": B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1760)
    ap.add_argument("--len", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    out = recurrence(a.nseq, a.len, a.hidden, a.rounds)
    if not a.no_step:
        out.update(train_step_ms(a.rounds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
