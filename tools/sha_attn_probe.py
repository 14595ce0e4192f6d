"""Times the one-head attention core of the transformer news encoder two ways on the same data, in the
same process, at the train size nseq = 1,760 titles (B = 32 x (5 candidates + 50 history)), L = 30, for
H = 384 and H = 152:

  (new)   nr_sha_attn_fwd + nr_sha_attn_bwd (csrc/sha_attn.hip), dropout 0.1 on the probabilities
  (base)  the same core written with torch-ROCm ops on the same GPU under autograd: baddbmm for the
          scaled scores, masked_fill(-inf) / softmax / masked_fill(0) for XSoftmax, dropout, bmm, and
          autograd's backward of that chain (q, k, v as column views of one [T, 3H] buffer, as the
          kernels take them)

Each variant is warmed up, then timed with device events over `--rounds` interleaved rounds
(base, new, base'), several calls each; medians are reported.  The noise floor is the spread between
the two timings of the baseline itself (base vs base').  Bytes/s are the compulsory traffic of the core
(forward: qkv in, ctx and probs out; backward: qkv, dctx and probs in, dqkv out) over the measured time,
for both variants alike.  Also times one transformer + attn train step at B = 32 (eager and as a graph
replay) unless --no-step.  Prints one JSON line per width.

python tools/sha_attn_probe.py [--nseq 1760] [--len 30] [--hidden 384 152] [--rounds 7] [--no-step]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "news-recommendation-mind_amd"))

import numpy as np
import torch

from newsrec_amd import kernels as K

P_DROP = 0.1


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def core(nseq, seq_len, H, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    T = nseq * seq_len
    scale = 1.0 / H ** 0.5
    qkv = torch.randn(T, 3 * H, device=dev, generator=g)
    dctx = torch.randn(T, H, device=dev, generator=g)
    lens = torch.randint(5, seq_len + 1, (nseq,), device=dev, generator=g)
    mask = (torch.arange(seq_len, device=dev)[None] < lens[:, None]).long().contiguous()
    ctx = torch.empty(T, H, device=dev)
    probs = torch.empty(T * seq_len, device=dev)
    dqkv = torch.empty(T, 3 * H, device=dev)

    def new_fwd(p=P_DROP):
        K.sha_attn_fwd(qkv, mask.view(-1), nseq, seq_len, H, ctx, probs, p_drop=p, seed=1, offset=2)

    def new_bwd(p=P_DROP):
        K.sha_attn_bwd(qkv, mask.view(-1), nseq, seq_len, H, probs, dctx, dqkv, p_drop=p, seed=1, offset=2)

    def new():
        new_fwd()
        new_bwd()

    leaf = qkv.clone().requires_grad_()
    rmask = (mask == 0)[:, None, :]
    zero = torch.zeros(nseq, seq_len, seq_len, device=dev)
    dctx3 = dctx.view(nseq, seq_len, H)
    state = {}

    def base_fwd(p=P_DROP):
        x = leaf.view(nseq, seq_len, 3 * H)
        q, k, v = x[..., :H], x[..., H:2 * H], x[..., 2 * H:]
        s = torch.baddbmm(zero, q, k.transpose(1, 2), beta=0.0, alpha=scale).masked_fill(rmask, float("-inf"))
        pr = torch.softmax(s, -1).masked_fill(rmask, 0.0)
        state["probs"] = pr
        state["ctx"] = torch.bmm(torch.nn.functional.dropout(pr, p, True), v)

    def base_bwd():
        leaf.grad = None
        state["ctx"].backward(dctx3)

    def base():
        base_fwd()
        base_bwd()

    # agreement without dropout (torch draws another mask)
    new_fwd(0.0)
    new_bwd(0.0)
    base_fwd(0.0)
    base_bwd()
    torch.cuda.synchronize()
    agree = {"ctx_maxdiff": float((ctx - state["ctx"].detach().reshape(T, H)).abs().max()),
             "dqkv_maxdiff": float((dqkv - leaf.grad).abs().max())}
    for fn in (new, base):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()

    def base_both():          # a backward needs its own forward's graph: timed as the pair, and forward alone
        base()

    fns = {"base": base_both, "new": new, "base2": base_both, "new_fwd": new_fwd, "new_bwd": new_bwd,
           "base_fwd": base_fwd}
    reps = {k: max(3, int(50.0 / max(timed(fn, 2), 1e-3))) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    fwd_bytes = 4 * (T * 3 * H + T * H + T * seq_len)
    bwd_bytes = 4 * (T * 3 * H + T * H + T * seq_len + T * 3 * H)
    out = {"nseq": nseq, "L": seq_len, "H": H, "rounds": rounds}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    base_ms = 0.5 * (med["base"] + med["base2"])
    out["noise_ms"] = round(abs(med["base"] - med["base2"]), 4)
    out["base_over_new"] = round(base_ms / med["new"], 3)
    out["core_MB"] = round((fwd_bytes + bwd_bytes) / 1e6, 1)
    out["new_GBps"] = round((fwd_bytes + bwd_bytes) / med["new"] / 1e6, 1)
    out["base_GBps"] = round((fwd_bytes + bwd_bytes) / base_ms / 1e6, 1)
    out["new_fwd_GBps"] = round(fwd_bytes / med["new_fwd"] / 1e6, 1)
    out["new_bwd_GBps"] = round(bwd_bytes / med["new_bwd"] / 1e6, 1)
    out.update(agree)
    return out


def train_step_ms(rounds, H, B=32, C=5, N=50, seq_len=30, vocab=30522):
    from newsrec_amd.manager import build_model, get_optim, train_step
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = build_model("transformer", "attn", H, vocab=vocab).train()
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
    return {"step_eager_ms": round(eager, 3), "step_graph_ms": round(replay, 3), "step_B": B, "step_H": H}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1760)
    ap.add_argument("--len", type=int, default=30)
    ap.add_argument("--hidden", type=int, nargs="+", default=[384, 152])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    for H in a.hidden:
        out = core(a.nseq, a.len, H, a.rounds)
        if not a.no_step:
            out.update(train_step_ms(a.rounds, H))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
