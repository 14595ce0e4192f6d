"""Times the dense-synthesizer attention core of the PLM synthesizer tower two ways on the same data, in the
same process, at the PLM train size nseq = 1,760 titles (B = 32 x (5 candidates + 50 history)), L = 30,
D = 768:

  (new)   nr_synth_attn_fwd + nr_synth_attn_bwd (csrc/synth_attn.hip)
  (base)  the same math written with torch-ROCm ops on the same GPU under autograd: addmm / relu / addmm /
          softmax / bmm, and autograd's backward of that chain down to hv (the weight gradients of the score
          MLP, which the fused path leaves to two small GEMMs, are computed by the baseline's autograd and
          by those two GEMMs in `new_wgrad`, reported separately and added to `new` in `new_total`)

Each variant is warmed up, then timed with device events over `--rounds` interleaved rounds
(base, new, base'), several calls each; medians are reported.  The noise floor is the spread between the two
timings of the baseline itself (base vs base').  Bytes/s are the compulsory traffic of the fused core
(forward: hv in, ctx, a1 and probs out; backward: hv, dctx, a1 and probs in, dhv, da1 and da2 out; W1 / W2
stay in L2) over the measured time.  Prints one JSON line.

python tools/synth_attn_probe.py [--nseq 1760] [--len 30] [--hidden 768] [--rounds 7]"""
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
from newsrec_amd.functions import _empty, _proj_wgrad


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def core(nseq, seq_len, D, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    T = nseq * seq_len
    hv = torch.randn(T, D, device=dev, generator=g)
    dctx = torch.randn(T, D, device=dev, generator=g)
    w1 = torch.randn(seq_len, D, device=dev, generator=g) * 1.2 / D ** 0.5
    b1 = 0.2 * torch.randn(seq_len, device=dev, generator=g)
    w2 = torch.randn(seq_len, seq_len, device=dev, generator=g) * 1.5 / seq_len ** 0.5
    b2 = 0.2 * torch.randn(seq_len, device=dev, generator=g)
    a1, da1, da2 = (_empty(T, seq_len, hv) for _ in range(3))
    probs = torch.empty(T * seq_len, device=dev)
    ctx = torch.empty(T, D, device=dev)
    dhv = torch.empty(T, D, device=dev)
    dw1, db1, dw2, db2 = torch.zeros_like(w1), torch.zeros_like(b1), torch.zeros_like(w2), torch.zeros_like(b2)

    def new_fwd():
        K.synth_attn_fwd(hv, w1, b1, w2, b2, nseq, seq_len, D, a1, probs, ctx)

    def new_bwd():
        K.synth_attn_bwd(hv, w1, w2, a1, probs, dctx, nseq, seq_len, D, da1, da2, dhv)

    def new():
        new_fwd()
        new_bwd()

    def new_wgrad():          # accumulates: the timing does not care
        _proj_wgrad(da2, K.operand(a1, L.MNCONTIG), dw2, db2, T)
        _proj_wgrad(da1, K.operand(hv, L.MNCONTIG), dw1, db1, T)

    def new_total():
        new()
        new_wgrad()

    leaf = hv.clone().requires_grad_()
    wl = [t.clone().requires_grad_() for t in (w1, b1, w2, b2)]
    dctx3 = dctx.view(nseq, seq_len, D)
    state = {}

    def base_fwd():
        h = torch.relu(torch.addmm(wl[1], leaf, wl[0].t()))
        pr = torch.softmax(torch.addmm(wl[3], h, wl[2].t()), -1).view(nseq, seq_len, seq_len)
        state["h"] = h
        state["ctx"] = torch.bmm(pr, leaf.view(nseq, seq_len, D))

    def base_bwd():
        leaf.grad = None
        for t in wl:
            t.grad = None
        state["ctx"].backward(dctx3)

    def base():               # autograd also sums the score MLP's weight gradients: compare with new_total
        base_fwd()
        base_bwd()

    def base_core():          # the weights as constants: the work of new (the two kernels) alone
        for t in wl:
            t.requires_grad_(False)
        base()
        for t in wl:
            t.requires_grad_(True)

    new_total()
    base()
    torch.cuda.synchronize()
    # a pre-activation within rounding of zero may gate differently in the two evaluations (about one in
    # 1e5 at N(0,1) scale): dhv is compared on the titles whose gates agree, and the weight-gradient sums,
    # which run over every title, only when all do
    flips = ((a1 > 0) != (state["h"] > 0)).view(nseq, -1).any(1)
    same = (~flips).repeat_interleave(seq_len)
    agree = {"gate_flips": int(flips.sum()),
             "ctx_maxdiff": float((ctx - state["ctx"].detach().reshape(T, D)).abs().max()),
             "dhv_maxdiff": float((dhv - leaf.grad)[same].abs().max()),
             "dw1_maxdiff": float((dw1 - wl[0].grad).abs().max()) if not flips.any() else None,
             "dw2_maxdiff": float((dw2 - wl[2].grad).abs().max()) if not flips.any() else None}
    for fn in (new_total, base, base_core):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()

    fns = {"base": base, "new": new, "base2": base, "new_fwd": new_fwd, "new_bwd": new_bwd, "new_wgrad": new_wgrad,
           "new_total": new_total, "base_fwd": base_fwd, "base_core": base_core}
    reps = {k: max(3, int(50.0 / max(timed(fn, 2), 1e-3))) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    fwd_bytes = 4 * (2 * T * D + 2 * T * seq_len)
    bwd_bytes = 4 * (3 * T * D + 4 * T * seq_len)
    out = {"nseq": nseq, "L": seq_len, "D": D, "rounds": rounds}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    base_ms = 0.5 * (med["base"] + med["base2"])
    out["noise_ms"] = round(abs(med["base"] - med["base2"]), 4)
    out["base_core_over_new"] = round(med["base_core"] / med["new"], 3)
    out["base_over_new_total"] = round(base_ms / med["new_total"], 3)
    out["core_MB"] = round((fwd_bytes + bwd_bytes) / 1e6, 1)
    out["new_GBps"] = round((fwd_bytes + bwd_bytes) / med["new"] / 1e6, 1)
    out["new_fwd_GBps"] = round(fwd_bytes / med["new_fwd"] / 1e6, 1)
    out["new_bwd_GBps"] = round(bwd_bytes / med["new_bwd"] / 1e6, 1)
    out.update(agree)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1760)
    ap.add_argument("--len", type=int, default=30)
    ap.add_argument("--hidden", type=int, nargs="+", default=[768])
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    for D in a.hidden:
        print(json.dumps(core(a.nseq, a.len, D, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
