"""Times the disentangled attention core of the PLM DeBERTa tower against two yardsticks on the same GPU, in the
same process, at the PLM train size nseq = 1,760 titles (B = 32 x (5 candidates + 50 history)), 12 heads,
L = 30:

  (new)   nr_deb_attn_fwd + nr_deb_attn_bwd (csrc/deberta_attn.hip), p = 0.1, DeBERTa's interleaved layout
  (base)  the same math written with torch-ROCm ops under autograd: three batched products, two gathers, the
          masked softmax, dropout, P V, and autograd's backward down to q, k, v, pk, pq
  (bert)  nr_bert_attn_fwd + nr_bert_attn_bwd at the same shape and dropout rate, in the exact-f32 arithmetic
          and in the thread's default GEMM arithmetic: BERT's core does one third of the score products

Each variant is warmed up, then timed with device events over `--rounds` interleaved rounds, several calls each;
medians are reported.  The noise floor is the spread between the two timings of the baseline itself (base vs
base2).  Prints one JSON line.

python tools/deberta_probe.py [--nseq 1760] [--len 30] [--heads 12] [--rounds 7]"""
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


def core(nseq, seq_len, heads, rounds, p):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    T, H = nseq * seq_len, 64 * heads
    scale = 1.0 / (3 * 64) ** 0.5
    qkv = torch.randn(T, 3 * H, device=dev, generator=g)
    pk = torch.randn(2 * seq_len, H, device=dev, generator=g)
    pq = torch.randn(2 * seq_len, H, device=dev, generator=g)
    dctx = torch.randn(T, H, device=dev, generator=g)
    lens = torch.randint(5, seq_len + 1, (nseq,), device=dev, generator=g)
    mask = (torch.arange(seq_len, device=dev)[None] < lens[:, None]).long().contiguous()
    probs = torch.empty(nseq * heads * seq_len * seq_len, device=dev)
    ctx = torch.empty(T, H, device=dev)
    dqkv = torch.empty(T, 3 * H, device=dev)
    dpk, dpq = torch.empty_like(pk), torch.empty_like(pq)
    work = torch.empty(K.deb_attn_bwd_workspace(nseq, seq_len, heads) // 4, device=dev)
    drop = dict(p_drop=p, seed=1, offset=0)

    def new_fwd():
        K.deb_attn_fwd(qkv, pk, pq, mask, nseq, seq_len, heads, probs, ctx, scale=scale, **drop)

    def new_bwd():
        K.deb_attn_bwd(qkv, pk, pq, mask, nseq, seq_len, heads, probs, dctx, dqkv, dpk, dpq, scale=scale, work=work,
                       **drop)

    def new():
        new_fwd()
        new_bwd()

    # BERT's core on a blocked projection of the same size
    ml = torch.empty(T * heads * 2, device=dev)
    bctx, bdqkv = torch.empty(T, H, device=dev), torch.empty(T, 3 * H, device=dev)

    def bert(prec):
        def fn():
            K.bert_attn_fwd(qkv, heads, mask, nseq, seq_len, bctx, ml, prec=prec, **drop)
            K.bert_attn_bwd(qkv, heads, mask, nseq, seq_len, bctx, ml, dctx, bdqkv, prec=prec, **drop)
        return fn

    # the torch composition under autograd (its own dropout mask: the timing does not care)
    v4 = qkv.view(nseq, seq_len, heads, 3, 64).permute(3, 0, 2, 1, 4)
    leaves = [t.contiguous().requires_grad_() for t in (v4[0], v4[1], v4[2])]
    pl = [t.view(2 * seq_len, heads, 64).permute(1, 0, 2).contiguous().requires_grad_() for t in (pk, pq)]
    r = torch.arange(seq_len, device=dev)
    idx = (r[:, None] - r[None, :] + seq_len).expand(nseq, heads, seq_len, seq_len)
    idx_t = idx.transpose(-1, -2).contiguous()
    both = ((mask != 0)[:, None, :, None] & (mask != 0)[:, None, None, :])
    dc4 = dctx.view(nseq, seq_len, heads, 64).permute(0, 2, 1, 3)
    state = {}

    def base_fwd():
        q, k, v = leaves
        c2p = torch.gather(torch.matmul(q, pl[0].transpose(-1, -2)), -1, idx)
        p2c = torch.gather(torch.matmul(k, pl[1].transpose(-1, -2)), -1, idx_t).transpose(-1, -2)
        s = (torch.matmul(q, k.transpose(-1, -2)) + c2p + p2c) * scale
        pr = torch.softmax(s.masked_fill(~both, torch.finfo(torch.float32).min), -1)
        state["probs"] = pr
        state["ctx"] = torch.matmul(torch.nn.functional.dropout(pr, p, True), v)

    def base_bwd():
        for t in leaves + pl:
            t.grad = None
        state["ctx"].backward(dc4)

    def base():
        base_fwd()
        base_bwd()

    new()
    base()
    torch.cuda.synchronize()
    agree = {"probs_maxdiff": float((probs.view(nseq, heads, seq_len, seq_len) - state["probs"].detach()).abs().max())}
    fns = {"base": base, "new": new, "base2": base, "new_fwd": new_fwd, "new_bwd": new_bwd, "base_fwd": base_fwd,
           "bert_f32": bert(L.GEMM_F32), "bert_default": bert(None)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {k: max(3, int(50.0 / max(timed(fn, 2), 1e-3))) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    units = nseq * heads * seq_len * seq_len * 64 * 2           # flop of one L x L x 64 product over every head
    out = {"nseq": nseq, "L": seq_len, "heads": heads, "p_drop": p, "rounds": rounds}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    base_ms = 0.5 * (med["base"] + med["base2"])
    out["noise_ms"] = round(abs(med["base"] - med["base2"]), 4)
    out["base_over_new"] = round(base_ms / med["new"], 3)
    out["new_over_bert_f32"] = round(med["new"] / med["bert_f32"], 3)
    out["new_over_bert_default"] = round(med["new"] / med["bert_default"], 3)
    # useful products: forward 4 (three score terms + P V), backward 8 (dPd, dV, 2 dQ, 2 dK, dpk, dpq)
    out["new_fwd_TFLOPs"] = round(4 * units / med["new_fwd"] / 1e9, 2)
    out["new_bwd_TFLOPs"] = round(8 * units / med["new_bwd"] / 1e9, 2)
    out.update(agree)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1760)
    ap.add_argument("--len", type=int, default=30)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--p", type=float, default=0.1)
    a = ap.parse_args()
    print(json.dumps(core(a.nseq, a.len, a.heads, a.rounds, a.p)), flush=True)


if __name__ == "__main__":
    main()
