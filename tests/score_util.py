"""Closed-form float64 references of the entry points of csrc/score_adam.hip that the kernel-level
tests compare with (tests/test_score_kernels_gpu.py), and the scorer's derived error bound.

  score_reference         nr_score_fwd / nr_score_bwd: the scaled dot products, the three heads and
                          their backward written out (no autograd)
  score_tolerance         the fp32 dot-product bound per (b, c), topk_util.dot_tolerance
  nll_reference           nr_score_nll_fwd / nr_score_nll_bwd: mean NLL (ignore_index -100) over
                          score_reference's log-softmax, and its gradient
  xsoftmax_bwd_reference  nr_xsoftmax_bwd (the forward is oracle.restatement.xsoftmax)
  adam_reference          nr_adam: one torch.optim.Adam step per element

Being closed form, tests/test_score_ref_cpu.py can hold them against autograd of
oracle/restatement.py's expressions and against torch.optim.Adam."""
import math

import numpy as np
import torch

from newsrec_amd import _lib as L
from topk_util import dot_tolerance, scale32

F64 = torch.float64
IGNORE_INDEX = -100


def _rows(cdd, B, C, idx):
    """[B, C, H] float64: row b*C+c of cdd, or row idx[b*C+c] when idx is given."""
    x = cdd.detach().to(F64)
    if idx is not None:
        x = x[idx.reshape(-1).long()]
    else:
        x = x[:B * C]
    return x.reshape(B, C, -1)


def score_reference(cdd, user, B, C, mode, idx=None, dlogits=None):
    """cdd [rows, H], user [B, H]; mode L.SCORE_RAW | L.SCORE_LOG_SOFTMAX | L.SCORE_SIGMOID; idx
    int64 [B*C] row ids into cdd or None (row b*C+c).

    -> dict of float64 tensors
         s [B, C]       (row(b, c) . user_b) * float64(float32(1 / sqrt(H))): the kernels' fp32 scale
         out [B, C]     s, s - logsumexp_c(s), or 1 / (1 + exp(-s))
       with dlogits [B, C] (the gradient of out) also
         dcdd [B*C, H]  the gradient of the rows (b, c) as scored (of the gathered rows under idx)
         duser [B, H]"""
    x = _rows(cdd, B, C, idx)
    u = user.detach().to(F64)[:B]
    H = x.shape[-1]
    scale = float(scale32(H))
    s = (x * u[:, None, :]).sum(-1) * scale
    if mode == L.SCORE_RAW:
        out = s
    elif mode == L.SCORE_LOG_SOFTMAX:
        mx = s.max(1, keepdim=True).values
        out = s - (mx + torch.log(torch.exp(s - mx).sum(1, keepdim=True)))
    elif mode == L.SCORE_SIGMOID:
        out = 1.0 / (1.0 + torch.exp(-s))
    else:
        raise ValueError(mode)
    res = {"s": s, "out": out}
    if dlogits is not None:
        dl = dlogits.detach().to(F64).reshape(B, C)
        if mode == L.SCORE_RAW:
            ds = dl
        elif mode == L.SCORE_LOG_SOFTMAX:
            ds = dl - torch.exp(out) * dl.sum(1, keepdim=True)
        else:
            ds = dl * out * (1.0 - out)
        ds = ds * scale
        res["dcdd"] = (ds[:, :, None] * u[:, None, :]).reshape(B * C, H)
        res["duser"] = (ds[:, :, None] * x).sum(1)
    return res


def score_tolerance(cdd, user, B, C, idx=None):
    """[B, C] float64 bound on |fp32 raw score - score_reference's s| (topk_util.dot_tolerance per (b, c))."""
    x = _rows(cdd, B, C, idx).numpy()
    u = user.detach().to(F64)[:B].numpy()
    H = x.shape[-1]
    absdot = (np.abs(x) * np.abs(u)[:, None, :]).sum(-1)
    dot = (x * u[:, None, :]).sum(-1)
    return torch.from_numpy(dot_tolerance(absdot, dot, H))


def nll_reference(cdd, user, label, B, C, dloss=1.0):
    """torch.nn.NLLLoss() (mean, ignore_index -100) over score_reference's log-softmax; label int64 [B],
    each in [0, C) or -100.

    -> dict: logits [B, C], loss (0-d; NaN when every label is ignored: 0 / 0), and the gradient of
       dloss * loss: dcdd [B*C, H], duser [B, H]"""
    label = label.reshape(B).long()
    keep = label != IGNORE_INDEX
    assert bool(((label[keep] >= 0) & (label[keep] < C)).all())
    logits = score_reference(cdd, user, B, C, L.SCORE_LOG_SOFTMAX)["out"]
    n = float(keep.sum())
    picked = logits[keep, label[keep]]
    loss = -picked.sum() / n if n else torch.tensor(float("nan"), dtype=F64)
    dl = torch.zeros(B, C, dtype=F64)
    if n:
        dl[keep, label[keep]] = -float(dloss) / n
    back = score_reference(cdd, user, B, C, L.SCORE_LOG_SOFTMAX, dlogits=dl)
    return {"logits": logits, "loss": loss, "dcdd": back["dcdd"], "duser": back["duser"]}


def xsoftmax_bwd_reference(y, dy):
    """_softmax_backward_data over the last dimension: y (dy - sum dy y), in float64."""
    y, dy = y.detach().to(F64), dy.detach().to(F64)
    return y * (dy - (dy * y).sum(-1, keepdim=True))


def f32(x):
    """A Python float holding x rounded to fp32: the value a kernel receives for a float argument."""
    return float(np.float32(x))


def adam_reference(p, g, m, v, lr, b1, b2, eps, wd, gscale, step):
    """One torch.optim.Adam step (amsgrad=False, maximize=False) per element in float64 on
    gradient g * gscale.  The hyper-parameters are taken as given: pass the fp32-rounded values (f32())
    the kernel receives, so that both compute the same function (1 - beta is then exact in fp32 too).
    The bias corrections are formed in double from them, as the kernel and torch form them.

    -> (p, m, v) float64"""
    p, g, m, v = (t.detach().to(F64) for t in (p, g, m, v))
    g = g * gscale
    if wd != 0:
        g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    den = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / den)
    return p, m, v
