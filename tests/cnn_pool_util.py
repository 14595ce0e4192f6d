"""Plain-torch reference of the CNN news encoder's fused word-attention head (nr_cnn_keypool_fwd /
nr_cnn_keypool_bwd of csrc/cnn_keypool.hip), and the seeded inputs and typed masks that the kernel-level
tests of that head and of nr_seq_pool_fwd / nr_seq_pool_bwd (csrc/seq_pool.hip) share.  The reference of
seq_pool is pool_util.attn_pool_reference without LayerNorm and dropout.

cnn_keypool_reference takes what the forward entry takes, evaluates the operation under autograd in the
dtype asked for out of oracle.restatement.xsoftmax and returns what the kernels write.
tests/test_cnn_pool_ref_cpu.py holds both against oracle.restatement.cnn_news / scaled_dp_attention."""
import math

import torch

from oracle import restatement as R
from pool_util import pool_mask


def cnn_keypool_reference(C, wq, bq, q, mask, dnews=None, dz=None, dtype=torch.float64):
    """C [n*L, H]: the conv output AFTER its ReLU (C >= 0); wq [H, H] (row j = output j), bq, q [H];
    mask [n, L] (nonzero = a token, -0.0 is zero).

    -> dict of detached ``dtype`` tensors
         K [n*L, H]      tanh(C wq^T + bq)
         probs [n, L]    XSoftmax(q . K_l / sqrt(H), mask)
         news [n, H]     sum_l probs_l C_l
       with dnews [n, H] (and dz [n*L, H], the gradient of the token output C), of
       (news * dnews).sum() + (C * dz).sum():
         dc [n*L, H]     the gradient of the conv PRE-activation: that of C where C > 0, else 0
         dwq [H, H], dbq [H], dq [H], dconv_b [H] = the column sums of dc"""
    n, L = mask.shape
    H = q.numel()
    assert C.shape == (n * L, H) and wq.shape == (H, H) and bq.numel() == H
    C, wq, bq, q = (t.detach().to(dtype).clone().requires_grad_() for t in (C, wq, bq, q))
    m = (mask != 0).to(dtype)
    K = torch.tanh(torch.matmul(C, wq.t()) + bq)
    probs = R.xsoftmax(torch.matmul(K.reshape(n, L, H), q) / math.sqrt(H), m)
    news = (probs.unsqueeze(-1) * C.reshape(n, L, H)).sum(1)
    out = {"K": K.detach(), "probs": probs.detach(), "news": news.detach()}
    if dnews is not None:
        loss = (news * dnews.detach().to(dtype)).sum()
        if dz is not None:
            loss = loss + (C * dz.detach().to(dtype)).sum()
        dC, dwq, dbq, dq = torch.autograd.grad(loss, [C, wq, bq, q])
        dc = dC * (C.detach() > 0).to(dtype)
        out.update(dc=dc, dwq=dwq, dbq=dbq, dq=dq, dconv_b=dc.sum(0))
    return out


def cnn_keypool_inputs(n, L, H, seed):
    """Seeded float32 inputs: C = ReLU(N(0,1)) [n*L, H] (about half of it exactly zero: the ReLU gate of
    dc), wq sqrt(2/H) N(0,1) [H, H], bq 0.1 N, q, dnews [n, H], dz [n*L, H] N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    return {
        "C": torch.relu(torch.randn(n * L, H, generator=g)),
        "wq": torch.randn(H, H, generator=g) * (2.0 / H) ** 0.5,
        "bq": torch.randn(H, generator=g) * 0.1,
        "q": torch.randn(H, generator=g),
        "dnews": torch.randn(n, H, generator=g),
        "dz": torch.randn(n * L, H, generator=g),
    }


def seq_pool_dq_per_seq(x, key, q, probs, dout, scale):
    """The share of each sequence in nr_seq_pool_bwd's dq, [n, D] in float64: sum_l ds_l K_l with
    ds = p (dp - sum p dp) scale, dp_l = dout . X_l (K = X when key is None).  The kernels add these
    shares onto dq's start one workgroup at a time; the tests bound the rounding of those additions with
    them."""
    n, L = probs.shape
    D = x.shape[-1]
    X = x.double().reshape(n, L, D)
    Kk = X if key is None else key.double().reshape(n, L, D)
    p = probs.double()
    dp = (X * dout.double()[:, None, :]).sum(-1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    return torch.einsum("nl,nld->nd", ds, Kk)


_KEPT = (2.0, -1.0, 0.5)


def typed_mask(L, n, dtype, start=0):
    """n sequences of L slots: row i is row (start + i) % 8 of pool_mask(L) (the empty sequence, length 1,
    full, L - 1, L / 2, holes, length 2, only the last slot), stored as attn_util.attn_mask stores its
    batch: float dtypes hold 2.0, -1.0, 0.5 in turn in the kept slots and -0.0 in the cleared slots with
    an even row + slot; int64 holds 1, 2^40, -1 in turn; uint8 255; bool True."""
    base = pool_mask(L) != 0
    keep = base[(start + torch.arange(n)) % base.shape[0]]
    b, j = torch.meshgrid(torch.arange(n), torch.arange(L), indexing="ij")
    if dtype == torch.bool:
        return keep
    if dtype == torch.uint8:
        return keep.to(torch.uint8) * 255
    if dtype == torch.int64:
        vals = torch.tensor([1, 1 << 40, -1])[(b + j) % 3]
        return torch.where(keep, vals, torch.zeros_like(vals))
    assert dtype in (torch.float32, torch.float64)
    vals = torch.tensor(_KEPT, dtype=dtype)[(b + j) % 3]
    zero = torch.where((b + j) % 2 == 0, torch.tensor(-0.0, dtype=dtype), torch.tensor(0.0, dtype=dtype))
    return torch.where(keep, vals, zero)
