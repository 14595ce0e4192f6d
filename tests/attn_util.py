"""Plain-torch references of the tied-QK attention core (nr_mha_attn_fwd / nr_mha_attn_bwd of
csrc/mha_attn.hip) and of the fused eval user encoder (nr_mha_user_pool_fwd of csrc/mha_pool.hip), and
the seeded inputs and masks of their tests.

The references take what the entries take, evaluate the operation under autograd in the dtype asked for
out of the primitives of oracle/restatement.py (xsoftmax, pairwise_mask, scaled_dp_attention) and return
what the kernels write.  tests/test_attn_ref_cpu.py holds them against oracle.restatement.
multihead_attention and mha_user."""
import math

import torch

from oracle import restatement as R
from pool_util import pool_mask


def _core(qk, v, m, heads, dk, dv):
    """qk [n*L, heads*dk], v [n*L, heads*dv], m [n, L] of 0/1 in their dtype -> O [n*L, heads*dv]."""
    n, L = m.shape
    kp = qk.reshape(n, L, heads, dk).permute(0, 2, 1, 3)
    vp = v.reshape(n, L, heads, dv).permute(0, 2, 1, 3)
    s = torch.matmul(kp, kp.transpose(-1, -2)) / math.sqrt(dk)
    p = R.xsoftmax(s, R.pairwise_mask(m))
    return torch.matmul(p, vp).permute(0, 2, 1, 3).reshape(n * L, heads * dv)


def mha_attn_reference(qk, v, mask, heads, dk, dv, dout=None, rows=None, dtype=torch.float64):
    """qk [T or R, heads*dk], v [T or R, heads*dv]; mask [n, L] (nonzero = a token, -0.0 is zero);
    rows (int64 [n*L], optional): token t reads qk / v row rows[t] -- gathered first, so the gradients
    stay per token.

    -> dict of detached ``dtype`` tensors
         out [n*L, heads*dv]   the heads of XSoftmax(Kp Kp^T / sqrt(dk), m_i m_j) Vp, concatenated
         scores_max            the largest score of a kept (i, j) pair (-inf without one)
       with dout [n*L, heads*dv], of (out * dout).sum():
         dqk [n*L, heads*dk], dv [n*L, heads*dv], dbias_k, dbias_v = their column sums"""
    n, L = mask.shape
    if rows is not None:
        qk, v = qk[rows], v[rows]
    assert qk.shape == (n * L, heads * dk) and v.shape == (n * L, heads * dv)
    qk = qk.detach().to(dtype).clone().requires_grad_()
    v = v.detach().to(dtype).clone().requires_grad_()
    m = (mask != 0).to(dtype)
    out = _core(qk, v, m, heads, dk, dv)
    with torch.no_grad():
        kp = qk.reshape(n, L, heads, dk).permute(0, 2, 1, 3)
        s = torch.matmul(kp, kp.transpose(-1, -2)) / math.sqrt(dk)
        kept = s[R.pairwise_mask(m).bool().expand_as(s)]
        smax = kept.max() if kept.numel() else torch.tensor(float("-inf"), dtype=dtype)
    res = {"out": out.detach(), "scores_max": smax}
    if dout is not None:
        dqk, dvv = torch.autograd.grad((out * dout.detach().to(dtype)).sum(), [qk, v])
        res.update(dqk=dqk, dv=dvv, dbias_k=dqk.sum(0), dbias_v=dvv.sum(0))
    return res


def mha_user_pool_reference(y, yrows, mask, heads, dk, dv, q, dtype=torch.float64):
    """y [R, >= heads*(dk+dv)] = [key projection | value projection] per news row; yrows int64 [n*L]
    (None: the identity); mask [n, L]; q [H = heads*dv].
    -> out [n, H] = sum_l XSoftmax(q . O_l / sqrt(H), mask)_l O_l over the core's O of y[yrows]."""
    n, L = mask.shape
    NK, H = heads * dk, heads * dv
    yy = (y if yrows is None else y[yrows]).detach().to(dtype)
    assert yy.shape[0] == n * L
    m = (mask != 0).to(dtype)
    O = _core(yy[:, :NK], yy[:, NK:NK + H], m, heads, dk, dv).reshape(n, L, H)
    qq = q.detach().to(dtype).reshape(1, 1, H).expand(n, 1, H)
    return R.scaled_dp_attention(qq, O, O, m.reshape(n, 1, L)).reshape(n, H).detach()


_KEPT = (2.0, -1.0, 0.5)


def attn_mask(L, dtype=torch.int64):
    """The tests' one batch of L-slot sequences: the eight rows of pool_mask(L) (prefixes, the empty
    sequence, holes at 1 and 3, the last slot alone), a row keeping every third slot (0, 3, 6, ...) and,
    for L > 32 -- where four waves own 16 keys each -- a row with slots 16..31 cleared and every other
    slot kept (a middle block masked) and a row keeping slots >= 32 only (the first two blocks masked).

    Float dtypes: kept slots hold 2.0, -1.0, 0.5 in turn, and the cleared slots with an even row + slot
    hold -0.0 (slot 0 of the empty row 0 always does).  int64: kept slots hold 1, 2^40, -1 in turn.  u8:
    255.  bool: True."""
    base = pool_mask(L)
    extra = [(torch.arange(L) % 3 == 0).long()]
    if L > 32:
        j = torch.arange(L)
        extra.append(((j < 16) | (j >= 32)).long())
        extra.append((j >= 32).long())
    keep = torch.cat([base, torch.stack(extra)], 0) != 0
    b, j = torch.meshgrid(torch.arange(keep.shape[0]), torch.arange(L), indexing="ij")
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


def attn_inputs(n, L, heads, dk, dv, seed, rows=None):
    """Seeded float32 inputs: qk 0.5 N(0,1) [rows or n*L, heads*dk], v N(0,1) [.., heads*dv], dout N(0,1)
    [n*L, heads*dv], q N(0,1) [heads*dv], dbias0 0.5 N(0,1) [heads*(dk+dv)] (what dbias starts from)."""
    g = torch.Generator().manual_seed(seed)
    R_ = rows or n * L
    return {
        "qk": torch.randn(R_, heads * dk, generator=g) * 0.5,
        "v": torch.randn(R_, heads * dv, generator=g),
        "dout": torch.randn(n * L, heads * dv, generator=g),
        "q": torch.randn(heads * dv, generator=g),
        "dbias0": torch.randn(heads * (dk + dv), generator=g) * 0.5,
    }
