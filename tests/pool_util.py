"""Plain-torch references of the two pooling ABIs (nr_mha_pool_fwd / nr_mha_pool_bwd of
csrc/mha_pool.hip, nr_attn_pool_fwd / nr_attn_pool_bwd of csrc/attn_pool.hip) and the seeded inputs
and masks of their tests.

Both references take what the forward entry takes, evaluate the operation under autograd in the dtype
asked for out of the primitives of oracle/restatement.py (xsoftmax, pairwise_mask) and return what the
kernels save and write, and, given the upstream gradients, what the backward entry writes.  The dropout
keep mask comes from oracle.restatement.dropout_keep, which restates the device RNG bit for bit.
tests/test_pool_ref_cpu.py holds them against oracle.restatement.mha_news / scaled_dp_attention."""
import math

import torch

from oracle import restatement as R


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_()


def _dropout(z, keep, p_drop):
    if keep is None:
        assert p_drop == 0
        return z
    return z * keep.reshape(z.shape).to(z.dtype) / (1.0 - p_drop)


def _layer_norm(x, gamma, beta, eps):
    """-> (LN(x), mean [rows, 1], rstd [rows, 1]); biased variance, rstd = (var + eps)^-1/2."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    return (x - mean) * rstd * gamma + beta, mean, rstd


def mha_pool_reference(y, mask, heads, dk, dv, gamma, beta, q, keep, p_drop, dnews=None, dz=None, eps=1e-5,
                       dtype=torch.float64):
    """y [n*L, heads*(dk+dv)] = [key projection | value projection] (head h: key columns h*dk ..,
    value columns heads*dk + h*dv ..); mask [n, L] (nonzero = a token); gamma, beta, q [H = heads*dv];
    keep bool [n*L, H] (None: no dropout, p_drop = 0).

    -> dict of detached ``dtype`` tensors
         O [n*L, H]      the heads of XSoftmax(Kp Kp^T / sqrt(dk), m_i m_j) Vp, concatenated
         Z [n*L, H]      Dropout(LayerNorm(O))
         news [n, H]     sum_l probs_l Z_l
         probs [n, L]    XSoftmax(q . Z_l / sqrt(H), mask)
         stats [n*L, 2]  LayerNorm mean, rstd
       with dnews [n, H] (and dz [n*L, H], the gradient of Z), of (news * dnews).sum() + (Z * dz).sum():
         dy [n*L, heads*(dk+dv)], dbias = its column sums, dq, dgamma, dbeta [H]"""
    n, L = mask.shape
    H, NK = heads * dv, heads * dk
    assert y.shape == (n * L, NK + H)
    y, gamma, beta, q = (_leaf(t, dtype) for t in (y, gamma, beta, q))
    m = (mask != 0).to(dtype)
    kp = y[:, :NK].reshape(n, L, heads, dk).permute(0, 2, 1, 3)
    vp = y[:, NK:].reshape(n, L, heads, dv).permute(0, 2, 1, 3)
    s = torch.matmul(kp, kp.transpose(-1, -2)) / math.sqrt(dk)
    p = R.xsoftmax(s, R.pairwise_mask(m))
    O = torch.matmul(p, vp).permute(0, 2, 1, 3).reshape(n * L, H)
    ln, mean, rstd = _layer_norm(O, gamma, beta, eps)
    Z = _dropout(ln, keep, p_drop)
    Zs = Z.reshape(n, L, H)
    probs = R.xsoftmax(torch.matmul(Zs, q) / math.sqrt(H), m)
    news = (probs.unsqueeze(-1) * Zs).sum(1)
    out = {"O": O.detach(), "Z": Z.detach(), "news": news.detach(), "probs": probs.detach(),
           "stats": torch.cat([mean, rstd], 1).detach()}
    if dnews is not None:
        loss = (news * dnews.detach().to(dtype)).sum()
        if dz is not None:
            loss = loss + (Z * dz.detach().to(dtype)).sum()
        dy, dq, dgamma, dbeta = torch.autograd.grad(loss, [y, q, gamma, beta])
        out.update(dy=dy, dbias=dy.sum(0), dq=dq, dgamma=dgamma, dbeta=dbeta)
    return out


def attn_pool_reference(x, key, q, mask, gamma, beta, keep, p_drop, scale, key_tanh, dout=None, dz=None, eps=1e-5,
                        dtype=torch.float64):
    """x [n*L, D]; key [n*L, D] as stored (already tanh-ed when key_tanh) or None (K = Z); q [D];
    mask [n, L]; gamma, beta [D] or None (no LayerNorm); keep bool [n*L, D] or None (p_drop = 0).

    -> dict of detached ``dtype`` tensors
         Z [n*L, D]      Dropout(LayerNorm(x))
         probs [n, L]    XSoftmax(scale * q . K_l, mask)
         out [n, D]      sum_l probs_l Z_l
         stats [n*L, 2]  LayerNorm mean, rstd (None without LayerNorm)
       with dout [n, D] (and dz [n*L, D]), of (out * dout).sum() + (Z * dz).sum():
         dx [n*L, D], dq [D], dgamma, dbeta [D] (LayerNorm only),
         dk [n*L, D] (separate key only): the gradient of ``key``, times 1 - key^2 when key_tanh"""
    n, L = mask.shape
    D = q.numel()
    assert x.shape == (n * L, D)
    x, q = _leaf(x, dtype), _leaf(q, dtype)
    m = (mask != 0).to(dtype)
    stats = None
    if gamma is not None:
        gamma, beta = _leaf(gamma, dtype), _leaf(beta, dtype)
        ln, mean, rstd = _layer_norm(x, gamma, beta, eps)
        stats = torch.cat([mean, rstd], 1).detach()
    else:
        ln = x
    Z = _dropout(ln, keep, p_drop)
    if key is not None:
        key = _leaf(key, dtype)
    K = key if key is not None else Z
    probs = R.xsoftmax(scale * torch.matmul(K.reshape(n, L, D), q), m)
    res = (probs.unsqueeze(-1) * Z.reshape(n, L, D)).sum(1)
    out = {"Z": Z.detach(), "probs": probs.detach(), "out": res.detach(), "stats": stats}
    if dout is not None:
        loss = (res * dout.detach().to(dtype)).sum()
        if dz is not None:
            loss = loss + (Z * dz.detach().to(dtype)).sum()
        leaves = {"dx": x, "dq": q}
        if gamma is not None:
            leaves.update(dgamma=gamma, dbeta=beta)
        if key is not None:
            leaves["dk"] = key
        grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
        if key is not None and key_tanh:
            grads["dk"] = grads["dk"] * (1 - key.detach() ** 2)
        out.update(grads)
    return out


def pool_mask(L, dtype=torch.int64):
    """The tests' one batch of 8 sequences of L slots: prefix lengths 0, 1, L, L-1, L/2, L, 2 (clamped
    to 1..L but for the first), sequence 5 with holes at positions 1 and 3 when L > 4, and a last
    sequence whose only token is the last slot."""
    lens = [0] + [min(max(v, 1), L) for v in (1, L, L - 1, L // 2, L, 2)]
    m = torch.zeros(len(lens) + 1, L, dtype=dtype)
    for b, v in enumerate(lens):
        m[b, :v] = 1
    if L > 4:
        m[5, 1] = 0
        m[5, 3] = 0
    m[-1, L - 1] = 1
    return m


def mha_pool_inputs(n, L, heads, dk, dv, seed, rows=None):
    """Seeded float32 inputs: y 0.5 N(0,1) ([rows or n*L, heads*(dk+dv)]), gamma 1 + 0.1 N, beta 0.1 N,
    q, dnews, dz N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    H = heads * dv
    return {
        "y": torch.randn(rows or n * L, heads * (dk + dv), generator=g) * 0.5,
        "gamma": 1 + 0.1 * torch.randn(H, generator=g),
        "beta": 0.1 * torch.randn(H, generator=g),
        "q": torch.randn(H, generator=g),
        "dnews": torch.randn(n, H, generator=g),
        "dz": torch.randn(n * L, H, generator=g),
    }


def attn_pool_inputs(n, L, D, seed):
    """Seeded float32 inputs: x 0.7 N(0,1), key tanh(N(0,1)), gamma 1 + 0.1 N, beta 0.1 N, q, dout,
    dz N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    return {
        "x": torch.randn(n * L, D, generator=g) * 0.7,
        "key": torch.tanh(torch.randn(n * L, D, generator=g)),
        "gamma": 1 + 0.1 * torch.randn(D, generator=g),
        "beta": 0.1 * torch.randn(D, generator=g),
        "q": torch.randn(D, generator=g),
        "dout": torch.randn(n, D, generator=g),
        "dz": torch.randn(n * L, D, generator=g),
    }
