"""Plain-torch references of the BERT tower's kernels between the GEMMs (csrc/bert.hip:
nr_bert_embed_fwd / _bwd, nr_bert_add_ln_fwd / _bwd, nr_bert_attn_fwd / _bwd, as include/newsrec_hip.h
states them) and the seeded inputs and masks of their tests.

Each reference takes what the forward entry takes, evaluates the operation under autograd in the dtype
asked for and returns detached tensors of what the entries save and write, and, given the upstream
gradient, what the backward entries (and, for the embeddings, the table-gradient chain behind them)
write.  The dropout keep masks come from oracle.restatement.BertDropout (bert_dropout below), which
restates the device RNG bit for bit.  tests/test_bert_ref_cpu.py holds the references against
independent formulations."""
import torch

from oracle import restatement as R

NEG = torch.finfo(torch.float32).min


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_()


def _dropout(z, keep, p_drop):
    if keep is None:
        assert p_drop == 0
        return z
    return z * keep.reshape(z.shape).to(z.dtype) / (1.0 - p_drop)


def _layer_norm(s, gamma, beta, eps):
    """-> (LN(s), mean [rows, 1], rstd [rows, 1]); biased variance, rstd = (var + eps)^-1/2."""
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    return (s - mean) * rstd * gamma + beta, mean, rstd


def embed_forward(word, pos, type0, ids, gamma, beta, eps, keep, p_drop):
    """The differentiable formula of embed_reference in the dtype of its arguments -> (out, mean, rstd, s)."""
    nseq, L = ids.shape
    s = (word[ids] + pos[:L] + type0).reshape(nseq * L, word.shape[1])
    ln, mean, rstd = _layer_norm(s, gamma, beta, eps)
    return _dropout(ln, keep, p_drop), mean, rstd, s


def add_ln_forward(x, res, gamma, beta, eps, keep, p_drop):
    """The differentiable formula of add_ln_reference -> (out, mean, rstd)."""
    return _layer_norm(_dropout(x, keep, p_drop) + res, gamma, beta, eps)


def attn_forward(q, k, v, mask, heads, keep, p_drop):
    """The differentiable formula of attn_reference -> (ctx [T, heads*64], row max and row sum [nseq,
    heads, L, 1])."""
    nseq, L = mask.shape
    T, H = nseq * L, heads * 64
    assert q.shape == (T, H)
    qh, kh, vh = (t.reshape(nseq, L, heads, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    add = (1.0 - (mask != 0).to(q.dtype)) * NEG
    s = torch.matmul(qh, kh.transpose(-1, -2)) / 8.0 + add[:, None, None, :]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = _dropout(e / l, keep, p_drop)
    return torch.matmul(p, vh).permute(0, 2, 1, 3).reshape(T, H), m, l


def embed_reference(word, pos, type0, ids, gamma, beta, eps, keep, p_drop, dout=None, padding_idx=0,
                    dtype=torch.float64):
    """word [V, H], pos [P >= L, H], type0 [H], ids int64 [nseq, L] (all inside [0, V)), gamma, beta [H],
    keep bool [nseq*L, H] or None (p_drop = 0).

    -> dict of detached ``dtype`` tensors
         out [T, H]     Dropout(LayerNorm(s)),  s[t] = word[ids[t]] + pos[t % L] + type0
         stats [T, 2]   LayerNorm mean, rstd
       with dout [T, H], of (out * dout).sum():
         ds [T, H]      the gradient of s (what nr_bert_embed_bwd stores)
         dword [V, H]   with row ``padding_idx`` zero (nn.Embedding(padding_idx=0)), dpos [P, H], dtype0 [H]
         dgamma, dbeta [H]"""
    word, pos, type0, gamma, beta = (_leaf(t, dtype) for t in (word, pos, type0, gamma, beta))
    y, mean, rstd, s = embed_forward(word, pos, type0, ids, gamma, beta, eps, keep, p_drop)
    out = {"out": y.detach(), "stats": torch.cat([mean, rstd], 1).detach()}
    if dout is not None:
        ds, dword, dpos, dtype0, dgamma, dbeta = torch.autograd.grad(
            (y * dout.detach().to(dtype)).sum(), [s, word, pos, type0, gamma, beta])
        dword = dword.clone()
        if padding_idx is not None:
            dword[padding_idx] = 0
        out.update(ds=ds, dword=dword, dpos=dpos, dtype0=dtype0, dgamma=dgamma, dbeta=dbeta)
    return out


def add_ln_reference(x, res, gamma, beta, eps, keep, p_drop, dout=None, dtype=torch.float64):
    """x, res [T, H]; keep bool [T, H] or None (p_drop = 0).

    -> dict of detached ``dtype`` tensors: out = LayerNorm(x * keep / (1 - p) + res) [T, H], stats [T, 2]
       (mean, rstd); with dout [T, H], of (out * dout).sum(): dres, dx [T, H], dgamma, dbeta [H]"""
    x, res, gamma, beta = (_leaf(t, dtype) for t in (x, res, gamma, beta))
    y, mean, rstd = add_ln_forward(x, res, gamma, beta, eps, keep, p_drop)
    out = {"out": y.detach(), "stats": torch.cat([mean, rstd], 1).detach()}
    if dout is not None:
        grads = torch.autograd.grad((y * dout.detach().to(dtype)).sum(), [res, x, gamma, beta])
        out.update(zip(("dres", "dx", "dgamma", "dbeta"), grads))
    return out


def attn_reference(q, k, v, mask, heads, keep, p_drop, dctx=None, dtype=torch.float64):
    """q, k, v [nseq*L, heads*64]; mask [nseq, L] (nonzero = a token); keep bool [nseq, heads, L, L]
    (query, key) or None (p_drop = 0).

    Scores s_ij = q_i . k_j / 8 + (1 - m_j) * finfo(float32).min; P = softmax_j(s); ctx = (P * keep /
    (1 - p)) v.  A fully masked sequence has every score at finfo.min (the O(1) products are absorbed,
    in float32 and in float64 alike): its rows are uniform over the L keys.

    -> dict of detached ``dtype`` tensors: ctx [T, heads*64], m [T, heads] the row maximum of s, il
       [T, heads] = 1 / sum_j exp(s_ij - m_i); with dctx [T, heads*64], of (ctx * dctx).sum(): dq, dk, dv"""
    nseq, L = mask.shape
    T = nseq * L
    q, k, v = (_leaf(t, dtype) for t in (q, k, v))
    ctx, m, l = attn_forward(q, k, v, mask, heads, keep, p_drop)

    def per_query(t):
        return t.squeeze(-1).permute(0, 2, 1).reshape(T, heads).detach()
    out = {"ctx": ctx.detach(), "m": per_query(m), "il": per_query(1.0 / l)}
    if dctx is not None:
        out.update(zip(("dq", "dk", "dv"), torch.autograd.grad((ctx * dctx.detach().to(dtype)).sum(), [q, k, v])))
    return out


def bert_dropout(seed, T, H, heads, p):
    """The counter ranges of one single-layer forward over T rows that starts at offset 0: site[0] the
    embeddings, site[1] the attention probabilities, site[2] the attention-output dense."""
    return R.BertDropout(seed, 0, T, H, 1, heads, p, p)


def attn_mask(L, dtype=torch.int64):
    """The attention tests' batch of 4 sequences of L slots: a full one, a ragged prefix (2L/3 tokens,
    at least one), a fully masked one, and a prefix of L - 1 tokens (L at L = 1) with holes at
    positions 1 and 3 when L > 4."""
    m = torch.zeros(4, L, dtype=dtype)
    m[0] = 1
    m[1, :max(1, 2 * L // 3)] = 1
    m[3, :max(1, L - 1)] = 1
    if L > 4:
        m[3, 1] = 0
        m[3, 3] = 0
    return m


def ln_inputs(T, H, seed):
    """Seeded float32 inputs of the add-LN entries: x 0.7 N(0,1), res N(0,1), gamma 1 + 0.1 N, beta 0.1 N,
    dout N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    return {
        "x": torch.randn(T, H, generator=g) * 0.7,
        "res": torch.randn(T, H, generator=g),
        "gamma": 1 + 0.1 * torch.randn(H, generator=g),
        "beta": 0.1 * torch.randn(H, generator=g),
        "dout": torch.randn(T, H, generator=g),
    }


def embed_inputs(nseq, L, H, V, P, seed):
    """Seeded float32 tables (0.5 N(0,1); the type table has 2 rows, row 0 is used), gamma 1 + 0.1 N,
    beta 0.1 N, dout N(0,1), and ids int64 [nseq, L] in [0, V): with more than two tokens the first is
    the padding id 0 and the last repeats the second."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (nseq, L), generator=g)
    flat = ids.view(-1)
    if flat.numel() > 2:
        flat[0] = 0
        flat[-1] = flat[1]
    return {
        "word": 0.5 * torch.randn(V, H, generator=g),
        "pos": 0.5 * torch.randn(P, H, generator=g),
        "type": 0.5 * torch.randn(2, H, generator=g),
        "gamma": 1 + 0.1 * torch.randn(H, generator=g),
        "beta": 0.1 * torch.randn(H, generator=g),
        "dout": torch.randn(nseq * L, H, generator=g),
        "ids": ids,
    }


def attn_inputs(nseq, L, heads, seed):
    """Seeded float32 q, k, v, dctx [nseq*L, heads*64]: q, k N(0,1) (scores q.k / 8 of unit variance),
    v 0.7 N(0,1), dctx N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    T, H = nseq * L, heads * 64
    return {
        "q": torch.randn(T, H, generator=g),
        "k": torch.randn(T, H, generator=g),
        "v": torch.randn(T, H, generator=g) * 0.7,
        "dctx": torch.randn(T, H, generator=g),
    }
