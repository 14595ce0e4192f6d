"""Plain-torch references of the one-head attention core (csrc/sha_attn.hip: nr_sha_attn_fwd / _bwd, as
include/newsrec_hip.h states them), the seeded inputs, masks and cases of their tests, and a float64
composition of the whole Transformer_Encoder (models/Encoders/Transformer.py, OneLayerBert.py).

sha_reference evaluates the contract's own formulas in the dtype asked for, the dropout keep mask passed
in; tests/test_sha_attn_ref_cpu.py holds it against torch.softmax under autograd and the composition
against the reference model's golden."""
import math

import torch

from bert_util import attn_mask as _four_titles

LN_EPS = 1e-12


def sha_mask(nseq, L, dtype=torch.int64):
    """bert_util.attn_mask's four titles (full, ragged prefix, fully masked, prefix with holes), repeated
    or cut to nseq titles."""
    m = _four_titles(L, dtype)
    return m.repeat((nseq + 3) // 4, 1)[:nseq].contiguous()


def sha_inputs(nseq, L, D, seed):
    """Seeded float32 q, k N(0,1) (scaled scores of unit variance), v 0.7 N(0,1), dctx N(0,1), each [nseq*L, D]."""
    g = torch.Generator().manual_seed(seed)
    T = nseq * L
    return {"q": torch.randn(T, D, generator=g), "k": torch.randn(T, D, generator=g),
            "v": torch.randn(T, D, generator=g) * 0.7, "dctx": torch.randn(T, D, generator=g)}


def sha_keep(seed, offset, nseq, L, p):
    """The kernels' keep mask [nseq, L, L] (query, key): element (s*L + i)*L + j of key (seed, offset)."""
    from oracle import restatement as R
    return R.dropout_keep(seed, offset, nseq * L, L, p).view(nseq, L, L)


def sha_reference(q, k, v, mask, scale, keep=None, p_drop=0.0, dctx=None, dtype=torch.float64):
    """q, k, v [nseq*L, D]; mask [nseq, L] (nonzero = a token); keep bool [nseq, L, L] or None (p_drop = 0).

    -> dict of ``dtype`` tensors: probs [nseq, L, L] = softmax over the unmasked keys of scale * q k^T, exactly
       0 at masked keys (all zero for a title without a token), ctx [T, D] = (probs * keep / (1 - p)) v; with
       dctx [T, D] also dq, dk, dv [T, D] by the contract's formulas (no autograd)."""
    nseq, L = mask.shape
    D = q.shape[1]
    q, k, v = (t.to(dtype).view(nseq, L, D) for t in (q, k, v))
    m = (mask != 0)[:, None, :].expand(nseq, L, L)
    s = torch.matmul(q, k.transpose(1, 2)) * scale
    s = s.masked_fill(~m, -math.inf)
    mx = s.max(-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)                       # exp(-inf) = 0 at masked keys
    den = e.sum(-1, keepdim=True)
    P = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    kf = torch.ones_like(P) if keep is None else keep.to(dtype) / (1.0 - p_drop)
    Pd = P * kf
    out = {"probs": P, "ctx": torch.matmul(Pd, v).reshape(nseq * L, D)}
    if dctx is not None:
        dc = dctx.to(dtype).view(nseq, L, D)
        g = torch.matmul(dc, v.transpose(1, 2)) * kf
        dS = P * (g - (g * P).sum(-1, keepdim=True))
        out["dv"] = torch.matmul(Pd.transpose(1, 2), dc).reshape(nseq * L, D)
        out["dq"] = (scale * torch.matmul(dS, k)).reshape(nseq * L, D)
        out["dk"] = (scale * torch.matmul(dS.transpose(1, 2), q)).reshape(nseq * L, D)
    return out


def _kernel_cases():
    """(nseq, L, D, p): the grid of shapes, two other title counts, the widest model at the longest title, and
    one case on each side of every structural boundary of the kernels: the 16-row thread tiles (L 16 | 17,
    32 | 33, 48 | 49), the 64-column chunks (D 64 | 68, 128 | 132) and the backward's LDS request crossing
    64 KB (L 40 | 41)."""
    out = [(4, L, D, p) for L in (1, 5, 30, 33, 64) for D in (4, 64, 152, 384) for p in (0.0, 0.1)]
    out += [(1, 30, 152, 0.1), (17, 30, 152, 0.1), (4, 64, 1024, 0.1)]
    out += [(4, 16, 68, 0.1), (4, 17, 60, 0.0), (4, 32, 128, 0.1), (4, 48, 132, 0.0), (4, 49, 64, 0.1),
            (4, 40, 64, 0.1), (4, 41, 64, 0.0)]
    return out


KERNEL_CASES = _kernel_cases()
KERNEL_SEED, KERNEL_OFFSET = 0x5EED, 12345
TENSORS = ("ctx", "probs", "dq", "dk", "dv")


def case_seed(nseq, L, D):
    return 100000 * nseq + 1000 * L + D


def case_references(nseq, L, D, p):
    """-> (inputs, mask, keep or None, {float64: reference, float32: reference}) of one kernel case."""
    inp = sha_inputs(nseq, L, D, case_seed(nseq, L, D))
    mask = sha_mask(nseq, L)
    keep = sha_keep(KERNEL_SEED, KERNEL_OFFSET, nseq, L, p) if p > 0 else None
    ref = {dt: sha_reference(inp["q"], inp["k"], inp["v"], mask, 1.0 / math.sqrt(D), keep, p, inp["dctx"], dtype=dt)
           for dt in (torch.float64, torch.float32)}
    return inp, mask, keep, ref


def bar_of(ref, name):
    """-> (bar, e32, max|ref64|): the project's bar 32 e32 + 32 * 2^-24 * max|ref64| of one tensor."""
    want = ref[torch.float64][name]
    scale = want.abs().max().item()
    e32 = (ref[torch.float32][name].double() - want).abs().max().item()
    return 32 * e32 + 32 * 2.0 ** -24 * scale, e32, scale


# ---------------------------------------------------------------------- the whole encoder

def _drop(z, keep, p):
    return z if keep is None else z * keep.reshape(z.shape).to(z.dtype) / (1.0 - p)


def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, LN_EPS)


def encoder_reference(P, x, mask, keeps=None, ps=(0.0, 0.0, 0.0), pre=""):
    """Transformer_Encoder on embeddings x [..., L, E] with mask [..., L], differentiable, in x's dtype.
    P: the state_dict names (prefix ``pre``) -> tensors.  keeps: None (eval) or three bool keep masks
    ([n, L, L], [n*L, H], [n*L, H]; None where that rate is 0) of the attention probabilities, the
    attention-output dense and the FFN-output dense, with their rates ps.  -> (tok [..., L, H], news [..., H])."""
    lin = torch.nn.functional.linear
    lead = x.shape[:-2]
    L, E = x.shape[-2:]
    g = lambda n: P[pre + n]   # noqa: E731
    H = g("project.weight").shape[0]
    keeps = (None, None, None) if keeps is None else keeps
    x0 = lin(x.reshape(-1, L, E), g("project.weight"), g("project.bias"))
    n = x0.shape[0]
    m = (mask.reshape(n, 1, L) != 0)
    at = "bert.attention.self."
    q, k, v = (lin(x0, g(at + t + ".weight"), g(at + t + ".bias")) for t in ("query", "key", "value"))

    def xsoftmax(s):
        p = torch.softmax(s.masked_fill(~m, -math.inf), -1)
        return torch.where(m, p, torch.zeros_like(p))      # also clears the NaN rows of a title without a token
    Pm = xsoftmax(torch.matmul(q, k.transpose(1, 2)) / math.sqrt(H))
    cx = torch.matmul(_drop(Pm, keeps[0], ps[0]), v)
    ao = "bert.attention.output."
    a = _ln(_drop(lin(cx, g(ao + "dense.weight"), g(ao + "dense.bias")).reshape(n * L, H), keeps[1], ps[1])
            .reshape(n, L, H) + x0, g(ao + "LayerNorm.weight"), g(ao + "LayerNorm.bias"))
    f = torch.nn.functional.gelu(lin(a, g("bert.intermediate.dense.weight"), g("bert.intermediate.dense.bias")))
    bo = "bert.output."
    tok = _ln(_drop(lin(f, g(bo + "dense.weight"), g(bo + "dense.bias")).reshape(n * L, H), keeps[2], ps[2])
              .reshape(n, L, H) + a, g(bo + "LayerNorm.weight"), g(bo + "LayerNorm.bias"))
    pw = xsoftmax(torch.matmul(g("query_words"), tok.transpose(1, 2)) / math.sqrt(H))     # [n, 1, L]
    news = torch.matmul(pw, tok).squeeze(1)
    return tok.reshape(*lead, L, H), news.reshape(*lead, H)


def encoder_keeps(seed, offset, n, L, H, ps):
    """The three keep masks of one training forward whose counter range starts at ``offset``."""
    from oracle import restatement as R
    T = n * L
    return (sha_keep(seed, offset, n, L, ps[0]) if ps[0] > 0 else None,
            R.dropout_keep(seed, offset + T * L, T, H, ps[1]) if ps[1] > 0 else None,
            R.dropout_keep(seed, offset + T * L + T * H, T, H, ps[2]) if ps[2] > 0 else None)
