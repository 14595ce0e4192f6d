"""Plain-torch restatements of the `-b deberta` PLM tower: the disentangled attention core as
include/newsrec_hip.h states nr_deb_attn_fwd / _bwd (dpk and dpq by their formulas, no autograd), a
differentiable composition of the whole DebertaModel + PLM's pooler in the dtype of its parameters, the case
grids of the kernel tests, and the replay of the tower's dropout counters (newsrec_amd/deberta.py's layout).

tests/test_deberta_ref_cpu.py holds the composition against the float64 golden of the installed
transformers' DebertaModel (tests/golden/make_deberta_golden.py) and the kernel contract against autograd.
The bar of every kernel comparison is sha_attn_util.bar_of's: 32 e32 + 32 * 2^-24 * max|ref64|."""
import glob
import os

import numpy as np
import torch

from sha_attn_util import bar_of, sha_mask  # noqa: F401  (the project's kernel bar and masks, shared)

LN_EPS = 1e-7
HEAD = 64
# the library takes sqrt(3 * 64) in float32 (scaled_size_sqrt), also in a .double() model
SCALE = 1.0 / float(torch.sqrt(torch.tensor(3.0 * HEAD, dtype=torch.float32)))
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    """tests/golden/deberta.npz and its deberta.part<k>.npz files as one dict of numpy arrays."""
    out = {}
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, "deberta.npz")) +
                   glob.glob(os.path.join(GOLDEN_DIR, "deberta.part*.npz")))
    assert paths, "tests/golden/deberta.npz is missing"
    for p in paths:
        with np.load(p) as d:
            for k in d.files:
                assert k not in out, k
                out[k] = d[k]
    return out


def golden_params(g, dtype=torch.float64, requires_grad=False):
    """The golden's parameters (model names in state_dict order, then pooler.0.*) -> name -> tensor."""
    names = [str(n) for n in g["meta.names"]] + ["pooler.0.weight", "pooler.0.bias"]
    return {n: torch.from_numpy(g[n]).to(dtype).requires_grad_(requires_grad) for n in names}


# ---------------------------------------------------------------------- the attention core

def delta_index(L):
    """delta(i, j) = i - j + L, [L, L] int64, in [1, 2L - 1]."""
    r = torch.arange(L)
    return r[:, None] - r[None, :] + L


def deb_scores(q, k, pk, pq, scale):
    """q, k [n, h, L, 64], pk, pq [2L, h, 64] -> S [n, h, L, L] = scale (q_i.k_j + q_i.pk[delta] + k_j.pq[delta]).
    Differentiable.  (A reference may form the L x 2L products and gather; the kernels do not.)"""
    n, h, L, _ = q.shape
    idx = delta_index(L).to(q.device)
    pkh, pqh = pk.permute(1, 0, 2), pq.permute(1, 0, 2)                      # [h, 2L, 64]
    c2c = torch.matmul(q, k.transpose(-1, -2))
    c2p = torch.gather(torch.matmul(q, pkh.transpose(-1, -2)), -1, idx.expand(n, h, L, L))
    # p2c[i][j] = k_j . pq[delta(i, j)]: gather row j of k pq^T at delta(i, j), then transpose
    p2c = torch.gather(torch.matmul(k, pqh.transpose(-1, -2)), -1, idx.t().expand(n, h, L, L)).transpose(-1, -2)
    return scale * (c2c + c2p + p2c)


def deb_probs(S, mask):
    """The library's masked_fill(finfo.min) + softmax: a query with mask 1 attends to the keys with mask 1
    (exactly 0 elsewhere), a query with mask 0 gets 1 / L at every key.  S [n, h, L, L], mask [n, L]."""
    n, h, L, _ = S.shape
    m = mask != 0
    km = m[:, None, None, :].expand(n, h, L, L)
    qm = m[:, None, :, None].expand(n, h, L, L)
    both = km & qm
    fill = S.masked_fill(~both, -float("inf"))
    mx = fill.max(-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.where(both, torch.exp(torch.where(both, S - mx, torch.zeros_like(S))), torch.zeros_like(S))
    den = e.sum(-1, keepdim=True)
    P = e / torch.where(den > 0, den, torch.ones_like(den))
    return torch.where(qm, P, torch.full_like(P, 1.0 / L))


def deb_keep(seed, offset, nseq, heads, L, p):
    """The kernels' keep mask [nseq, heads, L, L]: element ((s heads + h) L + i) L + j of key (seed, offset)."""
    from oracle import restatement as R
    return R.dropout_keep(seed, offset, nseq * heads * L, L, p).view(nseq, heads, L, L)


def deb_reference(q, k, v, pk, pq, mask, scale, keep=None, p_drop=0.0, dctx=None, dtype=torch.float64):
    """q, k, v [n, h, L, 64] (biases added), pk, pq [2L, h, 64], mask [n, L], keep bool [n, h, L, L] or None.

    -> dict of ``dtype`` tensors: probs [n, h, L, L], ctx [n, L, h, 64]; with dctx [n, L, h, 64] also dq, dk, dv
       [n, h, L, 64] and dpk, dpq [2L, h, 64] (summed over titles), by the contract's formulas (no autograd)."""
    q, k, v, pk, pq = (t.to(dtype) for t in (q, k, v, pk, pq))
    n, h, L, d = q.shape
    P = deb_probs(deb_scores(q, k, pk, pq, scale), mask)
    kf = torch.ones_like(P) if keep is None else keep.to(dtype) / (1.0 - p_drop)
    Pd = P * kf
    out = {"probs": P, "ctx": torch.matmul(Pd, v).permute(0, 2, 1, 3).contiguous()}
    if dctx is not None:
        dc = dctx.to(dtype).permute(0, 2, 1, 3)                              # [n, h, L, 64]
        g = torch.matmul(dc, v.transpose(-1, -2)) * kf
        qm = (mask != 0)[:, None, :, None].to(dtype)
        dS = scale * P * (g - (g * P).sum(-1, keepdim=True)) * qm             # a masked query's P is constant
        idx = delta_index(L)
        pk_g = pk.permute(1, 0, 2)[:, idx]                                   # [h, L, L, 64]: pk[delta(i, j)]
        pq_g = pq.permute(1, 0, 2)[:, idx]
        out["dv"] = torch.matmul(Pd.transpose(-1, -2), dc)
        out["dq"] = torch.matmul(dS, k) + torch.einsum("nhij,hijd->nhid", dS, pk_g)
        out["dk"] = torch.matmul(dS.transpose(-1, -2), q) + torch.einsum("nhij,hijd->nhjd", dS, pq_g)
        flat = idx.reshape(-1)
        tq = torch.einsum("nhij,nhid->ijhd", dS, q).reshape(L * L, h, d)     # dS[i][j] q_i summed over titles
        tk = torch.einsum("nhij,nhjd->ijhd", dS, k).reshape(L * L, h, d)
        out["dpk"] = torch.zeros(2 * L, h, d, dtype=dtype).index_add_(0, flat, tq)
        out["dpq"] = torch.zeros(2 * L, h, d, dtype=dtype).index_add_(0, flat, tk)
    return out


def deb_inputs(nseq, L, heads, seed):
    """Seeded float32 operands of one kernel case: q, k, pk, pq N(0,1) (scaled scores of unit variance), v
    0.7 N(0,1), dctx N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return {"q": r(nseq, heads, L, HEAD), "k": r(nseq, heads, L, HEAD), "v": 0.7 * r(nseq, heads, L, HEAD),
            "pk": r(2 * L, heads, HEAD), "pq": r(2 * L, heads, HEAD), "dctx": r(nseq, L, heads, HEAD)}


def _kernel_cases():
    """(nseq, L, heads, layout, p).  The grid (L x heads x nseq x both column layouts x p), and one case on each
    side of every structural boundary of the kernels:
      the 16-row thread tiles, L 16 | 17, 32 | 33 (grid: 30, 33), 48 | 49;
      the forward's LDS request (3 ceil4(L) + 2 L) 272 B crossing 64 KB, L 48 | 49, the backward's
      (4 ceil4(L) + 4 L) 272 B, L 28 | 29;
      the backward's walkers G = min(nseq, max(1, 512 / heads)): nseq 42 | 43 at 12 heads, 512 | 513 at 1;
    and one whose (title, head) count exceeds the workgroups launched so that the walk and the ordered
    reduction wrap (nseq 300, L 5, 2 heads: 256 walkers per head)."""
    out = [(n, L, h, lay, p) for L in (1, 5, 30, 33, 64) for h in (1, 2, 12) for n in (1, 4, 17)
           for lay in ("interleaved", "blocked") for p in (0.0, 0.1)]
    out += [(4, 16, 2, "interleaved", 0.1), (4, 17, 2, "blocked", 0.0), (4, 32, 2, "interleaved", 0.1),
            (4, 48, 2, "interleaved", 0.1), (4, 49, 2, "blocked", 0.1), (4, 28, 2, "blocked", 0.1),
            (4, 29, 2, "interleaved", 0.0), (42, 5, 12, "interleaved", 0.1), (43, 5, 12, "interleaved", 0.1),
            (512, 3, 1, "blocked", 0.1), (513, 3, 1, "blocked", 0.1), (300, 5, 2, "interleaved", 0.1)]
    return out


KERNEL_CASES = _kernel_cases()
KERNEL_SEED, KERNEL_OFFSET = 0xDEB, 54321
TENSORS = ("ctx", "probs", "dq", "dk", "dv", "dpk", "dpq")


def case_id(c):
    return "n%d-L%d-h%d-%s-p%g" % c


_CASE_CACHE = {}


def case_references(nseq, L, heads, p):
    """-> (inputs, mask, keep or None, {float64: reference, float32: reference}) of one kernel case; computed
    once and shared by both column layouts, never modified."""
    key = (nseq, L, heads, p)
    if key not in _CASE_CACHE:
        if len(_CASE_CACHE) > 8:
            _CASE_CACHE.clear()
        inp = deb_inputs(nseq, L, heads, 100000 * nseq + 1000 * L + heads)
        mask = sha_mask(nseq, L)
        keep = deb_keep(KERNEL_SEED, KERNEL_OFFSET, nseq, heads, L, p) if p > 0 else None
        ref = {dt: deb_reference(inp["q"], inp["k"], inp["v"], inp["pk"], inp["pq"], mask, SCALE, keep, p,
                                 inp["dctx"], dtype=dt) for dt in (torch.float64, torch.float32)}
        _CASE_CACHE[key] = (inp, mask, keep, ref)
    return _CASE_CACHE[key]


# ---------------------------------------------------------------------- the whole model

def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, LN_EPS)


def _drop(z, keep, p):
    return z if keep is None else z * keep.reshape(z.shape).to(z.dtype) / (1.0 - p)


class DebertaDropout:
    """The dropout of ONE DebertaFn training forward over segments of ``shapes`` = [(nseq, L), ...], restated
    from newsrec_amd/deberta.py's counter layout: ``offset`` is the model's _DropoutStream offset before the
    forward; sites: embeddings [T H], then per layer the relative rows, the attention probabilities, the
    attention-output dense [T H] and the FFN-output dense [T H]."""

    def __init__(self, seed, offset, shapes, H, layers, heads, p_hidden, p_attn):
        self.seed, self.H, self.heads, self.shapes = int(seed), H, heads, list(shapes)
        self.p_h, self.p_a = float(p_hidden), float(p_attn)
        T = sum(n * l for n, l in shapes)
        self.rel0 = [sum(2 * l * H for _, l in shapes[:g]) for g in range(len(shapes) + 1)]
        self.att0 = [sum(n * heads * l * l for n, l in shapes[:g]) for g in range(len(shapes) + 1)]
        sizes = [T * H] + [self.rel0[-1], self.att0[-1], T * H, T * H] * layers
        self.site, r = [], int(offset)
        for n in sizes:
            self.site.append(r)
            r += n
        self.end = r

    def _keep(self, offset, rows, width, p, row0=0):
        from oracle import restatement as R
        return R.dropout_keep(self.seed, offset, rows, width, p, row0=row0) if p > 0 else None

    def embed(self, r0, rows):
        return self._keep(self.site[0] + r0 * self.H, rows, self.H, self.p_h)

    def rel(self, layer, seg):
        return self._keep(self.site[1 + 4 * layer] + self.rel0[seg], 2 * self.shapes[seg][1], self.H, self.p_h)

    def attn(self, layer, seg):
        n, l = self.shapes[seg]
        k = self._keep(self.site[2 + 4 * layer] + self.att0[seg], n * self.heads * l, l, self.p_a)
        return None if k is None else k.view(n, self.heads, l, l)

    def dense(self, layer, which, r0, rows):
        return self._keep(self.site[3 + 4 * layer + which], rows, self.H, self.p_h, row0=r0)


def deberta_layers(P, pre=""):
    n = 0
    while pre + "encoder.layer.%d.attention.self.in_proj.weight" % n in P:
        n += 1
    return n


def deberta_model(P, ids, mask, pre="", drop=None, seg=0, r0=0, scale=SCALE):
    """DebertaModel on ids, mask [n, L], differentiable, in P's dtype -> last_hidden_state [n, L, H].
    ``drop``: a DebertaDropout whose masks are replayed for segment ``seg`` starting at row r0 of the pass."""
    lin = torch.nn.functional.linear
    n, L = ids.shape
    g = lambda name: P[pre + name]   # noqa: E731
    H = g("embeddings.LayerNorm.weight").shape[0]
    heads = H // HEAD
    KP = g("encoder.rel_embeddings.weight").shape[0] // 2
    p_h = drop.p_h if drop is not None else 0.0
    p_a = drop.p_a if drop is not None else 0.0
    m = (mask != 0).to(g("embeddings.LayerNorm.weight").dtype)[..., None]
    x = _ln(g("embeddings.word_embeddings.weight")[ids], g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"))
    x = _drop(x, drop.embed(r0, n * L) if drop else None, p_h) * m
    for li in range(deberta_layers(P, pre)):
        lp = "encoder.layer.%d." % li
        at = lp + "attention.self."
        qkv = lin(x, g(at + "in_proj.weight")).view(n, L, heads, 3 * HEAD).permute(0, 2, 1, 3)
        q, k, v = qkv.chunk(3, -1)
        q = q + g(at + "q_bias").view(1, heads, 1, HEAD)
        v = v + g(at + "v_bias").view(1, heads, 1, HEAD)
        rel = _drop(g("encoder.rel_embeddings.weight")[KP - L: KP + L], drop.rel(li, seg) if drop else None, p_h)
        pk = lin(rel, g(at + "pos_proj.weight")).view(2 * L, heads, HEAD)
        pq = lin(rel, g(at + "pos_q_proj.weight"), g(at + "pos_q_proj.bias")).view(2 * L, heads, HEAD)
        Pm = deb_probs(deb_scores(q, k, pk, pq, scale), mask)
        cx = torch.matmul(_drop(Pm, drop.attn(li, seg) if drop else None, p_a), v).permute(0, 2, 1, 3).reshape(n, L, H)
        a = lin(cx, g(lp + "attention.output.dense.weight"), g(lp + "attention.output.dense.bias"))
        a = _drop(a, drop.dense(li, 0, r0, n * L) if drop else None, p_h)
        h1 = _ln(a + x, g(lp + "attention.output.LayerNorm.weight"), g(lp + "attention.output.LayerNorm.bias"))
        f = torch.nn.functional.gelu(lin(h1, g(lp + "intermediate.dense.weight"), g(lp + "intermediate.dense.bias")))
        o = lin(f, g(lp + "output.dense.weight"), g(lp + "output.dense.bias"))
        o = _drop(o, drop.dense(li, 1, r0, n * L) if drop else None, p_h)
        x = _ln(o + h1, g(lp + "output.LayerNorm.weight"), g(lp + "output.LayerNorm.bias"))
    return x


def plm_pooler(P, hid, pre="pooler."):
    """PLM.py:26-28,102-106: GELU(Linear(last_hidden_state[:, 0]))."""
    return torch.nn.functional.gelu(torch.nn.functional.linear(hid[:, 0], P[pre + "0.weight"], P[pre + "0.bias"]))
