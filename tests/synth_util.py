"""Plain-torch references of the dense-synthesizer attention core (csrc/synth_attn.hip: nr_synth_attn_fwd /
_bwd, as include/newsrec_hip.h states them), the seeded inputs and cases of their tests, and a differentiable
float64 composition of the whole synthesizer BertModel (models/PLM.py:37-47 with
models/Modules/Synthesizer.py in every layer).

synth_reference evaluates the contract's own formulas in the dtype asked for, without autograd;
tests/test_synth_attn_ref_cpu.py holds it against torch.softmax / relu under autograd and against the
reference module's golden.  The bar of every kernel comparison is sha_attn_util.bar_of's:
32 e32 + 32 * 2^-24 * max|ref64|, e32 the float32 evaluation's own error."""
import torch

from sha_attn_util import bar_of  # noqa: F401  (the project's kernel bar, shared)

LN_EPS = 1e-12
STATE_NAMES = ("dense.0.weight", "dense.0.bias", "dense.2.weight", "dense.2.bias", "value_fn.weight",
               "value_fn.bias")


def synth_inputs(nseq, L, D, seed):
    """Seeded float32 operands of one kernel case: hv, dctx N(0,1) [nseq*L, D]; w1 [L, D] and w2 [L, L] scaled
    for O(1) pre-activations; b1, b2 0.2 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    T = nseq * L
    return {"hv": torch.randn(T, D, generator=g), "dctx": torch.randn(T, D, generator=g),
            "w1": torch.randn(L, D, generator=g) * 1.2 / D ** 0.5, "b1": 0.2 * torch.randn(L, generator=g),
            "w2": torch.randn(L, L, generator=g) * 1.5 / L ** 0.5, "b2": 0.2 * torch.randn(L, generator=g)}


def synth_reference(hv, w1, b1, w2, b2, nseq, L, dctx=None, gate=None, dtype=torch.float64):
    """hv [nseq*L, D], w1 [L, D], b1 [L], w2 [L, L], b2 [L]; gate: bool [nseq*L, L] standing for a1 > 0 in the
    backward (None: the gate of this evaluation's own forward).

    -> dict of ``dtype`` tensors: z1, a1 [T, L], probs [nseq, L, L], ctx [T, D]; with dctx [T, D] also da2, da1
       [T, L], dhv [T, D] and the sums over titles dw1, db1, dw2, db2, by the contract's formulas (no autograd)."""
    T, D = hv.shape
    hv, w1, b1, w2, b2 = (t.to(dtype) for t in (hv, w1, b1, w2, b2))
    z1 = hv @ w1.t() + b1
    a1 = z1.clamp_min(0)
    a2 = a1 @ w2.t() + b2
    e = torch.exp(a2 - a2.max(-1, keepdim=True).values)
    P = (e / e.sum(-1, keepdim=True)).view(nseq, L, L)
    hs = hv.view(nseq, L, D)
    out = {"z1": z1, "a1": a1, "probs": P, "ctx": torch.matmul(P, hs).reshape(T, D)}
    if dctx is not None:
        dc = dctx.to(dtype).view(nseq, L, D)
        dP = torch.matmul(dc, hs.transpose(1, 2))
        dA2 = (P * (dP - (dP * P).sum(-1, keepdim=True))).reshape(T, L)
        gt = (a1 > 0) if gate is None else gate
        dA1 = (dA2 @ w2) * gt.to(dtype)
        out["da2"], out["da1"] = dA2, dA1
        out["dhv"] = torch.matmul(P.transpose(1, 2), dc).reshape(T, D) + dA1 @ w1
        out["dw2"], out["db2"] = dA2.t() @ a1, dA2.sum(0)
        out["dw1"], out["db1"] = dA1.t() @ hv, dA1.sum(0)
    return out


def _kernel_cases():
    """(nseq, L, D): the grid of shapes, two other title counts, the widest model at the longest title, and one
    case on each side of every structural boundary of the kernels: the 16-row thread tiles (L 16 | 17, 32 | 33
    in the grid, 48 | 49), the 64-column chunks (D 64 | 68, 128 | 132) and the backward's LDS request
    (4 * ceil4(L) * 272 B) crossing 64 KB (L 60 | 61)."""
    out = [(4, L, D) for L in (1, 5, 30, 33, 64) for D in (4, 64, 152, 768)]
    out += [(1, 30, 152), (17, 30, 152), (4, 64, 1024)]
    out += [(4, 16, 68), (4, 17, 60), (4, 32, 128), (4, 48, 132), (4, 49, 64), (4, 60, 64), (4, 61, 64)]
    return out


KERNEL_CASES = _kernel_cases()
FWD_TENSORS = ("a1", "probs", "ctx")
BWD_TENSORS = ("da1", "da2", "dhv")


def case_seed(nseq, L, D):
    return 7 + 100000 * nseq + 1000 * L + D


_CASE_CACHE = {}


def case_inputs(nseq, L, D):
    """The case's inputs and its float64 / float32 forward references (computed once, shared, never modified)."""
    key = (nseq, L, D)
    if key not in _CASE_CACHE:
        inp = synth_inputs(nseq, L, D, case_seed(nseq, L, D))
        fwd = {dt: synth_reference(inp["hv"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], nseq, L, dtype=dt)
               for dt in (torch.float64, torch.float32)}
        _CASE_CACHE[key] = (inp, fwd)
    return _CASE_CACHE[key]


def case_references(nseq, L, D, gate=None):
    """-> (inputs, {float64: reference, float32: reference}) of one kernel case, the backward gated by ``gate``
    in both (None: each evaluation's own a1 > 0)."""
    inp, _ = case_inputs(nseq, L, D)
    ref = {dt: synth_reference(inp["hv"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], nseq, L, inp["dctx"], gate,
                               dtype=dt) for dt in (torch.float64, torch.float32)}
    return inp, ref


# ---------------------------------------------------------------------- the whole model

def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, LN_EPS)


def _drop(z, keep, p):
    return z if keep is None else z * keep.reshape(z.shape).to(z.dtype) / (1.0 - p)


def synth_attention_block(P, x, pre, trace=None):
    """Synthesizer.py's BertSelfAttention on x [n, L, H] with the state_dict names under ``pre``; no mask, no
    dropout.  ``trace``: a list that receives this block's z1 [n*L, L]."""
    lin = torch.nn.functional.linear
    hv = lin(x, P[pre + "value_fn.weight"], P[pre + "value_fn.bias"])
    z1 = lin(hv, P[pre + "dense.0.weight"], P[pre + "dense.0.bias"])
    if trace is not None:
        trace.append(z1.detach().reshape(-1, z1.shape[-1]))
    a2 = lin(torch.relu(z1), P[pre + "dense.2.weight"], P[pre + "dense.2.bias"])
    return torch.matmul(torch.softmax(a2, -1), hv)


def synth_bert_model(P, ids, pre="", drop=None, r0=0, trace=None):
    """BertModel(attention_type="synthesizer") on ids [n, L], differentiable, in P's dtype: R.bert_embeddings,
    per layer the block above + BERT's output dense / residual / LayerNorm / GELU FFN, the tanh pooler.  The
    attention mask plays no part.  ``drop``: an R.BertDropout whose hidden-dropout masks are replayed (its
    attention site is unused), this segment's rows starting at row r0 of the fused pass.
    -> (last_hidden_state [n, L, H], pooler_output [n, H])."""
    from oracle import restatement as R
    lin = torch.nn.functional.linear
    n, l = ids.shape
    on = drop is not None and drop.p_h > 0
    keep = drop.embed(r0, n * l).reshape(n, l, -1) if on else None
    h = R.bert_embeddings(P, ids, pre, eps=LN_EPS, keep=keep, p_drop=drop.p_h if on else 0.0)
    for li in range(R.bert_layers(P, pre)):
        lp = pre + "encoder.layer.%d." % li
        cx = synth_attention_block(P, h, lp + "attention.self.", trace)
        a = lin(cx, P[lp + "attention.output.dense.weight"], P[lp + "attention.output.dense.bias"])
        a = _drop(a, drop.dense(li, 0, r0, n * l) if on else None, drop.p_h if on else 0.0)
        h1 = _ln(a + h, P[lp + "attention.output.LayerNorm.weight"], P[lp + "attention.output.LayerNorm.bias"])
        f = torch.nn.functional.gelu(lin(h1, P[lp + "intermediate.dense.weight"], P[lp + "intermediate.dense.bias"]))
        o = lin(f, P[lp + "output.dense.weight"], P[lp + "output.dense.bias"])
        o = _drop(o, drop.dense(li, 1, r0, n * l) if on else None, drop.p_h if on else 0.0)
        h = _ln(o + h1, P[lp + "output.LayerNorm.weight"], P[lp + "output.LayerNorm.bias"])
    pooled = torch.tanh(lin(h[:, 0], P[pre + "pooler.dense.weight"], P[pre + "pooler.dense.bias"]))
    return h, pooled


# the model fixture of the GPU model tests: 2 layers, hidden 128 (2 heads of 64), FFN 256, L 5, 6 titles
FIX = dict(layers=2, hidden=128, heads=2, ffn=256, L=5, nseq=6, vocab=64, max_pos=16, p_hidden=0.1)
FIX_SEED = 3          # tests/test_synth_attn_ref_cpu.py: every ReLU pre-activation of the fixture is >= 1e-4 from 0
FIX_TORCH_SEED = 11   # torch.manual_seed before the model is built: the seed of its dropout stream


def fixture_shapes():
    """state_dict name -> shape of the fixture's BertModel(attention_type="synthesizer"), in state_dict order."""
    H, I, L, V, MP = FIX["hidden"], FIX["ffn"], FIX["L"], FIX["vocab"], FIX["max_pos"]
    sh = [("embeddings.word_embeddings.weight", (V, H)), ("embeddings.position_embeddings.weight", (MP, H)),
          ("embeddings.token_type_embeddings.weight", (2, H)), ("embeddings.LayerNorm.weight", (H,)),
          ("embeddings.LayerNorm.bias", (H,))]
    for i in range(FIX["layers"]):
        p = "encoder.layer.%d." % i
        sh += [(p + "attention.self.dense.0.weight", (L, H)), (p + "attention.self.dense.0.bias", (L,)),
               (p + "attention.self.dense.2.weight", (L, L)), (p + "attention.self.dense.2.bias", (L,)),
               (p + "attention.self.value_fn.weight", (H, H)), (p + "attention.self.value_fn.bias", (H,)),
               (p + "attention.output.dense.weight", (H, H)), (p + "attention.output.dense.bias", (H,)),
               (p + "attention.output.LayerNorm.weight", (H,)), (p + "attention.output.LayerNorm.bias", (H,)),
               (p + "intermediate.dense.weight", (I, H)), (p + "intermediate.dense.bias", (I,)),
               (p + "output.dense.weight", (H, I)), (p + "output.dense.bias", (H,)),
               (p + "output.LayerNorm.weight", (H,)), (p + "output.LayerNorm.bias", (H,))]
    sh += [("pooler.dense.weight", (H, H)), ("pooler.dense.bias", (H,))]
    return sh


def fixture(seed=FIX_SEED):
    """-> (params: name -> float32 tensor, ids int64 [6, 5] with pad tokens, mask int64 [6, 5], cotangents a
    [6, 5, H] and b [6, H]) of the model tests; O(1) pre-activations everywhere."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, shape in fixture_shapes():
        if "embeddings." in name and len(shape) == 2:
            P[name] = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith("LayerNorm.weight"):
            P[name] = 1 + 0.2 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            P[name] = 0.2 * torch.randn(shape, generator=g)
        else:
            P[name] = torch.randn(shape, generator=g) * 1.2 / shape[1] ** 0.5
    n, L = FIX["nseq"], FIX["L"]
    ids = torch.randint(1, FIX["vocab"], (n, L), generator=g)
    lens = torch.tensor([5, 3, 1, 4, 5, 2])
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    ids = ids * mask                                      # pad tokens (id 0) behind every title's length
    a = torch.randn(n, L, FIX["hidden"], generator=g)
    b = torch.randn(n, FIX["hidden"], generator=g)
    return P, ids, mask, a, b
