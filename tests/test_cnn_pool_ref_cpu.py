"""The references of tests/test_cnn_pool_kernels_gpu.py against oracle/restatement.py, in float64 to
1e-12 of each tensor's maximum (no GPU):

  cnn_pool_util.cnn_keypool_reference   against cnn_news (CNN.py:30-50) fed the same conv weights: the
      token output, the news vectors and, by autograd through cnn_news, the gradients of the key projection,
      the query and the conv bias; the gradient of the conv PRE-activation (the reference's dc) through an
      identity conv, where it is the embedding's gradient itself, and through a seeded conv, where dc
      pushed through the conv's own backward must give cnn_news's embedding and conv-weight gradients
  pool_util.attn_pool_reference         as nr_seq_pool_* use it (no LayerNorm, no dropout), against
      scaled_dp_attention with the key tied to the values and with a separate tanh key
and the places both make exactly zero: a fully masked sequence, and every feature at or past H of a
zero-padded head."""
import math

import pytest
import torch
import torch.nn.functional as F

from cnn_pool_util import cnn_keypool_inputs, cnn_keypool_reference, seq_pool_dq_per_seq, typed_mask
from oracle import restatement as R
from pool_util import attn_pool_inputs, attn_pool_reference, pool_mask

F64 = torch.float64
PRE = "encoderN."


def _close(got, want, name):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * scale, "%s: err %.3e of max %.3e" % (name, err, scale)


def _cnn_params(H, E, seed, identity):
    g = torch.Generator().manual_seed(seed)
    if identity:       # pre-activation = the embedding itself
        assert E == H
        w = torch.zeros(H, E, 3, dtype=F64)
        w[:, :, 1] = torch.eye(H, dtype=F64)
        b = torch.zeros(H, dtype=F64)
    else:
        w = torch.randn(H, E, 3, generator=g, dtype=F64) * (1.0 / (3 * E)) ** 0.5
        b = torch.randn(H, generator=g, dtype=F64) * 0.1
    P = {PRE + "cnn.weight": w, PRE + "cnn.bias": b,
         PRE + "wordQueryProject.weight": torch.randn(H, H, generator=g, dtype=F64) * (2.0 / H) ** 0.5,
         PRE + "wordQueryProject.bias": torch.randn(H, generator=g, dtype=F64) * 0.1,
         PRE + "query_words": torch.randn(1, H, generator=g, dtype=F64)}
    return {k: v.requires_grad_() for k, v in P.items()}, g


@pytest.mark.parametrize("L,H,E,identity,with_dz", [(7, 20, 20, True, True), (7, 20, 20, True, False),
                                                    (6, 20, 24, False, True), (1, 5, 8, False, False),
                                                    (32, 33, 40, False, True)])
def test_cnn_keypool_reference_matches_cnn_news(L, H, E, identity, with_dz):
    P, g = _cnn_params(H, E, 100 * L + H, identity)
    mask = pool_mask(L)
    n = mask.shape[0]
    emb = torch.randn(n, L, E, generator=g, dtype=F64).requires_grad_()
    dnews = torch.randn(n, H, generator=g, dtype=F64)
    dz = torch.randn(n * L, H, generator=g, dtype=F64) if with_dz else None
    c, news = R.cnn_news(emb, mask, P)
    loss = (news * dnews).sum()
    if with_dz:
        loss = loss + (c.reshape(n * L, H) * dz).sum()
    names = [PRE + "wordQueryProject.weight", PRE + "wordQueryProject.bias", PRE + "query_words", PRE + "cnn.bias",
             PRE + "cnn.weight"]
    demb, dwq, dbq, dq, dcb, dcw = torch.autograd.grad(loss, [emb] + [P[k] for k in names])

    ref = cnn_keypool_reference(c.detach().reshape(n * L, H), P[names[0]], P[names[1]], P[names[2]].reshape(H), mask,
                                dnews=dnews, dz=dz)
    _close(ref["news"], news.detach(), "news")
    key = torch.tanh(F.linear(c.detach(), P[names[0]].detach(), P[names[1]].detach())).reshape(n * L, H)
    _close(ref["K"], key, "K")
    _close(ref["dwq"], dwq, "dwq")
    _close(ref["dbq"], dbq, "dbq")
    _close(ref["dq"], dq.reshape(H), "dq")
    _close(ref["dconv_b"], dcb, "dconv_b")
    if identity:
        _close(ref["dc"].reshape(n, L, H), demb, "dc")
    # dc is the gradient of the conv's pre-activation: the conv's own backward takes it to the
    # embedding's and the conv weight's gradients
    e2 = emb.detach().clone().requires_grad_()
    w2 = P[PRE + "cnn.weight"].detach().clone().requires_grad_()
    pre = F.conv1d(e2.transpose(1, 2), w2, None, padding=1).transpose(1, 2)
    de2, dw2 = torch.autograd.grad(pre, [e2, w2], ref["dc"].reshape(n, L, H))
    _close(de2, demb, "demb")
    _close(dw2, dcw, "dconv_w")
    # and it is gated: exactly zero wherever the conv output is
    assert (ref["dc"][c.detach().reshape(n * L, H) <= 0] == 0).all()


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32, torch.bool])
def test_cnn_keypool_reference_exact_zeros_and_padding(dtype):
    """A fully masked title pools exact zeros and passes no gradient but dz; a head zero-padded from H to
    Hp gives the same numbers and exact zeros at or past H; the mask's dtype and values do not matter."""
    L, H, Hp = 9, 20, 32
    mask = typed_mask(L, 16, dtype)
    n = mask.shape[0]
    inp = cnn_keypool_inputs(n, L, H, 5)
    for with_dz in (False, True):
        dz = inp["dz"] if with_dz else None
        ref = cnn_keypool_reference(inp["C"], inp["wq"], inp["bq"], inp["q"], mask, inp["dnews"], dz)
        plain = cnn_keypool_reference(inp["C"], inp["wq"], inp["bq"], inp["q"], (mask != 0).long(), inp["dnews"], dz)
        for k in ref:
            assert torch.equal(ref[k], plain[k]), k
        empty = ((mask != 0).sum(1) == 0).nonzero().flatten().tolist()
        assert empty == [0, 8]
        for s in empty:
            assert (ref["news"][s] == 0).all() and (ref["probs"][s] == 0).all()
            rows = ref["dc"][s * L:(s + 1) * L]
            gate = (inp["C"][s * L:(s + 1) * L] > 0).double()
            assert torch.equal(rows, inp["dz"][s * L:(s + 1) * L].double() * gate if with_dz else torch.zeros_like(rows))
        assert (ref["probs"][mask == 0] == 0).all()

        def pad(t, *shape):
            o = torch.zeros(*shape)
            o[tuple(slice(0, s) for s in t.shape)] = t
            return o
        big = cnn_keypool_reference(pad(inp["C"], n * L, Hp), pad(inp["wq"], Hp, Hp), pad(inp["bq"], Hp), pad(inp["q"], Hp),
                                    mask, pad(inp["dnews"], n, Hp), None if dz is None else pad(dz, n * L, Hp))
        s = math.sqrt(H / Hp)        # the padded head divides its scores by sqrt(Hp)
        scaled = cnn_keypool_reference(inp["C"], inp["wq"], inp["bq"], inp["q"].double() * s, mask, inp["dnews"], dz)
        for k in ("K", "news", "dc", "dbq", "dconv_b"):
            _close(big[k][..., :H], scaled[k], k)
            assert (big[k][..., H:] == 0).all(), k
        _close(big["probs"], scaled["probs"], "probs")
        _close(big["dwq"][:H, :H], scaled["dwq"], "dwq")
        assert (big["dwq"][H:] == 0).all() and (big["dwq"][:, H:] == 0).all()
        _close(big["dq"][:H], scaled["dq"] * s, "dq")
        assert (big["dq"][H:] == 0).all()


@pytest.mark.parametrize("L,D", [(1, 5), (9, 6), (33, 150), (64, 3)])
@pytest.mark.parametrize("tied", [True, False])
def test_seq_pool_reference_matches_scaled_dp_attention(L, D, tied):
    mask = pool_mask(L, dtype=F64)
    n = mask.shape[0]
    inp = attn_pool_inputs(n, L, D, 10 * L + D)
    x = inp["x"].double().requires_grad_()
    kpre = torch.atanh(inp["key"].double()).requires_grad_()       # the stored key is its tanh
    q = inp["q"].double().requires_grad_()
    k = x if tied else torch.tanh(kpre)
    want = R.scaled_dp_attention(q.view(1, 1, D).expand(n, 1, D), k.view(n, L, D), x.view(n, L, D),
                                 mask.view(n, 1, L)).view(n, D)
    loss = (want * inp["dout"].double()).sum() + (x * inp["dz"].double()).sum()
    dx, dq, dkpre = torch.autograd.grad(loss, [x, q, kpre], allow_unused=True)
    scale = 1.0 / math.sqrt(D)
    ref = attn_pool_reference(inp["x"], None if tied else torch.tanh(kpre.detach()), inp["q"], mask, None, None, None, 0,
                              scale, not tied, dout=inp["dout"], dz=inp["dz"])
    _close(ref["out"], want.detach(), "out")
    _close(ref["dx"], dx, "dx")
    _close(ref["dq"], dq, "dq")
    if not tied:
        _close(ref["dk"], dkpre, "dk")
    assert ref["stats"] is None and torch.equal(ref["Z"], inp["x"].double())
    assert (ref["out"][0] == 0).all() and (ref["probs"][0] == 0).all() and (ref["probs"][mask == 0] == 0).all()
    # the per-sequence shares of dq that the GPU test bounds the accumulation's rounding with
    per = seq_pool_dq_per_seq(inp["x"], None if tied else torch.tanh(kpre.detach()), inp["q"], ref["probs"],
                              inp["dout"], scale)
    assert (per[0] == 0).all()
    assert (per.sum(0) - ref["dq"]).abs().max().item() <= 1e-12 * max(ref["dq"].abs().max().item(), 1e-300)


def test_seq_pool_reference_separate_key_without_tanh():
    """key_tanh = 0: dk is the plain gradient of the key rows."""
    L, D = 9, 6
    mask = pool_mask(L)
    n = mask.shape[0]
    inp = attn_pool_inputs(n, L, D, 3)
    x, key, q = (inp[k].double().requires_grad_() for k in ("x", "key", "q"))
    want = R.scaled_dp_attention(q.view(1, 1, D).expand(n, 1, D), key.view(n, L, D), x.view(n, L, D),
                                 mask.view(n, 1, L)).view(n, D)
    dx, dk, dq = torch.autograd.grad((want * inp["dout"].double()).sum(), [x, key, q])
    ref = attn_pool_reference(inp["x"], inp["key"], inp["q"], mask, None, None, None, 0, 1.0 / math.sqrt(D), False,
                              dout=inp["dout"])
    for name, got, w in (("out", ref["out"], want.detach()), ("dx", ref["dx"], dx), ("dk", ref["dk"], dk),
                         ("dq", ref["dq"], dq)):
        _close(got, w, name)
