"""The references of tests/sha_attn_util.py held to independent formulations, on the CPU:

  * the float64 composition of the whole encoder reproduces the reference model's golden
    (tests/golden/transformer_news.npz: tok and news to 1e-12, every gradient to 1e-10 of its scale);
  * the core reference equals torch.softmax over masked_fill(-inf) with zeros filled in, and its dq / dk /
    dv equal autograd through that, with and without a dropout keep mask;
  * a title without a token gives ctx == 0 and dq == dk == dv == 0 exactly;
  * the cap check: for every kernel-level case of the GPU test the project's bar
    32 e32 + 32 * 2^-24 * max|ref64| is at most 1e-4 * max|ref64| for every tensor, so the cap of
    tests/test_transformer_news_gpu.py leaves no case out."""
import math
import os

import numpy as np
import pytest
import torch

from sha_attn_util import (KERNEL_CASES, TENSORS, bar_of, case_references, encoder_reference, sha_inputs, sha_keep,
                           sha_mask, sha_reference)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer_news.npz")


def _golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_composition_reproduces_the_golden():
    z = _golden()
    names = [k for k in z if k.startswith(("project.", "bert.", "query_words"))]
    assert len(names) == 19
    P = {k: z[k].clone().requires_grad_() for k in names}
    x = z["x"].clone().requires_grad_()
    tok, news = encoder_reference(P, x, z["mask"])
    torch.testing.assert_close(tok, z["tok"], rtol=0, atol=1e-12)
    torch.testing.assert_close(news, z["news"], rtol=0, atol=1e-12)
    assert (news[1, 1] == 0).all(), "the title without a token must pool to exact zeros"
    assert torch.isfinite(tok[1, 1]).all() and (tok[1, 1] != 0).any()
    ((tok * z["a"]).sum() + (news * z["b"]).sum()).backward()
    for n, t in [("x", x)] + list(P.items()):
        ref = z["grad." + n]
        torch.testing.assert_close(t.grad, ref, rtol=0, atol=1e-10 * ref.abs().max().item(), msg=lambda s, n=n: n + ": " + s)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L,D", [(5, 8), (30, 152), (1, 4)])
def test_core_reference_vs_autograd(L, D, p):
    nseq = 4
    inp = sha_inputs(nseq, L, D, 7)
    mask = sha_mask(nseq, L)
    keep = sha_keep(3, 11, nseq, L, p) if p > 0 else None
    scale = 1.0 / math.sqrt(D)
    ref = sha_reference(inp["q"], inp["k"], inp["v"], mask, scale, keep, p, inp["dctx"])
    q, k, v = (inp[n].double().view(nseq, L, D).requires_grad_() for n in ("q", "k", "v"))
    m = (mask != 0)[:, None, :]
    P = torch.softmax((torch.matmul(q, k.transpose(1, 2)) * scale).masked_fill(~m, -math.inf), -1)
    P = torch.where(m, P, torch.zeros_like(P))
    Pd = P if keep is None else P * keep.double() / (1 - p)
    ctx = torch.matmul(Pd, v).reshape(nseq * L, D)
    torch.testing.assert_close(ref["probs"], P.detach(), rtol=0, atol=1e-14)
    torch.testing.assert_close(ref["ctx"], ctx.detach(), rtol=0, atol=1e-13)
    assert (ref["probs"][(mask == 0)[:, None, :].expand(nseq, L, L)] == 0).all()
    (ctx * inp["dctx"].double()).sum().backward()
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        torch.testing.assert_close(ref[n], t.grad.reshape(nseq * L, D), rtol=0, atol=1e-12, msg=lambda s, n=n: n + ": " + s)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_title_without_a_token_is_exactly_zero(dtype):
    nseq, L, D = 4, 5, 8
    inp = sha_inputs(nseq, L, D, 9)
    mask = sha_mask(nseq, L)
    assert (mask[2] == 0).all()
    keep = sha_keep(3, 11, nseq, L, 0.1)
    ref = sha_reference(inp["q"], inp["k"], inp["v"], mask, 1.0 / math.sqrt(D), keep, 0.1, inp["dctx"], dtype=dtype)
    rows = slice(2 * L, 3 * L)
    assert (ref["probs"][2] == 0).all()
    for n in ("ctx", "dq", "dk", "dv"):
        assert (ref[n][rows] == 0).all(), n
        assert ref[n].abs().max() > 0, n


@pytest.mark.parametrize("nseq,L,D,p", KERNEL_CASES, ids=["n%d-L%d-D%d-p%g" % c for c in KERNEL_CASES])
def test_cap_leaves_no_case_out(nseq, L, D, p):
    _, _, _, ref = case_references(nseq, L, D, p)
    for name in TENSORS:
        bar, e32, scale = bar_of(ref, name)
        if scale == 0:      # L = 1: dS = P (g - g P) = 0, so dq and dk are exact zeros
            assert L == 1 and name in ("dq", "dk")
            assert (ref[torch.float32][name] == 0).all()
            continue
        assert bar <= 1e-4 * scale, "%s: bar %.3e (e32 %.3e) exceeds 1e-4 of max %.3e" % (name, bar, e32, scale)
