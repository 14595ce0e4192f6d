"""The references of tests/synth_util.py held to independent formulations, on the CPU:

  * synth_reference equals torch.softmax / relu, and its da2 / da1 / dhv / weight-gradient sums equal autograd
    through them;
  * synth_reference and the model composition's attention block reproduce the reference module's golden
    (tests/golden/synthesizer.npz: the output to 1e-12, every gradient to 1e-10 of its scale);
  * a gate passed in replaces the forward's own;
  * at the fixture of the GPU model tests the float32 and float64 compositions take identical ReLU gates and
    every pre-activation is >= 1e-4 from zero (fp32 forward error there is ~1e-6), in eval() and with the
    replayed hidden dropout: a gradient mismatch in the model tests cannot be excused as a gate flip."""
import os

import numpy as np
import pytest
import torch

from synth_util import (FIX, FIX_TORCH_SEED, STATE_NAMES, fixture, fixture_shapes, synth_attention_block,
                        synth_bert_model, synth_inputs, synth_reference)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthesizer.npz")


def _golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("L,D", [(5, 8), (30, 152), (1, 4)])
def test_core_reference_vs_autograd(L, D):
    nseq = 4
    inp = synth_inputs(nseq, L, D, 7)
    ref = synth_reference(inp["hv"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], nseq, L, inp["dctx"])
    hv, w1, b1, w2, b2 = (inp[n].double().requires_grad_() for n in ("hv", "w1", "b1", "w2", "b2"))
    a1 = torch.relu(torch.addmm(b1, hv, w1.t()))
    P = torch.softmax(torch.addmm(b2, a1, w2.t()), -1).view(nseq, L, L)
    ctx = torch.bmm(P, hv.view(nseq, L, D)).reshape(nseq * L, D)
    torch.testing.assert_close(ref["a1"], a1.detach(), rtol=0, atol=1e-14)
    torch.testing.assert_close(ref["probs"], P.detach(), rtol=0, atol=1e-14)
    torch.testing.assert_close(ref["ctx"], ctx.detach(), rtol=0, atol=1e-13)
    assert (ref["probs"].sum(-1) - 1).abs().max() < 1e-14
    (ctx * inp["dctx"].double()).sum().backward()
    for n, t in (("dhv", hv), ("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2)):
        torch.testing.assert_close(ref[n], t.grad, rtol=0, atol=1e-12, msg=lambda s, n=n: n + ": " + s)


def test_a_gate_passed_in_replaces_the_forwards_own():
    nseq, L, D = 2, 5, 8
    inp = synth_inputs(nseq, L, D, 9)
    args = (inp["hv"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], nseq, L, inp["dctx"])
    own = synth_reference(*args)
    same = synth_reference(*args, gate=own["a1"] > 0)
    for n in ("da1", "da2", "dhv"):
        assert torch.equal(own[n], same[n]), n
    closed = synth_reference(*args, gate=torch.zeros(nseq * L, L, dtype=torch.bool))
    assert (closed["da1"] == 0).all() and torch.equal(closed["da2"], own["da2"])
    assert (closed["dhv"] - own["dhv"]).abs().max() > 0


def test_reference_and_block_reproduce_the_golden():
    z = _golden()
    assert set(STATE_NAMES) <= set(z)
    n, L, H = z["x"].shape
    # the contract's formulas on hv = value_fn(x), chained to x and value_fn by hand
    wv, bv = z["value_fn.weight"], z["value_fn.bias"]
    x2 = z["x"].reshape(n * L, H)
    hv = x2 @ wv.t() + bv
    ref = synth_reference(hv, z["dense.0.weight"], z["dense.0.bias"], z["dense.2.weight"], z["dense.2.bias"], n, L,
                          z["w"].reshape(n * L, H))
    torch.testing.assert_close(ref["ctx"].view(n, L, H), z["out"], rtol=0, atol=1e-12)
    mine = {"x": (ref["dhv"] @ wv).view(n, L, H), "value_fn.weight": ref["dhv"].t() @ x2,
            "value_fn.bias": ref["dhv"].sum(0), "dense.0.weight": ref["dw1"], "dense.0.bias": ref["db1"],
            "dense.2.weight": ref["dw2"], "dense.2.bias": ref["db2"]}
    for name, got in mine.items():
        want = z["grad." + name]
        torch.testing.assert_close(got, want, rtol=0, atol=1e-10 * want.abs().max().item(),
                                   msg=lambda s, name=name: name + ": " + s)
    # the model composition's block under autograd
    P = {k: z[k].clone().requires_grad_() for k in STATE_NAMES}
    x = z["x"].clone().requires_grad_()
    out = synth_attention_block(P, x, "")
    torch.testing.assert_close(out, z["out"], rtol=0, atol=1e-12)
    (out * z["w"]).sum().backward()
    for name, t in [("x", x)] + list(P.items()):
        want = z["grad." + name]
        torch.testing.assert_close(t.grad, want, rtol=0, atol=1e-10 * want.abs().max().item(),
                                   msg=lambda s, name=name: name + ": " + s)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "dropout"])
def test_fixture_keeps_its_relu_gates_away_from_zero(train):
    from oracle import restatement as R
    P, ids, _, _, _ = fixture()
    assert [tuple(P[n].shape) for n, _ in fixture_shapes()] == [s for _, s in fixture_shapes()]
    T = FIX["nseq"] * FIX["L"]
    drop = (R.BertDropout(FIX_TORCH_SEED, 0, T, FIX["hidden"], FIX["layers"], FIX["heads"], FIX["p_hidden"], 0.0)
            if train else None)
    z = {}
    for dt in (torch.float64, torch.float32):
        trace = []
        with torch.no_grad():
            synth_bert_model({k: v.to(dt) for k, v in P.items()}, ids, drop=drop, trace=trace)
        assert len(trace) == FIX["layers"]
        z[dt] = torch.cat(trace)
    assert torch.equal(z[torch.float64] > 0, z[torch.float32] > 0), "a ReLU gate flips between float32 and float64"
    margin = z[torch.float64].abs().min().item()
    fwd_err = (z[torch.float32].double() - z[torch.float64]).abs().max().item()
    print("fixture %s: min |z1| %.3e, float32 z1 error %.3e" % ("train" if train else "eval", margin, fwd_err))
    assert margin >= 1e-4
    assert fwd_err <= 1e-5
    frac = (z[torch.float64] > 0).double().mean().item()
    assert 0.2 < frac < 0.8, "the gates are not a mix of open and closed (%.2f open)" % frac
