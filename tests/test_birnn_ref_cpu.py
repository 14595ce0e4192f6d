"""tests/birnn_util.birnn_reference -- the yardstick of the nr_birnn_* kernel tests -- against the
reference model's own RNN_Encoder (tests/golden/rnn_news.npz, float64) and against
torch.nn.LSTM(bidirectional=True) fed the same weights."""
import os

import numpy as np
import pytest
import torch

from birnn_util import birnn_inputs, birnn_reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnn_news.npz")
NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _close(got, want, name, tol=1e-12):
    err = (got - want).abs().max().item()
    assert got.shape == want.shape and err <= tol, "%s: max error %.3e > %.0e" % (name, err, tol)


def test_reference_reproduces_the_golden():
    z = _golden()
    x = z["x"]
    B, N, L, E = x.shape
    H = z["rnn.weight_hh_l0"].shape[1]
    X = x.reshape(B * N * L, E)
    w_cat = torch.cat([z["rnn.weight_ih_l0"], z["rnn.weight_ih_l0_reverse"]])
    b_cat = torch.cat([z["rnn.bias_ih_l0"], z["rnn.bias_ih_l0_reverse"]])
    w_hh = torch.stack([z["rnn.weight_hh_l0"], z["rnn.weight_hh_l0_reverse"]])
    b_hh = torch.stack([z["rnn.bias_hh_l0"], z["rnn.bias_hh_l0_reverse"]])
    out = birnn_reference(X @ w_cat.t() + b_cat, w_hh, b_hh, B * N, L, dnews=z["b"].reshape(B * N, H),
                          dtok=z["a"].reshape(B * N * L, H))
    _close(out["tok"].view(B, N, L, H), z["tok"], "tok")
    _close(out["news"].view(B, N, H), z["news"], "news")
    dg = out["dg"]
    _close((dg @ w_cat).view_as(x), z["grad.x"], "grad x")
    dw = dg.t() @ X
    db = dg.sum(0)
    for d, sfx in enumerate(("", "_reverse")):
        sl = slice(d * 4 * H, (d + 1) * 4 * H)
        _close(dw[sl], z["grad.rnn.weight_ih_l0" + sfx], "dW_ih" + sfx)
        _close(db[sl], z["grad.rnn.bias_ih_l0" + sfx], "db_ih" + sfx)
        _close(db[sl], z["grad.rnn.bias_hh_l0" + sfx], "db_hh" + sfx)
        _close(out["dw_hh"][d], z["grad.rnn.weight_hh_l0" + sfx], "dW_hh" + sfx)


@pytest.mark.parametrize("nseq,L,E,H", [(3, 1, 4, 5), (5, 4, 6, 3), (17, 3, 7, 8)])
def test_reference_equals_torch_lstm(nseq, L, E, H):
    torch.manual_seed(nseq + L)
    rnn = torch.nn.LSTM(E, H, batch_first=True, bidirectional=True).double()
    inp = birnn_inputs(nseq, L, H, 5)
    x = torch.randn(nseq, L, E, dtype=torch.float64, requires_grad=True)
    out, (hn, _) = rnn(x)
    tok = out.view(nseq, L, 2, H).mean(-2)
    news = hn.mean(0)
    dnews, dtok = inp["dnews"].double(), inp["dtok"].double()
    ((tok.reshape(nseq * L, H) * dtok).sum() + (news * dnews).sum()).backward()
    P = {n: p.detach() for n, p in rnn.named_parameters()}
    w_cat = torch.cat([P["weight_ih_l0"], P["weight_ih_l0_reverse"]])
    b_cat = torch.cat([P["bias_ih_l0"], P["bias_ih_l0_reverse"]])
    X = x.detach().reshape(nseq * L, E)
    ref = birnn_reference(X @ w_cat.t() + b_cat, torch.stack([P["weight_hh_l0"], P["weight_hh_l0_reverse"]]),
                          torch.stack([P["bias_hh_l0"], P["bias_hh_l0_reverse"]]), nseq, L, dnews=dnews, dtok=dtok)
    _close(ref["tok"], tok.detach().reshape(nseq * L, H), "tok")
    _close(ref["news"], news.detach(), "news")
    _close(ref["hlast"], hn.detach(), "hlast")
    _close((ref["dg"] @ w_cat).view_as(x), x.grad, "grad x")
    _close(ref["dw_hh"][0], rnn.weight_hh_l0.grad, "dW_hh")
    _close(ref["dw_hh"][1], rnn.weight_hh_l0_reverse.grad, "dW_hh reverse")
    _close(ref["dg"].sum(0)[:4 * H], rnn.bias_hh_l0.grad, "db_hh")
    if L == 1:
        assert (ref["dw_hh"] == 0).all() and (ref["hprev"] == 0).all()


def test_float32_reference_and_single_gradients():
    """The float32 evaluation (the e32 of the kernel tests' bar) stays near float64, and dnews-only /
    dtok-only gradients add up to the joint one."""
    inp = birnn_inputs(5, 4, 6, 9)
    a = (inp["gx"], inp["w_hh"], inp["b_hh"], 5, 4)
    both = birnn_reference(*a, dnews=inp["dnews"], dtok=inp["dtok"])
    only_n = birnn_reference(*a, dnews=inp["dnews"])
    only_t = birnn_reference(*a, dtok=inp["dtok"])
    _close(only_n["dg"] + only_t["dg"], both["dg"], "dg", tol=1e-13)
    r32 = birnn_reference(*a, dnews=inp["dnews"], dtok=inp["dtok"], dtype=torch.float32)
    for k in ("news", "tok", "dg", "dw_hh"):
        assert r32[k].dtype == torch.float32
        assert (r32[k].double() - both[k]).abs().max().item() <= 1e-4 * both[k].abs().max().item(), k
