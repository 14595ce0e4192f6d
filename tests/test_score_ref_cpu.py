"""The closed-form references of tests/score_util.py held against code that already exists, in float64
to 1e-12 of each tensor's largest value: score_reference against oracle.restatement.compute_score /
predict_fast and autograd of the same expression, nll_reference against restatement.nll_loss and
torch's nll_loss, xsoftmax_bwd_reference against autograd through restatement.xsoftmax, and
adam_reference against torch.optim.Adam on float64 tensors."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from newsrec_amd import _lib as L
from oracle import restatement as R
from score_util import (adam_reference, f32, nll_reference, score_reference, score_tolerance,
                        xsoftmax_bwd_reference)
from topk_util import scale32, tolerances

F64 = torch.float64
MODES = [L.SCORE_RAW, L.SCORE_LOG_SOFTMAX, L.SCORE_SIGMOID]
# H = 16 and 64: 1 / sqrt(H) is a power of two, the fp32 scale of the kernels IS the reference's;
# H = 150: the fp32 scale differs from 1 / sqrt(H) by its rounding, see _scale_ratio
SHAPES = [(3, 4, 64), (2, 65, 16), (7, 5, 150)]


def _close(got, want, name):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), "%s: err %.3e of max %.3e" % (name, err, scale)


def _scale_ratio(H):
    """score_reference multiplies by float32(1 / sqrt(H)) as the kernels do, restatement.compute_score
    divides by sqrt(H) in the tensors' dtype: the expression they are compared on carries this factor
    (exactly 1 when H is a power of 4)."""
    return float(scale32(H)) * math.sqrt(H)


def _head(s, mode):
    return s if mode == L.SCORE_RAW else F.log_softmax(s, 1) if mode == L.SCORE_LOG_SOFTMAX else torch.sigmoid(s)


def _inputs(B, C, H, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows or B * C, H, generator=g), torch.randn(B, H, generator=g),
            torch.randn(B, C, generator=g))


def test_scale_ratio_is_one_for_powers_of_four():
    assert _scale_ratio(16) == 1.0 and _scale_ratio(64) == 1.0 and _scale_ratio(1) == 1.0
    assert _scale_ratio(150) != 1.0 and abs(_scale_ratio(150) - 1.0) < 2.0 ** -24


@pytest.mark.parametrize("B,C,H", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_score_reference_vs_compute_score_and_autograd(mode, B, C, H):
    cdd, user, dl = _inputs(B, C, H, 7 * B + C + H)
    c64 = cdd.double().requires_grad_()
    u64 = user.double().requires_grad_()
    s = R.compute_score(c64.reshape(B, C, H), u64.reshape(B, 1, H)) * _scale_ratio(H)
    want = _head(s, mode)
    (want * dl.double()).sum().backward()
    ref = score_reference(cdd, user, B, C, mode, dlogits=dl)
    _close(ref["s"], s.detach(), "s")
    _close(ref["out"], want.detach(), "out")
    _close(ref["dcdd"], c64.grad, "dcdd")
    _close(ref["duser"], u64.grad, "duser")
    # the forward alone returns the same values and no gradients
    fwd = score_reference(cdd, user, B, C, mode)
    assert set(fwd) == {"s", "out"} and torch.equal(fwd["out"], ref["out"])


@pytest.mark.parametrize("B,C,H", [(3, 4, 64), (7, 5, 150)])
def test_score_reference_gather_vs_predict_fast(B, C, H):
    table, user, dl = _inputs(B, C, H, 3, rows=40)
    idx = (torch.arange(B * C) * 7 + 3) % 40
    idx[0], idx[-1] = 39, 0
    want = R.predict_fast(table.double(), idx.reshape(B, C), user.double().reshape(B, 1, H))
    ref = score_reference(table, user, B, C, L.SCORE_SIGMOID, idx=idx)
    # predict_fast is sigmoid(s / sqrt(H)); undo the sigmoid to carry the scale ratio across
    s_want = torch.logit(want) * _scale_ratio(H)
    _close(ref["s"], s_want, "s")
    _close(ref["out"], torch.sigmoid(s_want), "out")
    # the same as scoring the gathered rows in place, gradients included
    plain = score_reference(table[idx], user, B, C, L.SCORE_SIGMOID, dlogits=dl)
    got = score_reference(table, user, B, C, L.SCORE_SIGMOID, idx=idx, dlogits=dl)
    for k in plain:
        assert torch.equal(plain[k], got[k]), k
    assert not torch.equal(got["s"], score_reference(table, user, B, C, L.SCORE_SIGMOID)["s"])


def test_score_tolerance_is_topk_bound_on_the_diagonal():
    """score_tolerance(b, c) is topk_util.tolerances of (user b, row (b, c)): one shared formula."""
    B, C, H = 3, 5, 150
    cdd, user, _ = _inputs(B, C, H, 11)
    tol = score_tolerance(cdd, user, B, C)
    full = tolerances(cdd.numpy(), user.numpy())                  # [B, B*C]
    for b in range(B):
        np.testing.assert_allclose(tol[b].numpy(), full[b, b * C:(b + 1) * C], rtol=1e-14, atol=0)
    idx = torch.arange(B * C).flip(0)
    np.testing.assert_allclose(score_tolerance(cdd, user, B, C, idx=idx).numpy(),
                               score_tolerance(cdd[idx], user, B, C).numpy(), rtol=0, atol=0)
    assert (tol > 0).all()


@pytest.mark.parametrize("B,C,H,labels", [(3, 65, 16, [64, -100, 0]), (2, 130, 64, [-100, 129]), (4, 5, 64, [1, 2, 3, 4])])
def test_nll_reference_vs_torch(B, C, H, labels):
    cdd, user, _ = _inputs(B, C, H, B + C)
    label = torch.tensor(labels)
    c64, u64 = cdd.double().requires_grad_(), user.double().requires_grad_()
    logits = F.log_softmax(R.compute_score(c64.reshape(B, C, H), u64.reshape(B, 1, H)), 1)
    want = R.nll_loss(logits, label)
    (2.5 * want).backward()
    ref = nll_reference(cdd, user, label, B, C, dloss=2.5)
    _close(ref["logits"], logits.detach(), "logits")
    _close(ref["loss"], want.detach(), "loss")
    _close(ref["loss"], F.nll_loss(logits.detach(), label, ignore_index=-100, reduction="mean"), "loss (torch)")
    _close(ref["dcdd"], c64.grad, "dcdd")
    _close(ref["duser"], u64.grad, "duser")
    for b, y in enumerate(labels):
        if y == -100:
            assert (ref["dcdd"][b * C:(b + 1) * C] == 0).all() and (ref["duser"][b] == 0).all()


def test_nll_reference_all_ignored_is_nan():
    cdd, user, _ = _inputs(2, 3, 4, 0)
    ref = nll_reference(cdd, user, torch.tensor([-100, -100]), 2, 3)
    assert torch.isnan(ref["loss"]) and (ref["dcdd"] == 0).all()
    assert torch.isnan(F.nll_loss(ref["logits"], torch.tensor([-100, -100])))


@pytest.mark.parametrize("rows,cols", [(5, 2), (4, 64), (7, 65), (3, 130)])
def test_xsoftmax_bwd_reference_vs_autograd(rows, cols):
    g = torch.Generator().manual_seed(rows * cols)
    x = torch.randn(rows, cols, generator=g, dtype=F64).requires_grad_()
    mask = torch.rand(rows, cols, generator=g) < 0.6
    mask[0] = False                                              # a fully masked row
    mask[1] = True
    dy = torch.randn(rows, cols, generator=g, dtype=F64)
    y = R.xsoftmax(x, mask)
    y.backward(dy)
    got = xsoftmax_bwd_reference(y.detach(), dy)
    _close(got, x.grad, "dx")
    assert (got[0] == 0).all() and (got[~mask] == 0).all() and got[1].abs().max() > 0


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_reference_vs_torch_adam(wd):
    g = torch.Generator().manual_seed(5)
    n = 1001
    hp = dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), wd=f32(wd))
    gscale = 1.0 / 128
    p0 = torch.randn(n, generator=g, dtype=F64)
    ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g, dtype=F64) * 10.0 ** -(step - 1)
        ref.grad = grad * gscale
        opt.step()
        p, m, v = adam_reference(p, grad, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], gscale, step)
        st = opt.state[ref]
        _close(p, ref.detach(), "p, step %d" % step)
        _close(m, st["exp_avg"], "m, step %d" % step)
        _close(v, st["exp_avg_sq"], "v, step %d" % step)
    assert (p - p0).abs().max() > 1e-3                           # three steps of about lr each were taken


def test_f32_hyperparameters_make_one_minus_beta_exact():
    """1 - beta of the fp32-rounded betas is the same number in fp32 and in double (adam_reference's
    premise: the kernel's 1.f - b1 is the reference's 1.0 - b1)."""
    for b in (0.9, 0.999):
        assert float(np.float32(1.0) - np.float32(b)) == 1.0 - f32(b)
