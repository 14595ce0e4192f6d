"""The float64 reference of the recurrent kernels (tests/rnn_util.py) against torch.nn.LSTM /
torch.nn.GRU, and the return codes of nr_rnn_fwd / nr_rnn_bwd for invalid and empty arguments.

The reference speaks the kernels' ABI: it takes the input projections gx and returns the gate
gradients dgi / dgh, from which the weight, bias and input gradients follow as RNNUserFn.backward
forms them (dW_ih = dgi^T x, dW_hh = dgh^T hprev, db = column sums, dx = dgi W_ih).  torch.nn runs
the same recurrence from x over pack_padded_sequence, so agreement is float64 rounding.

The argument checks of both entries return before any HIP call, so they run through ctypes on a
machine without a GPU, on a host buffer that no case ever dereferences."""
import ctypes
import os

import pytest
import torch

from newsrec_amd import _lib as L
from rnn_util import gates_per_cell, rnn_reference

B, N, H = 5, 9, 7
LENS = (1, 9, 4, 8, 2)
RTOL = 1e-12          # of each tensor's max: float64 rounding over 9 steps of width 7


def _close(got, want, name):
    scale = want.abs().max().item()
    assert scale > 0, name
    err = (got - want).abs().max().item()
    assert err <= RTOL * scale, "%s: %.3e of max %.3e" % (name, err, scale)


@pytest.mark.parametrize("form", ["packed", "packed_flipped", "packed_h0", "packed_flipped_h0", "lstur"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_reference_matches_torch_nn(cell, form):
    """packed: RNN_User_Encoder (RNN.py:50-73; flipped = descend_history, RNN.py:61-66: flip, then
    pack); *_h0: the same with an initial state; lstur: no mask, flipped, h0 given, c0 = 0
    (RNN.py:88-104; the GRU runs that form too, the ABI allows it)."""
    if form == "lstur":
        lens, reverse, with_h0 = (N,) * B, True, True
    else:
        lens, reverse, with_h0 = LENS, "flipped" in form, form.endswith("h0")
    G = gates_per_cell(cell)
    g = torch.Generator().manual_seed(11 + G + 2 * reverse + 4 * with_h0)
    rnn = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(H, H, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (1.5 / H ** 0.5 if p.dim() == 2 else 0.1))
    x = torch.randn(B, N, H, generator=g, dtype=torch.float64, requires_grad=True)
    h0 = (torch.randn(B, H, generator=g, dtype=torch.float64) * 0.3).requires_grad_() if with_h0 else None
    dhout = torch.randn(B, H, generator=g, dtype=torch.float64)

    xin = x.flip(1) if reverse else x
    if form != "lstur":
        xin = torch.nn.utils.rnn.pack_padded_sequence(xin, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    hx = None
    if with_h0:
        hx = (h0[None], torch.zeros(1, B, H, dtype=torch.float64)) if cell == "lstm" else h0[None]
    _, hn = rnn(xin, hx)
    want_h = (hn[0] if cell == "lstm" else hn)[0]
    (want_h * dhout).sum().backward()

    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))
    x2 = x.detach().reshape(B * N, H)
    gx = x2 @ w_ih.t() + b_ih
    r = rnn_reference(cell, gx, w_hh, b_hh, h0, lens, reverse, dhout=dhout)
    _close(r["hout"], want_h.detach(), "hout")
    _close((r["dgi"] @ w_ih).view(B, N, H), x.grad, "dx")
    _close(r["dgi"].t() @ x2, rnn.weight_ih_l0.grad, "dW_ih")
    _close(r["dgh"].t() @ r["hprev"], rnn.weight_hh_l0.grad, "dW_hh")
    _close(r["dgi"].sum(0), rnn.bias_ih_l0.grad, "db_ih")
    _close(r["dgh"].sum(0), rnn.bias_hh_l0.grad, "db_hh")
    if with_h0:
        _close(r["dh0"], h0.grad, "dh0")
    # what the kernels promise about the steps that do not run
    for b, n in enumerate(lens):
        rows = [b * N + (N - 1 - t if reverse else t) for t in range(n, N)]
        for k in ("gates", "hprev", "cprev", "dgi", "dgh"):
            if r[k] is not None:
                assert (r[k][rows] == 0).all(), k


def test_reference_len0_and_no_bias():
    """len == 0: hout = h0 and dh0 = dhout; b_hh = None equals a zero bias."""
    g = torch.Generator().manual_seed(5)
    for cell in ("lstm", "gru"):
        G = gates_per_cell(cell)
        gx = torch.randn(3 * 4, G * H, generator=g, dtype=torch.float64)
        w = torch.randn(G * H, H, generator=g, dtype=torch.float64) * 0.5
        h0 = torch.randn(3, H, generator=g, dtype=torch.float64)
        dh = torch.randn(3, H, generator=g, dtype=torch.float64)
        a = rnn_reference(cell, gx, w, None, h0, (0, 4, 2), True, dhout=dh)
        z = rnn_reference(cell, gx, w, torch.zeros(G * H, dtype=torch.float64), h0, (0, 4, 2), True, dhout=dh)
        assert torch.equal(a["hout"][0], h0[0]) and torch.equal(a["dh0"][0], dh[0])
        for k in a:
            if a[k] is not None:
                assert torch.equal(a[k], z[k]), k
        none = rnn_reference(cell, gx, w, None, None, (0, 4, 2), False, dhout=dh)
        assert (none["hout"][0] == 0).all() and torch.equal(none["dh0"][0], dh[0])


# ---------------------------------------------------------------------- return codes

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
_P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host memory, never read or written


def _fwd(**kw):
    a = dict(cell=L.CELL_LSTM, gx=_P, ldgx=16, whh_t=_P, bhh=_P, h0=_P, ldh0=4, h0_idx=_P, mask=_P, mask_dtype=0,
             reverse=0, B=2, N=3, H=4, gates=_P, hprev=_P, cprev=_P, hout=_P, ldho=4)
    a.update(kw)
    return L.load().nr_rnn_fwd(a["cell"], a["gx"], a["ldgx"], a["whh_t"], a["bhh"], a["h0"], a["ldh0"], a["h0_idx"],
                               a["mask"], a["mask_dtype"], a["reverse"], a["B"], a["N"], a["H"], a["gates"],
                               a["hprev"], a["cprev"], a["hout"], a["ldho"], None)


def _bwd(**kw):
    a = dict(cell=L.CELL_LSTM, whh=_P, gates=_P, hprev=_P, cprev=_P, mask=_P, mask_dtype=0, reverse=0, B=2, N=3, H=4,
             dhout=_P, lddho=4, dgi=_P, dgh=_P, lddg=16, dh0=_P, lddh0=4)
    a.update(kw)
    return L.load().nr_rnn_bwd(a["cell"], a["whh"], a["gates"], a["hprev"], a["cprev"], a["mask"], a["mask_dtype"],
                               a["reverse"], a["B"], a["N"], a["H"], a["dhout"], a["lddho"], a["dgi"], a["dgh"],
                               a["lddg"], a["dh0"], a["lddh0"], None)


# every case carries B = 0 unless it sets B itself, so that a check that failed to fire would return 0
# (and fail the case) rather than launch a kernel on host pointers
BAD_VALUES = [("cell=2", dict(cell=2)), ("cell=-1", dict(cell=-1)), ("B=-1", dict(B=-1)), ("N=0", dict(N=0)),
              ("N=-3", dict(N=-3)), ("H=0", dict(H=0)), ("H=-1", dict(H=-1)), ("H=513", dict(H=513))]
FWD_NULLS = [(c, p) for c in ("lstm", "gru") for p in ("gx", "whh_t", "gates", "hprev", "hout")] + [("lstm", "cprev")]
BWD_NULLS = ([(c, p) for c in ("lstm", "gru") for p in ("whh", "gates", "hprev", "dhout", "dgi")]
             + [("lstm", "cprev"), ("gru", "dgh")])
_CELL = {"lstm": L.CELL_LSTM, "gru": L.CELL_GRU}


@needs_lib
@pytest.mark.parametrize("entry", ["fwd", "bwd"])
@pytest.mark.parametrize("name,kw", BAD_VALUES, ids=[c[0] for c in BAD_VALUES])
def test_bad_value_codes(entry, name, kw):
    assert (_fwd if entry == "fwd" else _bwd)(**dict(dict(B=0), **kw)) == -1000


@needs_lib
@pytest.mark.parametrize("cell,arg", FWD_NULLS, ids=["%s-%s" % c for c in FWD_NULLS])
def test_fwd_null_pointer_codes(cell, arg):
    assert _fwd(cell=_CELL[cell], B=0, **{arg: None}) == -1001


@needs_lib
@pytest.mark.parametrize("cell,arg", BWD_NULLS, ids=["%s-%s" % c for c in BWD_NULLS])
def test_bwd_null_pointer_codes(cell, arg):
    assert _bwd(cell=_CELL[cell], B=0, **{arg: None}) == -1001


@needs_lib
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_empty_batch_and_optional_pointers(cell):
    """B == 0 is valid and launches nothing; the optional pointers may be NULL: bhh, h0, h0_idx, mask
    (and cprev for the GRU) in the forward, mask, dh0 (and dgh for the LSTM, cprev for the GRU) in
    the backward.  A bad value is reported before a NULL pointer."""
    c = _CELL[cell]
    assert _fwd(cell=c, B=0) == 0 and _bwd(cell=c, B=0) == 0
    assert _fwd(cell=c, B=0, H=512) == 0 and _bwd(cell=c, B=0, H=512) == 0
    assert _fwd(cell=c, B=0, bhh=None, h0=None, h0_idx=None, mask=None) == 0
    assert _bwd(cell=c, B=0, mask=None, dh0=None) == 0
    if cell == "gru":
        assert _fwd(cell=c, B=0, cprev=None) == 0 and _bwd(cell=c, B=0, cprev=None) == 0
    else:
        assert _bwd(cell=c, B=0, dgh=None) == 0
    assert _fwd(cell=c, B=0, H=513, gx=None) == -1000 and _bwd(cell=c, B=0, N=0, dgi=None) == -1000
