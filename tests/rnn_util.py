"""A plain-torch reference of the recurrent kernels' ABI (nr_rnn_fwd / nr_rnn_bwd) and the seeded
inputs of their tests.

rnn_reference() takes what nr_rnn_fwd takes -- the input projections gx of all steps, W_hh, b_hh,
the h0 row of every sequence and the lengths -- runs the recurrence step by step under autograd in
the dtype asked for and returns what the kernels save and write: hout, gates, hprev, cprev, and,
given dhout, the gate gradients dgi / dgh and dh0.  tests/test_rnn_cpu.py holds it against
torch.nn.LSTM / torch.nn.GRU."""
import torch
import torch.nn.functional as F


def gates_per_cell(cell):
    return 4 if cell == "lstm" else 3


def rnn_reference(cell, gx, w_hh, b_hh, h0, lens, reverse, dhout=None, dtype=torch.float64):
    """cell "lstm" | "gru"; gx [B*N, G*H]; w_hh [G*H, H]; b_hh [G*H] or None; h0 [B, H] (row b is
    sequence b's) or None; lens: B ints in 0..N; reverse: step t reads row N-1-t.  Only steps
    t < lens[b] run; a sequence of length 0 outputs its h0.

    -> dict of detached ``dtype`` tensors
         hout [B, H]
         gates [B*N, 4H]   LSTM i,f,g,o activated; GRU r,z,n activated, then W_hn h + b_hn
         hprev, cprev [B*N, H]   h / c before the step (cprev None for the GRU)
       rows of steps that do not run are zero; with dhout [B, H] also
         dgi [B*N, G*H]  d/d gx
         dgh [B*N, G*H]  d/d (h W_hh^T + b_hh): the gradient of a zero leaf added to the recurrent
                         pre-activations before the nonlinearities (for the GRU's n gate inside r * (.))
         dh0 [B, H]      d/d h0 (of a zero h0 when h0 is None)"""
    G = gates_per_cell(cell)
    GH, H = w_hh.shape
    assert GH == G * H
    B = len(lens)
    N = gx.shape[0] // B
    assert gx.shape == (B * N, GH) and all(0 <= int(n) <= N for n in lens)
    gx = gx.detach().to(dtype).clone().requires_grad_()
    eh = torch.zeros(B * N, GH, dtype=dtype, requires_grad=True)
    w = w_hh.detach().to(dtype)
    bias = b_hh.detach().to(dtype) if b_hh is not None else None
    h0 = (h0.detach().to(dtype).clone() if h0 is not None else torch.zeros(B, H, dtype=dtype)).requires_grad_()
    gates = torch.zeros(B * N, 4 * H, dtype=dtype)
    hprev = torch.zeros(B * N, H, dtype=dtype)
    cprev = torch.zeros(B * N, H, dtype=dtype) if cell == "lstm" else None
    hout = []
    for b in range(B):
        h = h0[b]
        c = torch.zeros(H, dtype=dtype)
        for t in range(int(lens[b])):
            row = b * N + (N - 1 - t if reverse else t)
            rec = F.linear(h, w, bias) + eh[row]
            hprev[row] = h.detach()
            if cell == "lstm":
                i, f, g, o = (gx[row] + rec).chunk(4)
                i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                cprev[row] = c.detach()
                c = f * c + i * g
                h = o * torch.tanh(c)
                gates[row] = torch.cat([i, f, g, o]).detach()
            else:
                xr, xz, xn = gx[row].chunk(3)
                hr, hz, hn = rec.chunk(3)
                r = torch.sigmoid(xr + hr)
                z = torch.sigmoid(xz + hz)
                n = torch.tanh(xn + r * hn)
                gates[row] = torch.cat([r, z, n, hn]).detach()
                h = (1 - z) * n + z * h
        hout.append(h)
    hout = torch.stack(hout)
    out = {"hout": hout.detach(), "gates": gates, "hprev": hprev, "cprev": cprev}
    if dhout is not None:
        dgi, dgh, dh0 = torch.autograd.grad((hout * dhout.detach().to(dtype)).sum(), [gx, eh, h0])
        out.update(dgi=dgi, dgh=dgh, dh0=dh0)
    return out


def rnn_inputs(cell, B, N, H, seed, table_rows=None):
    """Seeded float32 inputs at the scales of tests/golden/params.py: gx, dhout standard normal,
    w_hh 1.5 / sqrt(H), b_hh 0.1, h0 0.3.  h0 is [B, H], or a [table_rows, H] table to be indexed."""
    G = gates_per_cell(cell)
    g = torch.Generator().manual_seed(seed)
    return {
        "gx": torch.randn(B * N, G * H, generator=g),
        "w_hh": torch.randn(G * H, H, generator=g) * (1.5 / H ** 0.5),
        "b_hh": torch.randn(G * H, generator=g) * 0.1,
        "h0": torch.randn(table_rows or B, H, generator=g) * 0.3,
        "dhout": torch.randn(B, H, generator=g),
    }
