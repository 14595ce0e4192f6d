"""A plain-torch reference of the bidirectional-LSTM kernels' ABI (nr_birnn_fwd / nr_birnn_bwd) and the
seeded inputs of their tests.

birnn_reference() takes what nr_birnn_fwd takes -- the input projections gx of all steps and both
directions, the two W_hh and b_hh -- runs the two recurrences step by step under autograd in the
dtype asked for (all L steps, h0 = c0 = 0, no mask) and returns what the kernels write and save: news,
tok, the activated gates, h_{t-1} / c_{t-1} per step, each direction's final state and, given dnews /
dtok, the gate gradients dg and the dW_hh products dg_d^T hprev_d.  tests/test_birnn_ref_cpu.py holds it
against torch.nn.LSTM(bidirectional=True) and the reference model's golden."""
import torch


def birnn_reference(gx, w_hh, b_hh, nseq, L, dnews=None, dtok=None, dtype=torch.float64):
    """gx [nseq*L, 8H] (columns [0,4H) forward i,f,g,o, [4H,8H) reverse); w_hh [2, 4H, H]; b_hh [2, 4H]
    or None; dnews [nseq, H] / dtok [nseq*L, H] or None.

    -> dict of detached ``dtype`` tensors
         news [nseq, H], tok [nseq*L, H]
         gates [2, nseq*L, 4H]  i,f,g,o activated, per direction, at the token the step consumed
         hprev, cprev [2, nseq*L, H]   h / c before that step
         hlast [2, nseq, H]     each direction's final h
       with dnews and / or dtok also
         dg [nseq*L, 8H]        d/d gx of sum(news * dnews) + sum(tok * dtok)
         dw_hh [2, 4H, H]       dg_d^T hprev_d, the recurrent weight gradient"""
    H = w_hh.shape[2]
    T = nseq * L
    assert gx.shape == (T, 8 * H) and w_hh.shape == (2, 4 * H, H)
    gx = gx.detach().to(dtype).clone().requires_grad_()
    w = w_hh.detach().to(dtype)
    bias = b_hh.detach().to(dtype) if b_hh is not None else torch.zeros(2, 4 * H, dtype=dtype)
    g3 = gx.view(nseq, L, 8 * H)
    outs = [[None] * L, [None] * L]
    gates = torch.zeros(2, nseq, L, 4 * H, dtype=dtype)
    hprev = torch.zeros(2, nseq, L, H, dtype=dtype)
    cprev = torch.zeros(2, nseq, L, H, dtype=dtype)
    hlast = []
    for d in range(2):
        h = torch.zeros(nseq, H, dtype=dtype)
        c = torch.zeros(nseq, H, dtype=dtype)
        for t in range(L):
            tt = L - 1 - t if d else t
            pre = g3[:, tt, d * 4 * H:(d + 1) * 4 * H] + h @ w[d].t() + bias[d]
            i, f, g, o = pre.chunk(4, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            hprev[d, :, tt] = h.detach()
            cprev[d, :, tt] = c.detach()
            gates[d, :, tt] = torch.cat([i, f, g, o], 1).detach()
            c = f * c + i * g
            h = o * torch.tanh(c)
            outs[d][tt] = h
        hlast.append(h)
    tok = 0.5 * (torch.stack(outs[0], 1) + torch.stack(outs[1], 1)).reshape(T, H)
    news = 0.5 * (hlast[0] + hlast[1])
    out = {"news": news.detach(), "tok": tok.detach(), "gates": gates.view(2, T, 4 * H),
           "hprev": hprev.view(2, T, H), "cprev": cprev.view(2, T, H),
           "hlast": torch.stack(hlast).detach()}
    if dnews is not None or dtok is not None:
        loss = 0
        if dnews is not None:
            loss = loss + (news * dnews.detach().to(dtype)).sum()
        if dtok is not None:
            loss = loss + (tok * dtok.detach().to(dtype)).sum()
        dg, = torch.autograd.grad(loss, [gx])
        out["dg"] = dg
        out["dw_hh"] = torch.stack([dg[:, d * 4 * H:(d + 1) * 4 * H].t() @ out["hprev"][d] for d in range(2)])
    return out


def birnn_inputs(nseq, L, H, seed):
    """Seeded float32 inputs at rnn_util.rnn_inputs' scales: gx and the output gradients standard normal,
    w_hh 1.5 / sqrt(H), b_hh 0.1."""
    g = torch.Generator().manual_seed(seed)
    return {
        "gx": torch.randn(nseq * L, 8 * H, generator=g),
        "w_hh": torch.randn(2, 4 * H, H, generator=g) * (1.5 / H ** 0.5),
        "b_hh": torch.randn(2, 4 * H, generator=g) * 0.1,
        "dnews": torch.randn(nseq, H, generator=g),
        "dtok": torch.randn(nseq * L, H, generator=g),
    }


def unpack_gates(buf, nseq, L, H):
    """nr_birnn_fwd's saved gates (flat, [2][ntile][L][UT][5][64], lane = 16 * (unit & 3) + (seq & 15))
    -> (gates [2, nseq*L, 4H], cprev [2, nseq*L, H], rest): ``rest`` holds every element that belongs to
    no (unit < H, sequence < nseq) pair -- the kernel writes zeros there."""
    UT, ntile = (H + 3) // 4, (nseq + 15) // 16
    n = 2 * ntile * L * UT * 5 * 64
    v = buf[:n].view(2, ntile, L, UT, 5, 4, 16).permute(0, 1, 6, 2, 4, 3, 5).reshape(2, ntile * 16, L, 5, 4 * UT)
    live = v[:, :nseq, :, :, :H]
    gates = live[:, :, :, :4].reshape(2, nseq * L, 4 * H)
    cprev = live[:, :, :, 4].reshape(2, nseq * L, H)
    rest = torch.cat([v[:, nseq:].reshape(-1), v[:, :nseq, :, :, H:].reshape(-1)])
    return gates, cprev, rest
