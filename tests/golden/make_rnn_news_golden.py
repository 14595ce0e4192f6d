"""Golden vectors for the bidirectional-LSTM news encoder from the REFERENCE's own RNN_Encoder
(models/Encoders/RNN.py:5-33), in float64.

Runs where the reference checkout is available only (make_golden.REF, read-only).  Batch 2, n 3,
L 5, E 16, H 8, seeded parameters; writes rnn_news.npz (data only): the input x, every parameter
under its nn.LSTM name, the two output weightings a / b, tok, news, and the gradients of
sum(tok * a) + sum(news * b) with respect to x (``grad.x``) and every parameter (``grad.<name>``).

Usage:  python tests/golden/make_rnn_news_golden.py [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (REF)

B, N, L, E, H = 2, 3, 5, 16, 8
SEED = 20


def run(out_dir):
    sys.path.insert(0, MG.REF)
    sys.dont_write_bytecode = True
    from models.Encoders.RNN import RNN_Encoder
    torch.manual_seed(SEED)
    enc = RNN_Encoder(types.SimpleNamespace(embedding_dim=E, hidden_dim=H)).double()
    g = torch.Generator().manual_seed(SEED)
    out = {}
    with torch.no_grad():
        for name, p in enc.rnn.named_parameters():
            std = 0.1 if "bias" in name else 1.5 / p.shape[1] ** 0.5
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * std)
            out["rnn." + name] = p.detach().numpy().copy()
    x = torch.randn(B, N, L, E, generator=g, dtype=torch.float64).requires_grad_()
    a = torch.randn(B, N, L, H, generator=g, dtype=torch.float64)
    b = torch.randn(B, N, H, generator=g, dtype=torch.float64)
    tok, news = enc(x)
    ((tok * a).sum() + (news * b).sum()).backward()
    out.update(x=x.detach().numpy(), a=a.numpy(), b=b.numpy(), tok=tok.detach().numpy(), news=news.detach().numpy())
    out["grad.x"] = x.grad.numpy()
    for name, p in enc.rnn.named_parameters():
        out["grad.rnn." + name] = p.grad.numpy()
    path = os.path.join(out_dir, "rnn_news.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    run(ap.parse_args().out)
