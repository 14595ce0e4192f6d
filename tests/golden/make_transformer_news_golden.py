"""Golden vectors for the one-layer BERT news encoder from the REFERENCE's own Transformer_Encoder
(models/Encoders/Transformer.py, models/Modules/OneLayerBert.py), in float64 and eval() (no dropout).

Runs where the reference checkout is available only (make_golden.REF, read-only), with make_golden.py's
``_softmax_backward_data`` patch (XSoftmax.backward's torch >= 1.13 signature, same math).  Batch 2, n 3,
L 5, E 768 (the reference hard-codes BertConfig().hidden_size), H 8, parameters seeded at O(1)
pre-activations; the mask holds a full title, ragged prefixes, one title with holes and one title
without a token.  Writes transformer_news.npz (data only): the input x, the mask, every parameter under
its state_dict name, the two output weightings a / b, tok, news, and the gradients of
sum(tok * a) + sum(news * b) with respect to x (``grad.x``) and every parameter (``grad.<name>``).

Usage:  python tests/golden/make_transformer_news_golden.py [--out tests/golden]
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

B, N, L, E, H = 2, 3, 5, 768, 8
SEED = 21
MASK = [[[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 0, 0, 0, 0]],
        [[1, 0, 1, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 0]]]


def run(out_dir):
    sys.path.insert(0, MG.REF)
    sys.dont_write_bytecode = True
    import models.Modules.Attention as A
    A._softmax_backward_data = lambda g, y, d, _o: torch._softmax_backward_data(g, y, d, y.dtype)
    from models.Encoders.Transformer import Transformer_Encoder
    torch.manual_seed(SEED)
    enc = Transformer_Encoder(types.SimpleNamespace(hidden_dim=H)).double().eval()
    g = torch.Generator().manual_seed(SEED)
    out = {}
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if "LayerNorm.weight" in name:
                val = 1 + 0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64)
            elif p.dim() == 1:
                val = 0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64)
            else:                      # unit-variance inputs -> O(1) pre-activations
                val = torch.randn(p.shape, generator=g, dtype=torch.float64) * 1.2 / p.shape[1] ** 0.5
            p.copy_(val)
            out[name] = p.detach().numpy().copy()
    x = torch.randn(B, N, L, E, generator=g, dtype=torch.float64).requires_grad_()
    a = torch.randn(B, N, L, H, generator=g, dtype=torch.float64)
    b = torch.randn(B, N, H, generator=g, dtype=torch.float64)
    mask = torch.tensor(MASK, dtype=torch.int64)
    tok, news = enc(x, mask)
    ((tok * a).sum() + (news * b).sum()).backward()
    out.update(x=x.detach().numpy(), mask=mask.numpy(), a=a.numpy(), b=b.numpy(), tok=tok.detach().numpy(),
               news=news.detach().numpy())
    out["grad.x"] = x.grad.numpy()
    for name, p in enc.named_parameters():
        out["grad." + name] = p.grad.numpy()
    path = os.path.join(out_dir, "transformer_news.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("keys:", sorted(k for k in out if not k.startswith("grad.")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    run(ap.parse_args().out)
