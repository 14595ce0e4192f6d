"""Golden vectors for the dense-synthesizer self-attention from the REFERENCE's own module
(models/Modules/Synthesizer.py BertSelfAttention, the block `-b synthesizer` puts into every BERT layer,
models/PLM.py:37-47), in float64.

Runs where the reference checkout is available only (make_golden.REF, read-only).  The attention module is
run alone: the installed transformers' BertAttention unpacks two values from ``self.self(...)`` while the
reference module returns a 1-tuple, so the whole model cannot host it offline.  n 3 titles, L 5
(signal_length), H 128; parameters seeded at O(1) pre-activations.  Writes synthesizer.npz (data only): the
input x [n, L, H], the output weighting w, the six parameters under their state_dict names, the output
``out`` and the gradients of sum(out * w) with respect to x (``grad.x``) and every parameter
(``grad.<name>``).

Usage:  python tests/golden/make_synthesizer_golden.py [--out tests/golden]
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

N, L, H = 3, 5, 128
SEED = 33


def run(out_dir):
    sys.path.insert(0, MG.REF)
    sys.dont_write_bytecode = True
    from models.Modules.Synthesizer import BertSelfAttention
    torch.manual_seed(SEED)
    cfg = types.SimpleNamespace(num_attention_heads=2, hidden_size=H, signal_length=L,
                                attention_probs_dropout_prob=0.1)
    att = BertSelfAttention(cfg).double().eval()
    assert list(att.state_dict()) == ["dense.0.weight", "dense.0.bias", "dense.2.weight", "dense.2.bias",
                                      "value_fn.weight", "value_fn.bias"]
    g = torch.Generator().manual_seed(SEED)
    out = {}
    with torch.no_grad():
        for name, p in att.named_parameters():
            if p.dim() == 1:
                val = 0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64)
            else:                      # unit-variance inputs -> O(1) pre-activations
                val = torch.randn(p.shape, generator=g, dtype=torch.float64) * 1.2 / p.shape[1] ** 0.5
            p.copy_(val)
            out[name] = p.detach().numpy().copy()
    x = torch.randn(N, L, H, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(N, L, H, generator=g, dtype=torch.float64)
    y = att(x)[0]
    (y * w).sum().backward()
    out.update(x=x.detach().numpy(), w=w.numpy(), out=y.detach().numpy())
    out["grad.x"] = x.grad.numpy()
    for name, p in att.named_parameters():
        out["grad." + name] = p.grad.numpy()
    path = os.path.join(out_dir, "synthesizer.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("keys:", sorted(k for k in out if not k.startswith("grad.")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    run(ap.parse_args().out)
