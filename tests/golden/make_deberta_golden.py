"""Golden vectors for the `-b deberta` PLM tower from the installed transformers' DebertaModel, in float64.

Imports transformers only (not the reference checkout).  The model is microsoft/deberta-base's architecture
at a small size: DebertaConfig(vocab 64, H 128, 2 heads of 64, 2 layers, FFN 256, max_position_embeddings 16,
relative_attention, pos_att_type c2p | p2c, max_relative_positions -1, position_biased_input False,
type_vocab_size 0, layer_norm_eps 1e-7, dropouts 0).double(), with DebertaLayerNorm.forward replaced by the
same formula without its float32 cast (the library casts to float32 even in a .double() model).  Parameters
are float32-representable and seeded for O(1) pre-activations.  n 4 titles of L 7 tokens (full, ragged and
one-token masks); PLM's pooler (models/PLM.py:19-28: Linear + GELU on the CLS rows) in float64 on top.

Writes deberta.npz and deberta.part<k>.npz (data only; one golden split so that no file exceeds 1 MB:
tests/deberta_util.golden() reads them as one): ids, mask, the cotangents a / b, every parameter under its
state_dict name (``meta.names`` keeps the state_dict order), ``pooler.0.weight`` / ``pooler.0.bias``,
``last_hidden_state``, ``pooled``, ``meta.delta_min`` / ``meta.delta_max`` (the range of the relative index
the library gathers with), and ``grad.<name>`` of sum(last_hidden_state * a) + sum(pooled * b) for every
parameter.

Usage:  python tests/golden/make_deberta_golden.py [--out tests/golden]
"""
import argparse
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, L, V, H, HEADS, LAYERS, FFN, MAXPOS = 4, 7, 64, 128, 2, 2, 256, 16
LENS = (7, 4, 1, 5)
SEED = 41
PART_BYTES = 1000000


def _ln_forward(self, x):
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return self.weight * ((x - mean) / torch.sqrt(var + self.variance_epsilon)) + self.bias


def _seed_params(named, g):
    with torch.no_grad():
        for name, p in named:
            r = torch.randn(p.shape, generator=g, dtype=torch.float32).double()
            if name.endswith("LayerNorm.weight"):
                val = 1 + 0.2 * r
            elif "embeddings" in name:
                val = 0.5 * r
            elif p.dim() == 1:
                val = 0.2 * r
            else:                      # unit-variance inputs -> O(1) pre-activations
                val = r * 1.2 / p.shape[1] ** 0.5
            p.copy_(val.float().double())


def run(out_dir):
    from transformers import DebertaConfig, DebertaModel
    from transformers.models.deberta import modeling_deberta as M
    M.DebertaLayerNorm.forward = _ln_forward
    cfg = DebertaConfig(vocab_size=V, hidden_size=H, num_attention_heads=HEADS, num_hidden_layers=LAYERS,
                        intermediate_size=FFN, max_position_embeddings=MAXPOS, relative_attention=True,
                        pos_att_type=["c2p", "p2c"], max_relative_positions=-1, position_biased_input=False,
                        type_vocab_size=0, layer_norm_eps=1e-7, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(SEED)
    model = DebertaModel(cfg).double().eval()
    pooler = torch.nn.Sequential(torch.nn.Linear(H, H), torch.nn.GELU()).double()
    g = torch.Generator().manual_seed(SEED)
    _seed_params(model.named_parameters(), g)
    _seed_params(pooler.named_parameters(), g)
    names = list(model.state_dict())
    assert names == [n for n, _ in model.named_parameters()], "a buffer in the state_dict"

    mask = (torch.arange(L)[None] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(1, V, (N, L), generator=g) * mask
    a = torch.randn(N, L, H, generator=g, dtype=torch.float32).double()
    b = torch.randn(N, H, generator=g, dtype=torch.float32).double()

    # the relative index the library gathers with: delta = clamp(i - j + span) with span = min(L, K)
    rel = M.build_relative_position(torch.zeros(1, 1, L, 1), torch.zeros(1, 1, L, 1))
    delta = rel.long() + min(L, MAXPOS)

    hid = model(input_ids=ids, attention_mask=mask).last_hidden_state
    pooled = pooler(hid[:, 0])
    ((hid * a).sum() + (pooled * b).sum()).backward()

    out = {"ids": ids.numpy(), "mask": mask.numpy(), "a": a.numpy(), "b": b.numpy(),
           "last_hidden_state": hid.detach().numpy(), "pooled": pooled.detach().numpy(),
           "meta.names": np.array(names), "meta.delta_min": np.int64(delta.min().item()),
           "meta.delta_max": np.int64(delta.max().item()),
           "meta.config": np.array([V, H, HEADS, LAYERS, FFN, MAXPOS], dtype=np.int64)}
    for prefix, mod in (("", model), ("pooler.", pooler)):
        for name, p in mod.named_parameters():
            p32 = p.detach().float()
            assert torch.equal(p32.double(), p.detach()), name          # float32-representable
            out[prefix + name] = p32.numpy()
            out["grad." + prefix + name] = p.grad.numpy()

    # greedy split into files of at most PART_BYTES of array data
    parts, size = [{}], 0
    for k, v in out.items():
        v = np.asarray(v)
        if size + v.nbytes > PART_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for old in os.listdir(out_dir):
        if old.startswith("deberta.") and old.endswith(".npz"):
            os.remove(os.path.join(out_dir, old))
    for i, part in enumerate(parts):
        path = os.path.join(out_dir, "deberta.npz" if i == 0 else "deberta.part%d.npz" % i)
        np.savez(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes,", len(part), "arrays")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    run(ap.parse_args().out)
