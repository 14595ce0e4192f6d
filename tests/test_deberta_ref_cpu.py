"""The restatements of tests/deberta_util.py against independent evidence, on the CPU:

  golden     the float64 composition of DebertaModel + PLM's pooler against the installed transformers'
             DebertaModel (tests/golden/deberta*.npz): outputs and every parameter gradient;
  contract   the kernel contract's formulas (deb_reference: dq, dk, dv, dpk, dpq without autograd) against
             autograd through deb_scores / deb_probs, with a replayed dropout mask and sha_mask's four titles;
  counters   newsrec_amd.deberta.counter_keep (the counter RNG in torch ops) against oracle.restatement's
             dropout_keep, and DebertaDropout's layout against DebertaModel.drop_site_sizes;
  wiring     state_dict names / shapes / order against the golden's record, init statistics, the 64-token
             limit, PLM(bert="deberta")'s name and pooler, XFormer's refusal, newsbert's four layers."""
import numpy as np
import pytest
import torch

import deberta_util as U


@pytest.fixture(scope="module")
def gold():
    return U.golden()


def test_golden_delta_range(gold):
    L = gold["ids"].shape[1]
    assert (int(gold["meta.delta_min"]), int(gold["meta.delta_max"])) == (1, 2 * L - 1)
    d = U.delta_index(L)
    assert (d.min().item(), d.max().item()) == (1, 2 * L - 1)


def test_restatement_vs_golden(gold):
    """Measured: last_hidden_state 9.3e-16 and pooled 8.0e-16 of each tensor's max, the worst gradient ratio
    2.1e-15 over the 38 tensors; the bar is 1e-12."""
    P = U.golden_params(gold, requires_grad=True)
    ids, mask = torch.from_numpy(gold["ids"]), torch.from_numpy(gold["mask"])
    assert mask.sum(1).tolist() == [7, 4, 1, 5]                  # full, ragged, one-token titles
    hid = U.deberta_model(P, ids, mask)
    pooled = U.plm_pooler(P, hid)
    ((hid * torch.from_numpy(gold["a"])).sum() + (pooled * torch.from_numpy(gold["b"])).sum()).backward()
    worst = 0.0
    for name, got in (("last_hidden_state", hid), ("pooled", pooled)):
        want = torch.from_numpy(gold[name])
        r = (got.detach() - want).abs().max().item() / want.abs().max().item()
        print("deberta-golden %s: err / max %.2e" % (name, r))
        assert r <= 1e-12, name
    for n, p in P.items():
        want = torch.from_numpy(gold["grad." + n])
        assert p.grad is not None and want.abs().max() > 0, n
        r = (p.grad - want).abs().max().item() / want.abs().max().item()
        worst = max(worst, r)
        assert r <= 1e-12, (n, r)
    print("deberta-golden worst gradient err / max %.2e over %d tensors" % (worst, len(P)))
    # rel_embeddings: only the rows K - L .. K + L - 1 receive a gradient
    K, L = gold["encoder.rel_embeddings.weight"].shape[0] // 2, ids.shape[1]
    gr = P["encoder.rel_embeddings.weight"].grad
    assert (gr[:K - L] == 0).all() and (gr[K + L:] == 0).all() and gr[K - L + 1: K + L].abs().min(1).values.max() > 0


@pytest.mark.parametrize("nseq,L,heads,p", [(4, 5, 2, 0.0), (4, 7, 1, 0.1), (5, 1, 2, 0.1), (8, 12, 3, 0.1)])
def test_contract_formulas_vs_autograd(nseq, L, heads, p):
    inp, mask, keep, ref = U.case_references(nseq, L, heads, p)
    r = ref[torch.float64]
    leaves = {k: inp[k].double().requires_grad_() for k in ("q", "k", "v", "pk", "pq")}
    P = U.deb_probs(U.deb_scores(leaves["q"], leaves["k"], leaves["pk"], leaves["pq"], U.SCALE), mask)
    Pd = P if keep is None else P * keep.double() / (1.0 - p)
    ctx = torch.matmul(Pd, leaves["v"]).permute(0, 2, 1, 3)
    (ctx * inp["dctx"].double()).sum().backward()
    assert torch.allclose(P.detach(), r["probs"], rtol=0, atol=1e-15)
    assert torch.allclose(ctx.detach(), r["ctx"], rtol=0, atol=1e-14)
    for name, leaf in (("dq", "q"), ("dk", "k"), ("dv", "v"), ("dpk", "pk"), ("dpq", "pq")):
        want = leaves[leaf].grad
        assert (r[name] - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1.0), name
    assert (r["dpk"][0] == 0).all() and (r["dpq"][0] == 0).all()         # row 0 is never indexed
    # the masks: a masked query is uniform with no gradient to its scores, a valid one ignores masked keys
    m = mask != 0
    for s in range(nseq):
        for i in range(L):
            if not m[s, i]:
                assert (r["probs"][s, :, i] == 1.0 / L).all()
            else:
                assert (r["probs"][s, :, i][:, ~m[s]] == 0).all()
                assert (r["probs"][s, :, i].sum(-1) - 1).abs().max() < 1e-14


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_counter_keep_is_the_kernels_mask(p):
    from newsrec_amd.deberta import counter_keep
    from oracle import restatement as R
    seed, off = 0x1234ABCD5, 987654321
    rng = torch.tensor([seed, off], dtype=torch.int64)
    offs = torch.tensor([0, 7, 2 ** 33 + 5], dtype=torch.int64)
    got = counter_keep(rng, offs, 14 * 128, p)
    assert got.shape == (3, 14 * 128) and got.dtype == torch.bool
    for row, o in zip(got, offs.tolist()):
        assert torch.equal(row.view(14, 128), R.dropout_keep(seed, off + o, 14, 128, p))
    assert abs(got.float().mean().item() - (1 - p)) < 0.03


def _small_config(**kw):
    from newsrec_amd.deberta import DebertaConfig
    return DebertaConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                         intermediate_size=256, max_position_embeddings=16, **kw)


def test_dropout_layout_matches_the_model():
    from newsrec_amd.deberta import DebertaModel
    model = DebertaModel(_small_config())
    shapes = [(4, 7), (3, 5)]
    sizes = model.drop_site_sizes(shapes)
    d = U.DebertaDropout(1, 100, shapes, 128, 2, 2, 0.1, 0.1)
    assert len(sizes) == len(d.site) == 1 + 4 * 2
    assert d.site == [100 + sum(sizes[:k]) for k in range(len(sizes))] and d.end == 100 + sum(sizes)
    T = 4 * 7 + 3 * 5
    assert sizes == [T * 128] + [2 * 12 * 128, 2 * (4 * 49 + 3 * 25), T * 128, T * 128] * 2
    assert d.rel(1, 1).shape == (10, 128) and d.attn(0, 1).shape == (3, 2, 5, 5)


def test_state_dict_matches_the_golden_record(gold):
    from newsrec_amd.deberta import DebertaModel
    torch.manual_seed(0)
    model = DebertaModel(_small_config())
    sd = model.state_dict()
    names = [str(n) for n in gold["meta.names"]]
    assert list(sd) == names
    for n in names:
        assert tuple(sd[n].shape) == gold[n].shape, n
    assert [tuple(p.shape) for p in model.flat_params()] == [gold[n].shape for n in names]
    assert tuple(sd["encoder.rel_embeddings.weight"].shape) == (32, 128)
    # transformers' init: normal(0, 0.02), zero biases (q_bias and v_bias included), unit LayerNorms
    att = model.encoder.layer[1].attention.self
    for w in (att.in_proj.weight, att.pos_proj.weight, att.pos_q_proj.weight, model.encoder.rel_embeddings.weight,
              model.encoder.layer[0].output.dense.weight):
        assert abs(w.std().item() - 0.02) < 0.002 and abs(w.mean().item()) < 0.002
    for b in (att.q_bias, att.v_bias, att.pos_q_proj.bias, model.encoder.layer[0].intermediate.dense.bias):
        assert (b == 0).all()
    assert att.in_proj.bias is None and att.pos_proj.bias is None
    ln = model.encoder.layer[0].attention.output.LayerNorm
    assert (ln.weight == 1).all() and (ln.bias == 0).all() and ln.eps == 1e-7
    assert (model.embeddings.word_embeddings.weight[0] == 0).all()
    model.load_state_dict({n: torch.from_numpy(gold[n]) for n in names})     # a checkpoint loads unchanged


def test_default_config_is_deberta_base():
    from newsrec_amd.deberta import DebertaConfig
    c = DebertaConfig()
    assert (c.vocab_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size,
            c.max_position_embeddings, c.layer_norm_eps, c.pad_token_id) == (50265, 768, 12, 12, 3072, 512, 1e-7, 0)


def test_title_length_limit():
    from newsrec_amd.deberta import DebertaConfig, DebertaModel
    model = DebertaModel(DebertaConfig(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
                                       intermediate_size=64, max_position_embeddings=512))
    ids = torch.ones(2, 65, dtype=torch.int64)
    with pytest.raises(ValueError):
        model(ids, torch.ones_like(ids))
    with pytest.raises(ValueError):
        model.encode_segments([(ids[:, :64], ids[:, :64]), (ids, ids)])
    with pytest.raises(ValueError):
        DebertaModel(DebertaConfig(hidden_size=96, num_attention_heads=2))     # 48-dim heads


def _manager(**kw):
    from newsrec_amd.manager import ManagerConfig
    return ManagerConfig("bert", "attn", 128, bert_dim=128, signal_length=7, **kw)


def test_plm_wiring():
    from newsrec_amd import encoders as E
    from newsrec_amd.bert import BertModel
    from newsrec_amd.deberta import DebertaModel
    from newsrec_amd.xformer import PLM, XFormer
    import newsrec_amd.xformer as X
    m = _manager(bert="deberta")
    with pytest.raises(NotImplementedError):
        XFormer(m)                                       # the reference's XFormer reads .pooler_output
    seen = {}
    real_d, real_b = X.DebertaModel, X.BertModel
    X.DebertaModel = lambda cfg: seen.setdefault("deberta", cfg) and DebertaModel(_small_config())
    X.BertModel = lambda cfg: seen.setdefault("bert", cfg) and None
    try:
        model = PLM(m, E.Attention_Pooling(m))           # the default config, without its 12 layers
        PLM(_manager(bert="newsbert"), E.Attention_Pooling(m))
    finally:
        X.DebertaModel, X.BertModel = real_d, real_b
    c = seen["deberta"]
    assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.vocab_size, c.max_position_embeddings,
            c.layer_norm_eps) == (128, 2, 12, 50265, 512, 1e-7)
    assert m.name == model.name == "plm__deberta__attn"
    names = dict(model.named_parameters())
    assert tuple(names["pooler.0.weight"].shape) == (128, 128) and tuple(names["pooler.0.bias"].shape) == (128,)
    assert isinstance(model.pooler[1], torch.nn.GELU) and isinstance(model.bert, DebertaModel)
    assert "bert.encoder.rel_embeddings.weight" in names and "bert.encoder.layer.0.attention.self.q_bias" in names
    # "pooler.*" is not a "bert" parameter: it takes the base learning rate, as in the reference
    from newsrec_amd.manager import get_optim
    opt = get_optim(model)
    lr_of = {id(p): g["lr"] for g in opt.param_groups for p in g["params"]}
    assert lr_of[id(names["pooler.0.weight"])] == m.lr and lr_of[id(names["bert.encoder.rel_embeddings.weight"])] == m.bert_lr
    # newsbert: BERT cut to its first four layers, BERT's own pooler, no PLM pooler
    nb = seen["bert"]
    assert (nb.num_hidden_layers, nb.attention_type, nb.hidden_size, nb.num_attention_heads) == (4, "bert", 128, 2)
    small = BertModel(type(nb)(vocab_size=64, hidden_size=128, num_hidden_layers=4, num_attention_heads=2,
                               intermediate_size=256, max_position_embeddings=16))
    mn = _manager(bert="newsbert")
    pn = PLM(mn, E.Attention_Pooling(mn), bert=small)
    assert len(pn.bert.encoder.layer) == 4 and not hasattr(pn, "pooler") and pn.name == "plm__newsbert__attn"
    with pytest.raises(NotImplementedError):
        XFormer(_manager(bert="newsbert"))
    with pytest.raises(NotImplementedError):
        PLM(_manager(bert="longformer"), E.Attention_Pooling(m))
    assert np.isclose(U.SCALE, 192 ** -0.5, rtol=1e-7)
