"""The bidirectional-LSTM news encoder on the GPU, level by level:

  kernel   K.birnn_fwd / K.birnn_bwd (csrc/birnn.hip) called directly with gx supplied by the test (no
           GEMM in the path) into NaN-filled buffers with padded leading dimensions, against the
           float64 reference of tests/birnn_util.py;
  module   encoders.RNN_Encoder (autograd wrapper RNNNewsFn: gather-fused projection GEMM, recurrence,
           weight / table gradients) against the reference model's golden tests/golden/rnn_news.npz;
  model    build_model("rnn", "attn", 150) train logits and gradients against a float64 CPU composition
           of torch.nn.LSTM with oracle.restatement's pooling and scorer;
  graph    one captured train step replayed against eager.

nr_birnn_* dispatch on H alone: NT = ceil(ceil(H / 4) / 8) unit tiles per wave (H 3 -> 1, 64 -> 2,
96 -> 3, 150 -> 5) and, in the backward, 1 (H <= 128) or 2 row tiles of W_hh^T per wave.

The bar of the kernel-level cases is test_rnn_gpu.py's: with e32 = max|ref32 - ref64| per tensor (the
same reference evaluated in float32 on the CPU), the kernel must stay within
32 e32 + 32 * 2^-24 * max|ref64|, and that bar may itself never exceed 1e-4 * max|ref64|.  Every case
prints its err / e32 ratios ("birnn-ratio" lines, pytest -s).  Measured on an MI355X, the largest
ratio of any case and tensor: 2.16."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birnn_util import birnn_inputs, birnn_reference, unpack_gates

NAN = float("nan")
PAD_GX, PAD_H, PAD_DG = 5, 3, 7      # leading dimensions wider than the row by these many floats
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnn_news.npz")

# tok requested, dnews given, dtok given, b_hh given
VARIANTS = {
    "all": dict(tok=True, dnews=True, dtok=True, bias=True),
    "train": dict(tok=False, dnews=True, dtok=False, bias=True),     # the fused train path
    "tokens": dict(tok=True, dnews=False, dtok=True, bias=False),
}


def _cases():
    out = [(17, 2, H, v) for H in (150, 64, 96, 3) for v in VARIANTS]               # every width, every variant
    for H in (150, 64):
        out += [(n, 2, H, "all") for n in (1, 15, 16, 33)]                            # every tile boundary
        out += [(17, L, H, "all") for L in (1, 30)] + [(17, 1, H, "train")]           # every length
    out += [(33, 30, 150, "train")]
    return out


CASES = _cases()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _padded(t, pad):
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_kernels(nseq, L, H, inp, v):
    """One nr_birnn_fwd and one nr_birnn_bwd (on the forward's own saved gates, as RNNNewsFn runs them)
    into NaN-filled buffers -> {name: the whole buffer on the CPU, the padding columns included}."""
    from newsrec_amd import kernels as K
    T = nseq * L
    gx = _padded(inp["gx"], PAD_GX)
    whh_f, whh_b = K.birnn_pack_whh(inp["w_hh"][0].cuda(), inp["w_hh"][1].cuda())
    bhh = inp["b_hh"].cuda() if v["bias"] else None
    n_g = K.birnn_gates_numel(nseq, L, H)
    gates = _nan(n_g + 64)                                   # 64 guard floats behind the documented size
    hprev = _nan(2, T, H + PAD_H)
    hlast = _nan(2, nseq, H)
    news = _nan(nseq, H + PAD_H)
    tok = _nan(T, H + PAD_H) if v["tok"] else None
    K.birnn_fwd(gx, whh_f, bhh, nseq, L, H, gates, hprev, hlast, news[:, :H], tok=tok[:, :H] if tok is not None else None)
    dg = _nan(T, 8 * H + PAD_DG)
    dnews = _padded(inp["dnews"], PAD_H) if v["dnews"] else None
    dtok = _padded(inp["dtok"], PAD_H) if v["dtok"] else None
    K.birnn_bwd(whh_b, gates, nseq, L, H, dg[:, :8 * H], dnews=dnews, dtok=dtok)
    torch.cuda.synchronize()
    out = dict(gates_buf=gates, hprev=hprev, hlast=hlast, news=news, tok=tok, dg=dg)
    return {k: t.cpu() for k, t in out.items() if t is not None}


@pytest.mark.parametrize("nseq,L,H,variant", CASES, ids=["n%d-L%d-H%d-%s" % c for c in CASES])
def test_kernels_vs_reference(nseq, L, H, variant):
    v = VARIANTS[variant]
    T = nseq * L
    inp = birnn_inputs(nseq, L, H, 1000 * H + 10 * nseq + L)
    out = run_kernels(nseq, L, H, inp, v)

    # ---- exact properties: the layout
    from newsrec_amd import kernels as K
    n_g = K.birnn_gates_numel(nseq, L, H)
    assert torch.isnan(out["gates_buf"][n_g:]).all(), "gates: written past the documented size"
    assert torch.isfinite(out["gates_buf"][:n_g]).all(), "gates: unwritten or non-finite values"
    gates, cprev, rest = unpack_gates(out["gates_buf"], nseq, L, H)
    assert (rest == 0).all(), "gates: elements of no (unit, sequence) pair are not zero"
    for name, width in (("news", H), ("tok", H), ("dg", 8 * H)):
        if name in out:
            assert torch.isnan(out[name][:, width:]).all(), "%s: written past column %d" % (name, width)
            assert torch.isfinite(out[name][:, :width]).all(), "%s: unwritten or non-finite values" % name
    assert torch.isnan(out["hprev"][:, :, H:]).all(), "hprev: written past column %d" % H
    assert torch.isfinite(out["hprev"][:, :, :H]).all() and torch.isfinite(out["hlast"]).all()
    got = dict(news=out["news"][:, :H], gates=gates, cprev=cprev, hprev=out["hprev"][:, :, :H], hlast=out["hlast"],
               dg=out["dg"][:, :8 * H])
    if v["tok"]:
        got["tok"] = out["tok"][:, :H]
    got["dw_hh"] = torch.stack([got["dg"][:, d * 4 * H:(d + 1) * 4 * H].double().t() @ got["hprev"][d].double()
                                for d in range(2)])
    if L == 1:   # h_{t-1} of the only step is the zero initial state: the reference's scale is 0 here
        assert (got["hprev"] == 0).all() and (got["cprev"] == 0).all()
        assert (got["dw_hh"] == 0).all(), "dW_hh's operand product is not exactly zero at L = 1"

    # ---- the reference and the bar
    kw = dict(dnews=inp["dnews"] if v["dnews"] else None, dtok=inp["dtok"] if v["dtok"] else None)
    bias = inp["b_hh"] if v["bias"] else None
    ref = {dt: birnn_reference(inp["gx"], inp["w_hh"], bias, nseq, L, dtype=dt, **kw)
           for dt in (torch.float64, torch.float32)}
    late = []
    for name in ("news", "tok", "gates", "cprev", "hprev", "hlast", "dg", "dw_hh"):
        if name not in got:
            continue
        want = ref[torch.float64][name]
        scale = want.abs().max().item()
        if scale == 0:
            assert (got[name] == 0).all(), name
            continue
        e32 = (ref[torch.float32][name].double() - want).abs().max().item()
        bar = 32 * e32 + 32 * 2.0 ** -24 * scale
        err = (got[name].double() - want).abs().max().item()
        print("birnn-ratio n%d-L%d-H%d-%s %-5s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (nseq, L, H, variant, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        if not err <= bar:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))
    assert not late, "; ".join(late)

    again = run_kernels(nseq, L, H, inp, v)      # no atomics: a second call gives the same bits
    for name in out:
        assert _bits_equal(out[name], again[name]), "%s differs between two calls" % name


def test_tokens_do_not_change_news_or_state():
    """tok == NULL writes the same news and saved state, bit for bit, as a call that asks for tokens."""
    inp = birnn_inputs(17, 3, 150, 5)
    a = run_kernels(17, 3, 150, inp, VARIANTS["all"])
    b = run_kernels(17, 3, 150, inp, dict(VARIANTS["all"], tok=False))
    for name in ("news", "gates_buf", "hprev", "hlast", "dg"):
        assert _bits_equal(a[name], b[name]), name


# ---------------------------------------------------------------------- the module

@pytest.fixture(params=["bf16x6", "f32"])
def gemm_prec(request):
    """Both GEMM arithmetics, as in tests/test_rnn_gpu.py."""
    from newsrec_amd import _lib as Lb, kernels as Kn
    old = Kn.set_gemm_precision(Lb.GEMM_BF16X6 if request.param == "bf16x6" else Lb.GEMM_F32)
    yield request.param
    Kn.set_gemm_precision(old)


def _golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _golden_encoder(z):
    from newsrec_amd import encoders as E
    from model_util import Cfg
    E_, H = z["x"].shape[-1], z["rnn.weight_hh_l0"].shape[1]
    mod = E.RNN_Encoder(Cfg("rnn", "attn", H, bert_dim=E_)).cuda()
    sd = {k: v.float() for k, v in z.items() if k.startswith("rnn.")}
    mod.load_state_dict(sd)            # the reference's parameter names, all of them
    return mod


def test_module_vs_golden(gemm_prec):
    z = _golden()
    mod = _golden_encoder(z)
    x = z["x"].float().cuda().requires_grad_()
    tok, news = mod(x, attn_mask=torch.zeros(z["x"].shape[:-1], dtype=torch.long, device="cuda"))   # mask ignored
    assert tok.shape == z["tok"].shape and news.shape == z["news"].shape
    ((tok * z["a"].float().cuda()).sum() + (news * z["b"].float().cuda()).sum()).backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(tok.detach().cpu().double(), z["tok"], rtol=0, atol=1e-4)
    torch.testing.assert_close(news.detach().cpu().double(), z["news"], rtol=0, atol=1e-4)
    grads = {"x": x.grad}
    grads.update({"rnn." + n: p.grad for n, p in mod.rnn.named_parameters()})
    assert len(grads) == 9
    for n, got in grads.items():
        ref = z["grad." + n]
        assert got is not None, n
        torch.testing.assert_close(got.cpu().double(), ref, rtol=0, atol=1e-3 * ref.abs().max().item(),
                                   msg=lambda s, n=n: n + ": " + s)


def test_module_news_only_gradient(gemm_prec):
    """An unused token output costs no dtok: the backward runs from dnews alone."""
    z = _golden()
    mod = _golden_encoder(z)
    x = z["x"].float().cuda().requires_grad_()
    _, news = mod(x)
    (news * z["b"].float().cuda()).sum().backward()
    x64 = z["x"].clone().requires_grad_()
    ref = torch.nn.LSTM(x64.shape[-1], news.shape[-1], batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k[4:]: v for k, v in z.items() if k.startswith("rnn.")})
    hn = ref(x64.view(-1, *x64.shape[2:]))[1][0]
    (hn.mean(0).view_as(z["news"]) * z["b"]).sum().backward()
    torch.testing.assert_close(x.grad.cpu().double(), x64.grad, rtol=0, atol=1e-3 * x64.grad.abs().max().item())


def test_encode_tokens_equals_forward():
    """The fused entry (gather inside the GEMM, scatter epilogue) against forward(table[ids]); ids include
    the pad id 0 and repeats; the table's row 0 receives exactly zero gradient."""
    z = _golden()
    mod = _golden_encoder(z)
    E_ = z["x"].shape[-1]
    g = torch.Generator().manual_seed(3)
    table = torch.randn(11, E_, generator=g)
    table[0] = 0
    ids = torch.tensor([[[5, 3, 0, 0, 0], [1, 1, 7, 5, 0], [10, 2, 3, 4, 6]],
                        [[0, 0, 0, 0, 0], [9, 8, 9, 8, 9], [5, 3, 0, 0, 1]]]).cuda()
    wt = torch.randn(2, 3, 5, mod.hidden_dim, generator=g).cuda()
    wn = torch.randn(2, 3, mod.hidden_dim, generator=g).cuda()
    res = []
    for fused in (True, False):
        t = table.clone().cuda().requires_grad_()
        mod.zero_grad()
        if fused:
            tok, news = mod.encode_tokens(t, ids, None, pad_row=0, want_tokens=True)
        else:
            tok, news = mod(torch.nn.functional.embedding(ids, t, padding_idx=0))
        ((tok * wt).sum() + (news * wn).sum()).backward()
        res.append([tok.detach(), news.detach(), t.grad] + [p.grad.clone() for p in mod.parameters()])
    assert (res[0][2][0] == 0).all(), "table row 0 received a gradient"
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    # without tokens: None, and the same news
    tok, news = mod.encode_tokens(table.cuda(), ids, None)
    assert tok is None
    torch.testing.assert_close(news, res[0][1], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------- the model

MB, MC, MN, ML, MV, MH = 2, 3, 4, 5, 64, 150


def _model_batch(seed):
    g = torch.Generator().manual_seed(seed)

    def titles(n):
        tok = torch.randint(1, MV, (n, ML), generator=g)
        lens = torch.randint(1, ML + 1, (n,), generator=g)
        mask = (torch.arange(ML)[None] < lens[:, None]).long()
        return tok * mask, mask
    ct, cm = titles(MB * MC)
    ht, hm = titles(MB * MN)
    his_mask = torch.ones(MB, MN, 1, dtype=torch.float64)
    his_mask[1, -1] = 0
    return {"cdd_encoded_index": ct.view(MB, MC, ML), "cdd_attn_mask": cm.view(MB, MC, ML),
            "his_encoded_index": ht.view(MB, MN, ML), "his_attn_mask": hm.view(MB, MN, ML),
            "his_mask": his_mask, "user_id": torch.tensor([1, 2]), "label": torch.tensor([0, 2])}


def _rnn_model(seed=11):
    from newsrec_amd.manager import build_model
    torch.manual_seed(seed)
    model = build_model("rnn", "attn", MH, vocab=MV)
    with torch.no_grad():     # O(1) pre-activations: the table at 0.5, the input weights at 1 / sqrt(E)
        model.embedding.bert_word_embedding.weight.mul_(0.5)
        model.embedding.bert_word_embedding.weight[0] = 0
    return model


def test_build_model_dispatch():
    from newsrec_amd import encoders as E
    from newsrec_amd.manager import build_model
    assert isinstance(build_model("rnn", "attn", MH, vocab=MV).encoderN, E.RNN_Encoder)
    with pytest.raises(ValueError):
        build_model("nope", "attn", MH, vocab=MV)


def _model_reference(model, x):
    """Float64 CPU composition: torch.nn.LSTM over table[tokens] (all steps, masks ignored), then
    oracle.restatement's attention pooling, scorer and NLL."""
    from oracle import restatement as R
    P = {n: p.detach().cpu().double().requires_grad_() for n, p in model.named_parameters()}
    lstm = torch.nn.LSTM(P["embedding.bert_word_embedding.weight"].shape[1], MH, batch_first=True,
                         bidirectional=True).double()

    def news(tokens):
        emb = R.word_embedding(P["embedding.bert_word_embedding.weight"], tokens)
        w = {n: P["encoderN.rnn." + n] for n, _ in lstm.named_parameters()}
        hn = torch.func.functional_call(lstm, w, (emb.view(-1, ML, emb.shape[-1]),))[1][0]
        return hn.mean(0).view(emb.shape[0], emb.shape[1], MH)
    cdd = news(x["cdd_encoded_index"])
    user = R.attn_pool_user(news(x["his_encoded_index"]), x["his_mask"], P)
    logits = torch.nn.functional.log_softmax(R.compute_score(cdd, user), 1)
    R.nll_loss(logits, x["label"]).backward()
    return logits.detach(), {n: p.grad for n, p in P.items()}


def test_model_train_step_vs_float64(gemm_prec):
    model = _rnn_model()
    model.train()
    x = _model_batch(4)
    logits, loss = model.forward_loss({k: v.cuda() for k, v in x.items()})
    loss.backward()
    torch.cuda.synchronize()
    want, grads = _model_reference(model, x)
    torch.testing.assert_close(logits.detach().cpu().double(), want, rtol=0, atol=1e-3 * want.abs().max().item())
    for n, p in model.named_parameters():
        ref = grads[n]
        assert p.grad is not None and ref is not None, n
        scale = ref.abs().max().item()
        assert scale > 0, n
        torch.testing.assert_close(p.grad.cpu().double(), ref, rtol=0, atol=1e-3 * scale, msg=lambda s, n=n: n + ": " + s)
    assert (model.embedding.bert_word_embedding.weight.grad[0] == 0).all()


# ---------------------------------------------------------------------- graph capture

def test_graph_replay_matches_eager():
    import copy
    from newsrec_amd.manager import get_optim, train_step
    m_eager = _rnn_model(5)
    m_eager.train()
    m_graph = copy.deepcopy(m_eager)
    o_eager, o_graph = get_optim(m_eager, capturable=False), get_optim(m_graph, capturable=True)
    batches = [{k: v.cuda() for k, v in _model_batch(s).items()} for s in (1, 2, 3)]
    static = {k: v.clone() for k, v in batches[0].items()}
    for b in batches[:2]:                        # eager warm-up of both (allocator, optimizer state)
        train_step(m_eager, o_eager, b, check_labels=False)
        for k, v in b.items():
            static[k].copy_(v)
        train_step(m_graph, o_graph, static, check_labels=False)
    torch.cuda.synchronize()
    for k, v in batches[2].items():
        static[k].copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(m_graph, o_graph, static, check_labels=False).detach()
    before = m_graph.encoderN.rnn.weight_hh_l0.detach().clone()
    graph.replay()
    train_step(m_eager, o_eager, batches[2], check_labels=False)
    torch.cuda.synchronize()
    assert not torch.equal(before, m_graph.encoderN.rnn.weight_hh_l0), "the replay did not train"
    for (n, a), (_, b) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=2e-5, msg=n)
