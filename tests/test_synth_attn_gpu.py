"""The PLM synthesizer tower on the GPU.

  kernel   K.synth_attn_fwd / K.synth_attn_bwd (csrc/synth_attn.hip) called directly into NaN-filled buffers
           with padded leading dimensions, against the float64 reference of tests/synth_util.py under the
           project's kernel bar (sha_attn_util.bar_of: 32 e32 + 32 * 2^-24 * max|ref64|).  The backward
           reference takes its ReLU gate from the kernel's own stored a1 > 0, and the test separately asserts
           that this gate differs from the float64 gate only where |z1_64| is within the bar of a1;
  model    BertModel(attention_type="synthesizer") against the float64 composition, in eval() and in train()
           with the hidden-dropout masks replayed through R.BertDropout, both GEMM precisions
           (test_bert_gpu.py's bars: outputs atol 1e-4, gradients 1e-3 of max|grad|);
  wiring   state_dict names and shapes, the default init of the three new Linears, the signal_length check;
  PLM      ManagerConfig(bert="synthesizer"): the fused pass against the unfused encode_news / encode_user,
           the news table, XFormer's refusal, one train step, and its captured-graph replay.

Every kernel case prints its err / e32 ratios ("synth-ratio" lines): the worst ratio per tensor is quoted in
DESIGN.md."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from synth_util import (BWD_TENSORS, FIX, FIX_TORCH_SEED, FWD_TENSORS, KERNEL_CASES, bar_of, case_inputs,
                        case_references, fixture, fixture_shapes, synth_bert_model)

NAN = float("nan")
PAD_H, PAD_C, PAD_D, PAD_G = 4, 8, 12, 4       # leading-dimension pads of hv, ctx, dctx, dhv


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_kernels(nseq, L, D, inp, lda=None, pads=(PAD_H, PAD_C, PAD_D, PAD_G), hv=None):
    """One nr_synth_attn_fwd and one nr_synth_attn_bwd (on the forward's own a1 and probs, as BertFn runs them)
    into NaN-filled buffers -> {name: the whole buffer on the CPU, padding included}.  The padding columns of
    hv and dctx hold NaN: a kernel that read them would spread it.  lda None: ceil4(L) + 4."""
    from newsrec_amd import kernels as K
    T = nseq * L
    lda = (L + 3) // 4 * 4 + 4 if lda is None else lda
    ph, pc, pd, pg = pads
    hvb = _nan(T, D + ph)
    hvb[:, :D] = (inp["hv"] if hv is None else hv).cuda()
    w1, b1, w2, b2 = (inp[n].cuda() for n in ("w1", "b1", "w2", "b2"))
    a1, probs, ctx = _nan(T, lda), _nan(nseq * L * L + 64), _nan(T, D + pc)   # 64 guard floats behind probs
    K.synth_attn_fwd(hvb[:, :D], w1, b1, w2, b2, nseq, L, D, a1[:, :L], probs, ctx[:, :D])
    dctx = _nan(T, D + pd)
    dctx[:, :D] = inp["dctx"].cuda()
    da1, da2, dhv = _nan(T, lda), _nan(T, lda), _nan(T, D + pg)
    K.synth_attn_bwd(hvb[:, :D], w1, w2, a1[:, :L], probs, dctx[:, :D], nseq, L, D, da1[:, :L], da2[:, :L],
                     dhv[:, :D])
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(a1=a1, probs_buf=probs, ctx=ctx, da1=da1, da2=da2, dhv=dhv).items()}


def _unpack(out, nseq, L, D):
    got = {k: out[k][:, :L] for k in ("a1", "da1", "da2")}
    got.update(ctx=out["ctx"][:, :D], dhv=out["dhv"][:, :D], probs=out["probs_buf"][:nseq * L * L].view(nseq, L, L))
    return got


def _check_layout(out, nseq, L, D):
    for k in ("a1", "da1", "da2"):
        assert torch.isnan(out[k][:, L:]).all(), "%s: written in the pad columns [%d, lda)" % (k, L)
    for k in ("ctx", "dhv"):
        assert torch.isnan(out[k][:, D:]).all(), "%s: written past column %d" % (k, D)
    assert torch.isnan(out["probs_buf"][nseq * L * L:]).all(), "probs: written past nseq*L*L"
    got = _unpack(out, nseq, L, D)
    for name, t in got.items():
        assert torch.isfinite(t).all(), "%s: unwritten or non-finite values" % name
    return got


def _compare(tag, names, got, ref, late):
    for name in names:
        want = ref[torch.float64][name]
        bar, e32, scale = bar_of(ref, name)
        if scale == 0:      # L = 1: P = 1, so dA2 = P (dP - dP P) and dA1 are exact zeros
            assert (got[name] == 0).all(), name
            continue
        err = (got[name].double() - want.reshape(got[name].shape)).abs().max().item()
        print("synth-ratio %s %-5s err %.3e e32 %.3e err/e32 %s err/bar %.3f bar %.3e max %.3e"
              % (tag, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", err / bar, bar, scale))
        if not err <= bar:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))


@pytest.mark.parametrize("nseq,L,D", KERNEL_CASES, ids=["n%d-L%d-D%d" % c for c in KERNEL_CASES])
def test_kernels_vs_reference(nseq, L, D):
    inp, fwd = case_inputs(nseq, L, D)
    out = run_kernels(nseq, L, D, inp)
    got = _check_layout(out, nseq, L, D)
    tag = "n%d-L%d-D%d" % (nseq, L, D)
    assert (got["a1"] >= 0).all()
    assert (got["probs"].sum(-1) - 1).abs().max() < 1e-5

    late = []
    _compare(tag, FWD_TENSORS, got, fwd, late)
    # the kernel's gate may differ from the float64 gate only where the pre-activation is within a1's bar of 0
    gate = got["a1"] > 0
    z64 = fwd[torch.float64]["z1"]
    flips = gate != (z64 > 0)
    a1_bar = bar_of(fwd, "a1")[0]
    assert (z64[flips].abs() <= a1_bar).all(), "a ReLU gate flipped at |z1| = %.3e > %.3e" % (
        z64[flips].abs().max().item(), a1_bar)
    _, ref = case_references(nseq, L, D, gate=gate)
    _compare(tag, BWD_TENSORS, got, ref, late)
    assert not late, "; ".join(late)

    again = run_kernels(nseq, L, D, inp)      # no atomics: a second call gives the same bits
    for name in out:
        assert _bits_equal(out[name], again[name]), "%s differs between two calls" % name


@pytest.mark.parametrize("L,lda", [(30, 30), (5, 5), (30, 32), (5, 8)], ids=lambda v: str(v))
def test_exact_and_padded_activation_strides(L, lda):
    """lda = L (rows of 120 B / 20 B: 4-B aligned only) and lda padded to a multiple of 4, the wide matrices at
    ld = D exactly: the same bits as the main test's layout, pad columns untouched."""
    nseq, D = 4, 152
    inp, _ = case_inputs(nseq, L, D)
    base = _unpack(run_kernels(nseq, L, D, inp), nseq, L, D)
    out = run_kernels(nseq, L, D, inp, lda=lda, pads=(0, 0, 0, 0))
    got = _check_layout(out, nseq, L, D)
    assert out["a1"].shape[1] == lda
    for name in base:
        assert _bits_equal(base[name], got[name]), name


def test_pad_tokens_attend_and_are_attended_to():
    """No mask: changing hv at one (padded) position changes ctx at the OTHER positions of that title, and
    nothing in any other title."""
    nseq, L, D = 4, 5, 64
    inp, _ = case_inputs(nseq, L, D)
    a = _unpack(run_kernels(nseq, L, D, inp), nseq, L, D)
    hv = inp["hv"].clone()
    s, j = 2, L - 1                           # the last position of title 2: a pad token in any real batch
    hv[s * L + j] += 1.0
    b = _unpack(run_kernels(nseq, L, D, inp, hv=hv), nseq, L, D)
    ca, cb = a["ctx"].view(nseq, L, D), b["ctx"].view(nseq, L, D)
    others = [t for t in range(nseq) if t != s]
    assert _bits_equal(ca[others], cb[others])
    assert _bits_equal(a["probs"][others], b["probs"][others])
    for i in range(L):
        if i != j:
            assert (ca[s, i] - cb[s, i]).abs().max() > 1e-3, "position %d does not attend to position %d" % (i, j)
    assert (a["probs"][s, j] - b["probs"][s, j]).abs().max() > 1e-4, "the changed position's own scores did not move"


# ---------------------------------------------------------------------- the model

@pytest.fixture(params=["bf16x6", "f32"])
def gemm_prec(request):
    """Both GEMM arithmetics, as in tests/test_transformer_news_gpu.py."""
    from newsrec_amd import _lib as Lb, kernels as Kn
    old = Kn.set_gemm_precision(Lb.GEMM_BF16X6 if request.param == "bf16x6" else Lb.GEMM_F32)
    yield request.param
    Kn.set_gemm_precision(old)


def _config(p_hidden=0.0, **kw):
    from newsrec_amd.bert import BertConfig
    return BertConfig(vocab_size=FIX["vocab"], hidden_size=FIX["hidden"], num_hidden_layers=FIX["layers"],
                      num_attention_heads=FIX["heads"], intermediate_size=FIX["ffn"],
                      max_position_embeddings=FIX["max_pos"], hidden_dropout_prob=p_hidden,
                      attention_probs_dropout_prob=p_hidden, **kw)


def _fixture_model(p_hidden):
    from newsrec_amd.bert import BertModel
    torch.manual_seed(FIX_TORCH_SEED)          # the model's dropout stream takes its seed from here
    model = BertModel(_config(p_hidden, attention_type="synthesizer", signal_length=FIX["L"]))
    P, ids, mask, a, b = fixture()
    sd = model.state_dict()
    assert list(sd) == [n for n, _ in fixture_shapes()]
    with torch.no_grad():
        for n, t in P.items():
            assert sd[n].shape == t.shape, n
            sd[n].copy_(t)
    return model.cuda(), P, ids, mask, a, b


@pytest.mark.parametrize("train", [False, True], ids=["eval", "dropout"])
def test_model_vs_float64_composition(gemm_prec, train):
    from oracle import restatement as R
    model, P, ids, mask, a, b = _fixture_model(FIX["p_hidden"])
    model.train(train)
    rng = model._rng
    assert rng.seed == FIX_TORCH_SEED and rng.offset == 0
    out = model(ids.cuda(), mask.cuda())
    ((out.last_hidden_state * a.cuda()).sum() + (out.pooler_output * b.cuda()).sum()).backward()
    torch.cuda.synchronize()
    T, H = FIX["nseq"] * FIX["L"], FIX["hidden"]
    drop = None
    if train:
        drop = R.BertDropout(FIX_TORCH_SEED, 0, T, H, FIX["layers"], FIX["heads"], FIX["p_hidden"], 0.0)
        # one counter range in the bert tower's layout; the attention site is in it, unused
        assert rng.offset == T * H + FIX["layers"] * T * (64 + 2 * H)
    P64 = {n: t.double().requires_grad_() for n, t in P.items()}
    hid, pooled = synth_bert_model(P64, ids, drop=drop)
    ((hid * a.double()).sum() + (pooled * b.double()).sum()).backward()
    for name, got, want in (("last_hidden_state", out.last_hidden_state, hid), ("pooler_output", out.pooler_output, pooled)):
        err = (got.detach().cpu().double() - want.detach()).abs().max().item()
        print("synth-model %s %s %s: err %.3e (max %.3e)" % (gemm_prec, "train" if train else "eval", name, err,
                                                              want.detach().abs().max().item()))
        assert err <= 1e-4, name
    ps = dict(model.named_parameters())
    assert set(ps) == set(P64)
    worst = 0.0
    for n, p64 in P64.items():
        want = p64.grad.clone()
        if n == "embeddings.word_embeddings.weight":
            want[0] = 0          # nn.Embedding(padding_idx=0): the pad row takes no gradient
        assert ps[n].grad is not None, n
        scale = want.abs().max().item()
        assert scale > 0, n
        err = (ps[n].grad.detach().cpu().double() - want).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 1e-3 * scale, (n, err, scale)
    print("synth-model %s %s: worst gradient error / max %.3e over %d tensors"
          % (gemm_prec, "train" if train else "eval", worst, len(P64)))


def test_model_wiring():
    from newsrec_amd.bert import BertModel
    torch.manual_seed(0)
    L, H = FIX["L"], FIX["hidden"]
    synth = BertModel(_config(attention_type="synthesizer", signal_length=L))
    plain = BertModel(_config())
    want = []
    for k, v in plain.state_dict().items():
        if ".attention.self.query." in k:
            k2, shape = k.replace("query", "dense.0"), (L, H) if k.endswith("weight") else (L,)
        elif ".attention.self.key." in k:
            k2, shape = k.replace("key", "dense.2"), (L, L) if k.endswith("weight") else (L,)
        elif ".attention.self.value." in k:
            k2, shape = k.replace("value", "value_fn"), tuple(v.shape)
        else:
            k2, shape = k, tuple(v.shape)
        want.append((k2, shape))
    got = [(k, tuple(v.shape)) for k, v in synth.state_dict().items()]
    assert sorted(got) == sorted(want)
    assert [k for k, _ in got] == [n for n, _ in fixture_shapes()]
    assert len(synth.flat_params()) == len(plain.flat_params()) == 5 + 16 * FIX["layers"] + 2
    # nn.Linear's default init (uniform +-1/sqrt(fan_in): std 1/sqrt(3 * 128) = 0.051), not normal(0, 0.02)
    att = synth.encoder.layer[1].attention.self
    assert abs(att.value_fn.weight.std().item() - (3 * H) ** -0.5) < 0.005
    assert abs(att.dense[0].weight.std().item() - (3 * H) ** -0.5) < 0.01
    assert att.dense[2].weight.std().item() > 0.1            # 1/sqrt(3 * 5) = 0.26
    assert att.value_fn.bias.abs().max() > 0                 # default biases are not zeroed either
    assert abs(synth.encoder.layer[1].attention.output.dense.weight.std().item() - 0.02) < 0.002
    assert abs(plain.encoder.layer[1].attention.self.value.weight.std().item() - 0.02) < 0.002
    synth = synth.cuda()
    ids = torch.ones(3, L + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        synth(ids, torch.ones_like(ids))
    with pytest.raises(ValueError):
        synth.encode_segments([(ids[:, :L], ids[:, :L]), (ids, ids)])
    with pytest.raises(ValueError):
        BertModel(_config(attention_type="synthesizer"))               # signal_length is required
    with pytest.raises(ValueError):
        BertModel(_config(attention_type="synthesizer", signal_length=65))
    with pytest.raises(ValueError):
        BertModel(_config(attention_type="performer"))


# ---------------------------------------------------------------------- PLM

B_, C_, N_ = 2, 3, 4


def _plm(p_hidden=0.0):
    from newsrec_amd import encoders as E
    from newsrec_amd.manager import ManagerConfig
    from newsrec_amd.xformer import PLM
    H = FIX["hidden"]
    torch.manual_seed(5)
    m = ManagerConfig("bert", "attn", H, bert_dim=H, signal_length=FIX["L"], his_size=N_, npratio=C_ - 1,
                      bert="synthesizer")
    bc = _config(p_hidden, attention_type="synthesizer", signal_length=FIX["L"])
    model = PLM(m, E.Attention_Pooling(m), bert_config=bc)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 2 and "embeddings" not in n and "bert" in n:
                p.normal_(0, 1.2 / p.shape[1] ** 0.5)
    return m, model.cuda()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    L, V = FIX["L"], FIX["vocab"]

    def titles(n):
        t = torch.randint(1, V, (n, L), generator=g)
        lens = torch.randint(1, L + 1, (n,), generator=g)
        msk = (torch.arange(L)[None] < lens[:, None]).long()
        return t * msk, msk
    ct, cm = titles(B_ * C_)
    ht, hm = titles(B_ * N_)
    return {"cdd_encoded_index": ct.view(B_, C_, L), "cdd_attn_mask": cm.view(B_, C_, L),
            "his_encoded_index": ht.view(B_, N_, L), "his_attn_mask": hm.view(B_, N_, L),
            "his_mask": torch.ones(B_, N_, 1, dtype=torch.float64), "his_id": torch.arange(1, 1 + B_ * N_).view(B_, N_),
            "user_id": torch.tensor([1, 2]), "label": torch.tensor([0, 2])}


def test_plm_fused_pass_equals_the_unfused_towers():
    from newsrec_amd import _lib as Lb
    m, model = _plm()
    assert m.name == model.name == "plm__synthesizer__attn"
    assert model.bert.config.attention_type == "synthesizer" and model.bert.config.signal_length == FIX["L"]
    model.eval()
    x = {k: v.cuda() for k, v in _batch(1).items()}
    with torch.no_grad():
        logits, _ = model(x)
        cdd = model.encode_news(x)
        user, _ = model.encode_user(x)
        by_hand = model.compute_score(cdd, user, Lb.SCORE_SIGMOID)
        # the same again through model.bert itself
        L = FIX["L"]
        his = model.bert(x["his_encoded_index"].view(-1, L), x["his_attn_mask"].view(-1, L)).pooler_output
        user2 = model.encoderU(his.view(B_, N_, -1), his_mask=x["his_mask"]) + model.userBias
    # not a comparison between constants: the sigmoid scores spread over 100x the bar below
    assert logits.shape == (B_, C_) and logits.std().item() > 1e-3
    # the same arithmetic over other row counts: a GEMM may take another tiling or K split, so the bar is
    # float32 re-association through 2 layers of O(1) values (a few 1e-6), not bit equality
    torch.testing.assert_close(logits, by_hand, rtol=0, atol=1e-5)
    torch.testing.assert_close(user2, user, rtol=0, atol=1e-5)
    # the history read from an installed news table (PLM.py:95-97)
    table = torch.zeros(1 + B_ * N_, FIX["hidden"], device="cuda")
    table[1:] = his
    model.init_embedding(table)
    with torch.no_grad():
        user3, _ = model.encode_user(x)
        logits3, _ = model(x)
    model.destroy_embedding()
    torch.testing.assert_close(user3, user, rtol=0, atol=1e-5)
    torch.testing.assert_close(logits3, logits, rtol=0, atol=1e-5)


def test_plm_default_config_and_xformer_refusal():
    from newsrec_amd import encoders as E
    from newsrec_amd.manager import ManagerConfig
    from newsrec_amd.xformer import PLM, XFormer
    m = ManagerConfig("bert", "attn", 128, bert_dim=128, signal_length=7, bert="synthesizer")
    assert ManagerConfig().bert == "bert"
    with pytest.raises(NotImplementedError):
        XFormer(m)
    with pytest.raises(NotImplementedError):
        PLM(ManagerConfig("bert", "attn", 128, bert_dim=128, bert="longformer"), E.Attention_Pooling(m))
    from newsrec_amd.bert import BertModel
    small = BertModel(_config(attention_type="synthesizer", signal_length=7))
    assert PLM(m, E.Attention_Pooling(m), bert=small).bert is small
    import newsrec_amd.xformer as X
    seen = {}
    real = X.BertModel
    X.BertModel = lambda cfg: seen.setdefault("cfg", cfg) and small      # the default config, without 12 layers
    try:
        PLM(m, E.Attention_Pooling(m))
    finally:
        X.BertModel = real
    c = seen["cfg"]
    assert (c.attention_type, c.signal_length, c.hidden_size, c.num_attention_heads) == ("synthesizer", 7, 128, 2)


def test_plm_train_step_runs():
    from newsrec_amd.manager import get_optim, train_step
    _, model = _plm(0.1)
    model.train()
    opt = get_optim(model)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    x = {k: v.cuda() for k, v in _batch(2).items()}
    loss = train_step(model, opt, x)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and loss.item() > 0
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert torch.isfinite(p).all(), n
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    for key in ("dense.0.weight", "dense.2.weight", "dense.2.bias", "value_fn.weight", "query_news", "userBias"):
        assert any(key in n for n in moved), key


def test_plm_graph_replay_matches_eager():
    """bench.GraphedStep on the synthesizer PLM: 2 eager warm-up steps + 2 replays vs 4 eager steps, within the
    bars of test_fullsize_gpu.py's replay test."""
    import bench
    from newsrec_amd.manager import get_optim
    _, m_eager = _plm(0.1)
    m_graph = copy.deepcopy(m_eager)
    batches = [{k: v.cuda() for k, v in _batch(10 + i).items()} for i in range(4)]
    o_eager = get_optim(m_eager)
    o_graph = get_optim(m_graph, capturable=True)
    m_eager.train()
    m_graph.train()
    for i in range(2):
        bench.train_step(m_eager, o_eager, batches[i], None)
    g = bench.GraphedStep(m_graph, o_graph, bench.ResidentFeed(batches), None, 2)
    for i in range(2, 4):
        bench.train_step(m_eager, o_eager, batches[i], None)
        g(i)
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=2e-5, msg=n)
