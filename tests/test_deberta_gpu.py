"""The PLM DeBERTa tower on the GPU.

  kernel   K.deb_attn_fwd / K.deb_attn_bwd (csrc/deberta_attn.hip) called directly into NaN-filled buffers with
           padded leading dimensions, in both column layouts, against the float64 contract of
           tests/deberta_util.py under the project's kernel bar (sha_attn_util.bar_of: 32 e32 + 32 * 2^-24 *
           max|ref64|) over ctx, probs, dq, dk, dv, dpk, dpq; pad and unrelated columns untouched, row 0 of
           dpk / dpq zero, a second call bit-equal;
  model    DebertaModel + PLM's pooler at the golden's shapes against the float64 composition, in eval() and in
           train() with every dropout mask replayed (DebertaDropout), both GEMM precisions (test_bert_gpu.py's
           bars: outputs atol 1e-4, gradients 1e-3 of max|grad|), every parameter covered;
  PLM      ManagerConfig(bert="deberta"): the fused pass against the unfused encode_news / encode_user, the news
           table, one train step, and its captured-graph replay.

Every kernel case prints its err / e32 ratios ("deb-ratio" lines): the worst ratio per tensor is quoted in
DESIGN.md."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_util as U
from deberta_util import KERNEL_CASES, KERNEL_OFFSET, KERNEL_SEED, TENSORS, bar_of, case_id, case_references

@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """Some later tests depend on where the caching allocator places a block (test_row_grad_gpu.py reuses a
    freed gradient's address): give back every block this module cached, so it leaves no free blocks of its
    own sizes behind."""
    yield
    import gc
    U._CASE_CACHE.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


NAN = float("nan")
PAD_Q, PAD_P, PAD_C, PAD_D, PAD_G, PAD_R = 4, 8, 12, 4, 8, 4      # ld pads of qkv, pk/pq, ctx, dctx, dqkv, dpk/dpq


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _layout(name, heads):
    from newsrec_amd import kernels as K
    if name == "interleaved":
        return K.DEB_INTERLEAVED
    if name == "blocked":
        return K.deb_blocked(heads)
    return name                                          # an explicit (hstride, qoff, koff, voff)


def _cols(layout, heads):
    """-> ({'q' / 'k' / 'v': column index [heads, 64]}, width)."""
    hs, qo, ko, vo = layout
    base = torch.arange(heads)[:, None] * hs + torch.arange(64)[None, :]
    return {"q": base + qo, "k": base + ko, "v": base + vo}, (heads - 1) * hs + max(qo, ko, vo) + 64


def run_kernels(nseq, L, heads, layout, p, inp, mask, pads=(PAD_Q, PAD_P, PAD_C, PAD_D, PAD_G, PAD_R)):
    """One nr_deb_attn_fwd and one nr_deb_attn_bwd (on the forward's own probs, as DebertaFn runs them) into
    NaN-filled buffers -> {name: the whole buffer on the CPU, padding included}.  The padding columns of qkv,
    pk, pq and dctx hold NaN: a kernel that read them would spread it."""
    from newsrec_amd import kernels as K
    T, H = nseq * L, 64 * heads
    pq_, pp, pc, pd, pg, pr = pads
    cols, width = _cols(layout, heads)
    qkv = _nan(T, width + pq_)
    for n in ("q", "k", "v"):
        qkv[:, cols[n].reshape(-1).cuda()] = inp[n].permute(0, 2, 1, 3).reshape(T, H).cuda()
    pk, pq =_nan(2 * L, H + pp), _nan(2 * L, H + pp)
    pk[:, :H] = inp["pk"].reshape(2 * L, H).cuda()
    pq[:, :H] = inp["pq"].reshape(2 * L, H).cuda()
    m = mask.cuda()
    probs, ctx = _nan(nseq * heads * L * L + 64), _nan(T, H + pc)       # 64 guard floats behind probs
    drop = dict(p_drop=p, seed=KERNEL_SEED, offset=KERNEL_OFFSET) if p > 0 else {}
    K.deb_attn_fwd(qkv[:, :width], pk[:, :H], pq[:, :H], m, nseq, L, heads, probs, ctx[:, :H], layout=layout,
                   scale=U.SCALE, **drop)
    dctx = _nan(T, H + pd)
    dctx[:, :H] = inp["dctx"].reshape(T, H).cuda()
    dqkv, dpk, dpq = _nan(T, width + pg), _nan(2 * L, H + pr), _nan(2 * L, H + pr)
    K.deb_attn_bwd(qkv[:, :width], pk[:, :H], pq[:, :H], m, nseq, L, heads, probs, dctx[:, :H], dqkv[:, :width],
                   dpk[:, :H], dpq[:, :H], layout=layout, scale=U.SCALE, **drop)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(probs_buf=probs, ctx=ctx, dqkv=dqkv, dpk=dpk, dpq=dpq).items()}


def _unpack(out, nseq, L, heads, layout):
    T, H = nseq * L, 64 * heads
    cols, width = _cols(layout, heads)
    got = {"probs": out["probs_buf"][:nseq * heads * L * L].view(nseq, heads, L, L),
           "ctx": out["ctx"][:, :H].reshape(nseq, L, heads, 64),
           "dpk": out["dpk"][:, :H].reshape(2 * L, heads, 64), "dpq": out["dpq"][:, :H].reshape(2 * L, heads, 64)}
    for n in ("q", "k", "v"):
        got["d" + n] = out["dqkv"][:, cols[n].reshape(-1)].reshape(nseq, L, heads, 64).permute(0, 2, 1, 3)
    return got, cols, width


def _check_layout(out, nseq, L, heads, layout):
    H = 64 * heads
    got, cols, width = _unpack(out, nseq, L, heads, layout)
    assert torch.isnan(out["probs_buf"][nseq * heads * L * L:]).all(), "probs: written past nseq*heads*L*L"
    for k in ("ctx", "dpk", "dpq"):
        assert torch.isnan(out[k][:, H:]).all(), "%s: written past column %d" % (k, H)
    used = torch.zeros(out["dqkv"].shape[1], dtype=torch.bool)
    for n in ("q", "k", "v"):
        used[cols[n].reshape(-1)] = True
    assert torch.isnan(out["dqkv"][:, ~used]).all(), "dqkv: written outside the q / k / v blocks"
    for name, t in got.items():
        assert torch.isfinite(t).all(), "%s: unwritten or non-finite values" % name
    assert (got["dpk"][0] == 0).all() and (got["dpq"][0] == 0).all(), "row 0 of dpk / dpq is not zero"
    return got


def _compare(tag, got, ref, late):
    for name in TENSORS:
        want = ref[torch.float64][name]
        bar, e32, scale = bar_of(ref, name)
        if scale == 0:      # L = 1: P = 1, so dS and everything behind it are exact zeros
            assert (got[name] == 0).all(), name
            continue
        err = (got[name].double() - want.reshape(got[name].shape)).abs().max().item()
        print("deb-ratio %s %-5s err %.3e e32 %.3e err/e32 %s err/bar %.3f bar %.3e max %.3e"
              % (tag, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", err / bar, bar, scale))
        if not err <= bar:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))


def _check_masks(got, mask, L):
    """Padded query rows are 1 / L at every key and give their scores no gradient: with dS = 0 there, dq of a
    padded query is exactly 0; a valid query's probabilities are exactly 0 at the padded keys."""
    m = mask != 0
    qm = m[:, None, :, None].expand_as(got["probs"])
    km = m[:, None, None, :].expand_as(got["probs"])
    assert (got["probs"][~qm] == 1.0 / torch.tensor(float(L))).all(), "a padded query row is not 1 / L"
    assert (got["probs"][qm & ~km] == 0).all(), "a valid query attends to a padded key"
    assert (got["dq"][~m[:, None, :].expand(got["dq"].shape[:3])] == 0).all(), "a padded query row has dS != 0"


@pytest.mark.parametrize("nseq,L,heads,layout,p", KERNEL_CASES, ids=[case_id(c) for c in KERNEL_CASES])
def test_kernels_vs_reference(nseq, L, heads, layout, p):
    inp, mask, keep, ref = case_references(nseq, L, heads, p)
    lay = _layout(layout, heads)
    out = run_kernels(nseq, L, heads, lay, p, inp, mask)
    got = _check_layout(out, nseq, L, heads, lay)
    _check_masks(got, mask, L)
    late = []
    _compare(case_id((nseq, L, heads, layout, p)), got, ref, late)
    assert not late, "; ".join(late)
    again = run_kernels(nseq, L, heads, lay, p, inp, mask)      # no atomics: a second call gives the same bits
    for name in out:
        assert _bits_equal(out[name], again[name]), "%s differs between two calls" % name


def test_gapped_layout_and_exact_strides():
    """A layout with 64 unrelated columns per head (hstride 256): the gaps of dqkv stay untouched; and every
    matrix at its exact width (no ld padding): the same bits as the padded buffers."""
    nseq, L, heads, p = 4, 5, 2, 0.1
    inp, mask, keep, ref = case_references(nseq, L, heads, p)
    base, _, _ = _unpack(run_kernels(nseq, L, heads, _layout("interleaved", heads), p, inp, mask), nseq, L, heads,
                         _layout("interleaved", heads))
    for lay, pads in (((256, 64, 0, 128), (PAD_Q, PAD_P, PAD_C, PAD_D, PAD_G, PAD_R)),
                      (_layout("interleaved", heads), (0, 0, 0, 0, 0, 0)), (_layout("blocked", heads), (0, 0, 0, 0, 0, 0))):
        out = run_kernels(nseq, L, heads, lay, p, inp, mask, pads=pads)
        got = _check_layout(out, nseq, L, heads, lay)
        for name in base:
            assert _bits_equal(base[name], got[name]), (lay, name)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool, torch.float32, torch.float64])
def test_mask_dtypes(dtype):
    from newsrec_amd import kernels as K
    nseq, L, heads = 4, 5, 2
    inp, mask, _, _ = case_references(nseq, L, heads, 0.0)
    lay = K.DEB_INTERLEAVED
    a = run_kernels(nseq, L, heads, lay, 0.0, inp, mask)
    b = run_kernels(nseq, L, heads, lay, 0.0, inp, mask.to(dtype))
    for name in a:
        assert _bits_equal(a[name], b[name]), name


# ---------------------------------------------------------------------- the model

TORCH_SEED = 11          # torch.manual_seed before the model is built: the seed of its dropout stream
P_DROP = 0.1


@pytest.fixture(params=["bf16x6", "f32"])
def gemm_prec(request):
    """Both GEMM arithmetics, as in tests/test_synth_attn_gpu.py."""
    from newsrec_amd import _lib as Lb, kernels as Kn
    old = Kn.set_gemm_precision(Lb.GEMM_BF16X6 if request.param == "bf16x6" else Lb.GEMM_F32)
    yield request.param
    Kn.set_gemm_precision(old)


@pytest.fixture(scope="module")
def gold():
    return U.golden()


def _config(gold, p=0.0):
    from newsrec_amd.deberta import DebertaConfig
    V, H, heads, layers, ffn, maxpos = (int(v) for v in gold["meta.config"])
    return DebertaConfig(vocab_size=V, hidden_size=H, num_hidden_layers=layers, num_attention_heads=heads,
                         intermediate_size=ffn, max_position_embeddings=maxpos, hidden_dropout_prob=p,
                         attention_probs_dropout_prob=p)


def _golden_model(gold, p):
    from newsrec_amd.deberta import DebertaModel
    torch.manual_seed(TORCH_SEED)
    model = DebertaModel(_config(gold, p))
    names = [str(n) for n in gold["meta.names"]]
    assert list(model.state_dict()) == names
    model.load_state_dict({n: torch.from_numpy(gold[n]) for n in names})
    pooler = torch.nn.Linear(model.config.hidden_size, model.config.hidden_size)
    with torch.no_grad():
        pooler.weight.copy_(torch.from_numpy(gold["pooler.0.weight"]))
        pooler.bias.copy_(torch.from_numpy(gold["pooler.0.bias"]))
    return model.cuda(), pooler.cuda()


@pytest.mark.parametrize("train", [False, True], ids=["eval", "dropout"])
def test_model_vs_float64_composition(gold, gemm_prec, train):
    from newsrec_amd.deberta import ClsGeluPoolFn
    model, pooler = _golden_model(gold, P_DROP)
    model.train(train)
    rng = model._rng
    assert rng.seed == TORCH_SEED and rng.offset == 0
    ids, mask = torch.from_numpy(gold["ids"]), torch.from_numpy(gold["mask"])
    a, b = torch.from_numpy(gold["a"]), torch.from_numpy(gold["b"])
    n, L = ids.shape
    c = model.config
    out = model(ids.cuda(), mask.cuda())
    pooled = ClsGeluPoolFn.apply(out.last_hidden_state, pooler.weight, pooler.bias)
    ((out.last_hidden_state * a.float().cuda()).sum() + (pooled * b.float().cuda()).sum()).backward()
    torch.cuda.synchronize()
    drop = None
    if train:
        drop = U.DebertaDropout(TORCH_SEED, 0, [(n, L)], c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                                P_DROP, P_DROP)
        assert rng.offset == drop.end == sum(model.drop_site_sizes([(n, L)]))
    P64 = U.golden_params(gold, requires_grad=True)
    hid64 = U.deberta_model(P64, ids, mask, drop=drop)
    pooled64 = U.plm_pooler(P64, hid64)
    ((hid64 * a).sum() + (pooled64 * b).sum()).backward()
    tag = "%s %s" % (gemm_prec, "train" if train else "eval")
    if not train:        # dropouts 0: the composition is the golden's model
        assert (hid64.detach() - torch.from_numpy(gold["last_hidden_state"])).abs().max() < 1e-12
    for name, got, want in (("last_hidden_state", out.last_hidden_state, hid64), ("pooled", pooled, pooled64)):
        err = (got.detach().cpu().double() - want.detach()).abs().max().item()
        print("deb-model %s %s: err %.3e (max %.3e)" % (tag, name, err, want.detach().abs().max().item()))
        assert err <= 1e-4, name
    ps = {n_: p for n_, p in model.named_parameters()}
    ps.update({"pooler.0.weight": pooler.weight, "pooler.0.bias": pooler.bias})
    assert set(ps) == set(P64)
    worst = 0.0
    for name, p64 in P64.items():
        want = p64.grad.clone()
        assert ps[name].grad is not None, name
        scale = want.abs().max().item()
        assert scale > 0, name
        err = (ps[name].grad.detach().cpu().double() - want).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 1e-3 * scale, (name, err, scale)
    print("deb-model %s: worst gradient error / max %.3e over %d tensors" % (tag, worst, len(P64)))
    for key in ("encoder.rel_embeddings.weight", "encoder.layer.0.attention.self.q_bias",
                "encoder.layer.1.attention.self.v_bias"):
        assert key in P64
    K_, gr = c.max_position_embeddings, ps["encoder.rel_embeddings.weight"].grad
    assert (gr[:K_ - L] == 0).all() and (gr[K_ + L:] == 0).all()       # only rows K - L .. K + L - 1 receive any


def test_two_segments_equal_two_passes(gold):
    """encode_segments over two segments of different L = each segment alone (eval; float32 re-association of the
    GEMMs over other row counts only)."""
    model, _ = _golden_model(gold, 0.0)
    model.eval()
    ids, mask = torch.from_numpy(gold["ids"]).cuda(), torch.from_numpy(gold["mask"]).cuda()
    with torch.no_grad():
        one = model(ids, mask).last_hidden_state
        two = model(ids[:3, :5].contiguous(), mask[:3, :5].contiguous()).last_hidden_state
        o1, o2 = model.encode_segments([(ids, mask), (ids[:3, :5].contiguous(), mask[:3, :5].contiguous())])
    torch.testing.assert_close(o1.last_hidden_state, one, rtol=0, atol=1e-5)
    torch.testing.assert_close(o2.last_hidden_state, two, rtol=0, atol=1e-5)


# ---------------------------------------------------------------------- PLM

B_, C_, N_, L_, V_ = 2, 3, 4, 7, 64


def _plm(gold, p=0.0):
    from newsrec_amd import encoders as E
    from newsrec_amd.manager import ManagerConfig
    from newsrec_amd.xformer import PLM
    H = int(gold["meta.config"][1])
    torch.manual_seed(5)
    m = ManagerConfig("bert", "attn", H, bert_dim=H, signal_length=L_, his_size=N_, npratio=C_ - 1, bert="deberta")
    model = PLM(m, E.Attention_Pooling(m), bert_config=_config(gold, p))
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if p_.dim() == 2 and "embeddings" not in n and ("bert" in n or "pooler" in n):
                p_.normal_(0, 1.2 / p_.shape[1] ** 0.5)
            elif "rel_embeddings" in n or "word_embeddings" in n:
                p_.normal_(0, 0.5)
    return m, model.cuda()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)

    def titles(n):
        t = torch.randint(1, V_, (n, L_), generator=g)
        lens = torch.randint(1, L_ + 1, (n,), generator=g)
        msk = (torch.arange(L_)[None] < lens[:, None]).long()
        return t * msk, msk
    ct, cm = titles(B_ * C_)
    ht, hm = titles(B_ * N_)
    return {"cdd_encoded_index": ct.view(B_, C_, L_), "cdd_attn_mask": cm.view(B_, C_, L_),
            "his_encoded_index": ht.view(B_, N_, L_), "his_attn_mask": hm.view(B_, N_, L_),
            "his_mask": torch.ones(B_, N_, 1, dtype=torch.float64), "his_id": torch.arange(1, 1 + B_ * N_).view(B_, N_),
            "user_id": torch.tensor([1, 2]), "label": torch.tensor([0, 2])}


def test_plm_fused_pass_equals_the_unfused_towers(gold):
    from newsrec_amd import _lib as Lb
    from newsrec_amd.deberta import DebertaModel
    m, model = _plm(gold)
    assert m.name == model.name == "plm__deberta__attn" and isinstance(model.bert, DebertaModel)
    model.eval()
    x = {k: v.cuda() for k, v in _batch(1).items()}
    H = model.bert.config.hidden_size
    with torch.no_grad():
        logits, _ = model(x)
        cdd = model.encode_news(x)
        user, _ = model.encode_user(x)
        by_hand = model.compute_score(cdd, user, Lb.SCORE_SIGMOID)
        # the same again through model.bert and model.pooler themselves
        hid = model.bert(x["his_encoded_index"].view(-1, L_), x["his_attn_mask"].view(-1, L_)).last_hidden_state
        his = model.pooler(hid[:, 0])
        user2 = model.encoderU(his.view(B_, N_, -1), his_mask=x["his_mask"]) + model.userBias
    # not a comparison between constants: the sigmoid scores spread over 100x the bar below
    assert logits.shape == (B_, C_) and logits.std().item() > 1e-3
    # the same arithmetic over other row counts: a GEMM may take another tiling or K split, so the bar is
    # float32 re-association through 2 layers of O(1) values (a few 1e-6), not bit equality
    torch.testing.assert_close(logits, by_hand, rtol=0, atol=1e-5)
    torch.testing.assert_close(user2, user, rtol=0, atol=1e-5)
    # the history read from an installed news table (PLM.py:95-97)
    table = torch.zeros(1 + B_ * N_, H, device="cuda")
    table[1:] = his
    model.init_embedding(table)
    with torch.no_grad():
        user3, _ = model.encode_user(x)
        logits3, _ = model(x)
    model.destroy_embedding()
    torch.testing.assert_close(user3, user, rtol=0, atol=1e-5)
    torch.testing.assert_close(logits3, logits, rtol=0, atol=1e-5)


def test_plm_train_step_runs(gold):
    from newsrec_amd.manager import get_optim, train_step
    _, model = _plm(gold, 0.1)
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
    for key in ("in_proj.weight", "pos_proj.weight", "pos_q_proj.weight", "pos_q_proj.bias", "q_bias", "v_bias",
                "rel_embeddings.weight", "pooler.0.weight", "pooler.0.bias", "query_news", "userBias"):
        assert any(key in n for n in moved), key


def test_plm_graph_replay_matches_eager(gold):
    """bench.GraphedStep on the DeBERTa PLM: 2 eager warm-up steps + 2 replays vs 4 eager steps, within the bars
    of test_fullsize_gpu.py's replay test."""
    import bench
    from newsrec_amd.manager import get_optim
    _, m_eager = _plm(gold, 0.1)
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
