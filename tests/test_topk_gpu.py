"""Full-corpus top-K retrieval on the device (csrc/topk.hip, evaluate.topk_news / recommend /
recall_metrics) against the definition in topk_util:

  exact      integer-valued inputs (every partial sum exact in fp32): ids and score BITS equal the
             oracle's, over user / news / K / H sizes on both sides of every tile boundary, with heavy
             ties and duplicated rows, and an identity user matrix against an asymmetric table (the
             MFMA lane maps)
  geometry   n_slices 1, 2, 7 and automatic give the same bits on real-valued data
  real       randn inputs: the property check of topk_util (tolerance derived there)
  eligible   first_row, row_mask, exclude (padding, repeats, whole lists), strides, odd alignment
  errors     non-finite scores, every invalid-argument code, wrapper argument checks
  e2e        recommend / recall_metrics on the synthetic split for two model families
"""
import numpy as np
import pytest
import torch

import topk_util as TU
from mind_util import load_data

pytestmark = pytest.mark.gpu

DEV = "cuda"
US, NS, KS, HS = (1, 63, 64, 65, 129), (1, 9, 127, 128, 129, 1000), (1, 10, 64, 100, 128), (1, 2, 7, 64, 150)


def _exact_cases():
    """(U, N, K, H, first_row): every (U, N) pair once (30 cases), every K with every U, every H with
    every N; then K == N, K > N and the largest of everything."""
    out = []
    for i in range(30):
        out.append((US[i % 5], NS[i % 6], KS[(i + i // 5) % 5], HS[(i + i // 6) % 5], i % 2))
    out += [(64, 128, 128, 64, 0), (65, 9, 10, 7, 0), (1, 1, 1, 1, 1), (129, 1000, 128, 150, 1), (63, 129, 128, 2, 1)]
    return out


def _ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _run(table, user, k, **kw):
    from newsrec_amd.evaluate import topk_news
    t = {n: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v)
         for n, v in kw.items()}
    ids, sc = topk_news(torch.from_numpy(table).to(DEV), torch.from_numpy(user).to(DEV), k, **t)
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    return ids.cpu().numpy(), sc.cpu().numpy()


def _same_bits(got, want):
    ids, sc = got
    wi, ws = want
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(sc.view(np.int32), ws.view(np.int32))


def test_exact_cases_cover_every_size():
    c = _exact_cases()
    for col, vals in enumerate((US, NS, KS, HS)):
        assert {x[col] for x in c} == set(vals)
    assert {(x[0], x[2]) for x in c} >= {(u, k) for u in US for k in KS}
    assert any(x[2] > x[1] for x in c) and any(x[2] == x[1] for x in c)


@pytest.mark.parametrize("U,N,K,H,first_row", _exact_cases())
def test_exact_family(U, N, K, H, first_row):
    rng = np.random.default_rng(1000 * U + N + K + H)
    table, user = _ints(rng, (N, H)), _ints(rng, (U, H))
    _same_bits(_run(table, user, K, first_row=first_row), TU.expected(table, user, K, first_row))


@pytest.mark.parametrize("n_slices", [0, 1, 7])
def test_ties_follow_ascending_id(n_slices):
    """Entries in {-1, 0, 1} at H = 8 (a handful of distinct scores) and the second half of the table a
    copy of the first: equal scores on both sides of every 128-row tile and of every slice."""
    rng = np.random.default_rng(5)
    half = _ints(rng, (500, 8), -1, 1)
    table, user = np.concatenate([half, half]), _ints(rng, (65, 8), -1, 1)
    want = TU.expected(table, user, 100)
    assert (np.diff(want[1], axis=1) == 0).mean() > 0.8            # mostly ties
    _same_bits(_run(table, user, 100, n_slices=n_slices), want)


def test_identity_users_asymmetric_table():
    """user = I: score[i][j] = table[j][i] * scale.  A swapped operand or output map would return
    table[i][j]-shaped results; the table is far from symmetric."""
    H = 64
    j, k = np.meshgrid(np.arange(128), np.arange(H), indexing="ij")
    table = ((j * 7 + k * k * 3 + (k > j) * 5) % 23 - 11).astype(np.float32)
    assert (table[:H] != table[:H].T).mean() > 0.5
    user = np.eye(H, dtype=np.float32)
    _same_bits(_run(table, user, 128, first_row=0), TU.expected(table, user, 128, 0))


@pytest.fixture(scope="module")
def real():
    """H -> (table [1000, H], user [65, H]) randn; built once, never modified."""
    rng = np.random.default_rng(17)
    return {H: (rng.standard_normal((1000, H)).astype(np.float32), rng.standard_normal((65, H)).astype(np.float32))
            for H in (150, 384)}


def test_geometry_independence(real):
    table, user = real[150]
    base = _run(table, user, 100, n_slices=1)
    for ns in (2, 7, 0):
        _same_bits(_run(table, user, 100, n_slices=ns), base)
    TU.check_properties(table, user, base[0], base[1], 100)


@pytest.mark.parametrize("H", [150, 384])
@pytest.mark.parametrize("K", [10, 128])
def test_real_family_properties(real, H, K):
    table, user = real[H]
    ids, sc = _run(table, user, K)
    TU.check_properties(table, user, ids, sc, K)


@pytest.mark.parametrize("first_row", [0, 1])
@pytest.mark.parametrize("E", [1, 50, 256])
def test_mask_and_exclude(first_row, E):
    rng = np.random.default_rng(100 + E)
    N, U, K, H = 300, 65, 64, 7
    table, user = _ints(rng, (N, H)), _ints(rng, (U, H))
    top = TU.expected(table, user, 128, first_row)[0]
    ex = np.full((U, E), -1, np.int64)
    ex[:, 0] = top[:, 0]                                     # the row that would be first
    if E > 1:
        ex[:, 1] = N                                         # padding on the other side
        ex[:, 2] = top[:, 0]                                 # a repeat
        ex[:, 3:E // 2] = top[:, 1:E // 2 - 2]               # more of the best rows
        ex[::2, E // 2:] = rng.integers(0, N, (len(ex[::2]), E - E // 2))
    _same_bits(_run(table, user, K, first_row=first_row, exclude=ex), TU.expected(table, user, K, first_row, None, ex))
    # a mask that leaves fewer than K rows, with and without the exclude list
    mask = (rng.random(N) < 0.1).astype(np.uint8)
    mask[:3] = 1
    assert 3 < mask.sum() < K
    _same_bits(_run(table, user, K, first_row=first_row, row_mask=mask), TU.expected(table, user, K, first_row, mask))
    got = _run(table, user, K, first_row=first_row, row_mask=mask, exclude=ex)
    _same_bits(got, TU.expected(table, user, K, first_row, mask, ex))
    assert (got[0][:, -1] == -1).all() and np.isneginf(got[1][:, -1]).all()


def test_user_with_every_eligible_row_excluded():
    rng = np.random.default_rng(3)
    N, U, K, H = 200, 5, 10, 64
    table, user = _ints(rng, (N, H)), _ints(rng, (U, H))
    mask = np.zeros(N, np.uint8)
    keep = np.array([0, 5, 130, 131, 199])
    mask[keep] = 1
    ex = np.full((U, 6), -1, np.int64)
    ex[2, :5] = keep                                         # user 2: nothing left
    ex[3, :2] = (5, 199)
    ids, sc = _run(table, user, K, first_row=1, row_mask=mask, exclude=ex)
    _same_bits((ids, sc), TU.expected(table, user, K, 1, mask, ex))
    assert (ids[2] == -1).all() and np.isneginf(sc[2]).all()
    assert sorted(ids[3][:2].tolist()) == [130, 131] and (ids[3][2:] == -1).all()
    assert sorted(ids[0][:4].tolist()) == [5, 130, 131, 199]


def test_strides_and_alignment():
    from newsrec_amd.evaluate import topk_news
    rng = np.random.default_rng(8)
    N, U, K, H = 260, 70, 10, 64
    table, user = _ints(rng, (N, H)), _ints(rng, (U, H))
    want = TU.expected(table, user, K)
    # column slices of wider tensors: odd leading dimensions, then 16-byte rows at a 16-byte offset
    for toff, tw, uoff, uw in ((3, H + 5, 4, H + 8), (4, H + 8, 8, H + 12)):
        wt = torch.from_numpy(_ints(rng, (N, tw))).to(DEV)
        wu = torch.from_numpy(_ints(rng, (U, uw))).to(DEV)
        wt[:, toff:toff + H] = torch.from_numpy(table).to(DEV)
        wu[:, uoff:uoff + H] = torch.from_numpy(user).to(DEV)
        t, u = wt[:, toff:toff + H], wu[:, uoff:uoff + H]
        assert t.stride(0) == tw and u.stride(0) == uw and t.stride(1) == 1
        ids, sc = topk_news(t, u, K)
        _same_bits((ids.cpu().numpy(), sc.cpu().numpy()), want)
    # dense rows from a base pointer that is 4-byte but not 16-byte aligned
    flat_t = torch.zeros(N * H + 4, dtype=torch.float32, device=DEV)
    flat_u = torch.zeros(U * H + 4, dtype=torch.float32, device=DEV)
    t2, u2 = flat_t[1:1 + N * H].view(N, H), flat_u[3:3 + U * H].view(U, H)
    t2.copy_(torch.from_numpy(table))
    u2.copy_(torch.from_numpy(user))
    assert t2.data_ptr() % 16 == 4 and u2.data_ptr() % 16 == 12
    ids, sc = topk_news(t2, u2, K)
    _same_bits((ids.cpu().numpy(), sc.cpu().numpy()), want)


def _raw(lib, L, table, user, K, ids, sc, st, ws=None, ws_bytes=0, N=None, U=None, H=None, ldt=None, ldu=None,
         first_row=1, mask=None, ex=None, E=0, n_slices=1):
    P = L.ptr
    return lib.nr_topk_news(P(table), table.stride(0) if ldt is None else ldt, table.shape[0] if N is None else N,
                            P(user), user.stride(0) if ldu is None else ldu, user.shape[0] if U is None else U,
                            table.shape[1] if H is None else H, K, first_row, P(mask), P(ex), E, n_slices, P(ids), P(sc),
                            P(ws), ws_bytes, P(st), L.stream_ptr(table))


def test_non_finite_scores_and_guards():
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import topk_news
    rng = np.random.default_rng(21)
    N, U, K, H = 300, 65, 10, 150
    table = rng.standard_normal((N, H)).astype(np.float32)
    user = rng.standard_normal((U, H)).astype(np.float32)
    table[137, 5] = np.inf
    t, u = torch.from_numpy(table).to(DEV), torch.from_numpy(user).to(DEV)
    with pytest.raises(ValueError, match="non-finite"):
        topk_news(t, u, K)
    # excluded from the search, the row is no error
    mask = torch.ones(N, dtype=torch.uint8, device=DEV)
    mask[137] = 0
    ids, sc = topk_news(t, u, K, row_mask=mask)
    m = mask.cpu().numpy()
    TU.check_properties(np.where(np.isinf(table), 0, table).astype(np.float32), user, ids.cpu().numpy(),
                        sc.cpu().numpy(), K, 1, m)
    # the raw entry: flag set, NR_OK, and nothing stored outside [U, K] of either output
    lib = L.load()
    G = 256
    for ns in (1, 3):
        gi = torch.full((U * K + 2 * G,), -77, dtype=torch.int64, device=DEV)
        gs = torch.full((U * K + 2 * G,), 123.0, dtype=torch.float32, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        nb = int(lib.nr_topk_workspace(U, N, K, ns))
        ws = torch.zeros(nb // 8, dtype=torch.int64, device=DEV)
        assert _raw(lib, L, t, u, K, gi[G:G + U * K], gs[G:G + U * K], st, ws, nb, n_slices=ns) == 0
        torch.cuda.synchronize()
        assert int(st.item()) == L.TOPK_NONFINITE
        for g, fill in ((gi, -77), (gs, 123.0)):
            g = g.cpu().numpy()
            assert (g[:G] == fill).all() and (g[G + U * K:] == fill).all()
        inner = gi[G:G + U * K].cpu().numpy()
        assert ((inner >= 1) & (inner < N)).all()


def test_entry_rejects_bad_arguments():
    from newsrec_amd import _lib as L
    lib = L.load()
    N, U, K, H = 40, 3, 5, 8
    t = torch.ones(N, H, device=DEV)
    u = torch.ones(U, H, device=DEV)
    ids = torch.full((U, K), -77, dtype=torch.int64, device=DEV)
    sc = torch.full((U, K), 123.0, dtype=torch.float32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(U * 2 * K, dtype=torch.int64, device=DEV)
    ex = torch.zeros(U, 257, dtype=torch.int64, device=DEV)
    r = lambda **kw: _raw(lib, L, t, u, kw.pop("K", K), kw.pop("ids", ids), kw.pop("sc", sc), kw.pop("st", st), **kw)
    assert r(N=-1) == -1000 and r(U=-1) == -1000 and r(H=0) == -1000 and r(E=-1) == -1000
    assert r(first_row=-1) == -1000 and r(n_slices=-1) == -1000 and r(ws_bytes=-1) == -1000
    assert r(K=0) == -1002 and r(K=L.TOPK_MAX_K + 1) == -1002
    assert r(ex=ex, E=L.TOPK_MAX_EXCLUDE + 1) == -1003
    assert r(ldt=H - 1) == -1004 and r(ldu=H - 1) == -1004
    assert r(n_slices=65) == -1005
    assert r(ids=None) == -1001 and r(sc=None) == -1001 and r(st=None) == -1001
    assert _raw(lib, L, t, u, K, ids, sc, st, U=U, N=N, H=H, ldt=H, ldu=H) == 0            # the valid call
    P = L.ptr
    S = L.stream_ptr(t)
    assert lib.nr_topk_news(None, H, N, P(u), H, U, H, K, 1, None, None, 0, 1, P(ids), P(sc), None, 0, P(st), S) == -1001
    assert lib.nr_topk_news(P(t), H, N, None, H, U, H, K, 1, None, None, 0, 1, P(ids), P(sc), None, 0, P(st), S) == -1001
    torch.cuda.synchronize()
    ids.fill_(-77)
    # two slices need U * 2 * K entries of workspace
    assert r(n_slices=2, ws=ws, ws_bytes=U * 2 * K * 8 - 1) == -1006
    assert r(n_slices=2, ws=None, ws_bytes=U * 2 * K * 8) == -1006
    assert r(n_slices=2, ws=ws, ws_bytes=0) == -1006
    # no users: NR_OK with null outputs, nothing launched
    assert lib.nr_topk_news(P(t), H, N, None, H, 0, H, K, 1, None, None, 0, 0, None, None, None, 0, None, S) == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int((ids != -77).sum().item()) == 0
    assert r(n_slices=2, ws=ws, ws_bytes=U * 2 * K * 8) == 0
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == [[1, 2, 3, 4, 5]] * U and int(st.item()) == 0


def test_wrapper_argument_checks():
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import topk_news
    t = torch.rand(40, 8, device=DEV)
    u = torch.rand(3, 8, device=DEV)
    with pytest.raises(L.HipError):
        topk_news(t.double(), u, 5)
    with pytest.raises(L.HipError):
        topk_news(t, u.half(), 5)
    with pytest.raises(L.HipError):
        topk_news(t.cpu(), u, 5)
    with pytest.raises(L.HipError):
        topk_news(t, u.cpu(), 5)
    with pytest.raises(L.HipError):
        topk_news(torch.rand(40, 16, device=DEV)[:, ::2], u, 5)
    with pytest.raises(L.HipError):
        topk_news(t, torch.rand(3, 9, device=DEV), 5)
    for k in (0, -1, L.TOPK_MAX_K + 1):
        with pytest.raises(L.HipError):
            topk_news(t, u, k)
    with pytest.raises(L.HipError):
        topk_news(t, u, 5, row_mask=torch.ones(39, dtype=torch.uint8, device=DEV))
    with pytest.raises(L.HipError):
        topk_news(t, u, 5, row_mask=torch.ones(40, dtype=torch.bool, device=DEV))
    with pytest.raises(L.HipError):
        topk_news(t, u, 5, exclude=torch.zeros(2, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(L.HipError):
        topk_news(t, u, 5, exclude=torch.zeros(3, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(L.HipError):
        topk_news(t, u, 5, exclude=torch.zeros(3, L.TOPK_MAX_EXCLUDE + 1, dtype=torch.int64, device=DEV))
    ids, sc = topk_news(t, u[:0], 5)
    assert ids.shape == (0, 5) and sc.shape == (0, 5)


def test_consistent_with_the_ragged_scorer(real):
    """The same rows through nr_score_ragged (raw logits): another summation order, so within the
    derived tolerance, not bit for bit."""
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import score_ragged, topk_news
    table, user = real[384]
    t, u = torch.from_numpy(table).to(DEV), torch.from_numpy(user).to(DEV)
    K = 10
    ids, sc = topk_news(t, u, K)
    seg = torch.arange(u.shape[0], dtype=torch.int32, device=DEV).repeat_interleave(K)
    other, _ = score_ragged(t, u, ids.reshape(-1), seg, 0, mode=L.SCORE_RAW)
    tol = TU.tolerances(table, user)
    rows = np.repeat(np.arange(user.shape[0]), K)
    bound = tol[rows, ids.cpu().numpy().reshape(-1)]
    assert (np.abs(other.cpu().numpy().astype(np.float64) - sc.cpu().numpy().reshape(-1)) <= bound).all()


def _small_model(H, encN, encU):
    from newsrec_amd.manager import build_model
    torch.manual_seed(11)
    m = build_model(encN, encU, H, vocab=30522, device=DEV, user_num=600, dropout_p=0.2)
    with torch.no_grad():           # spread the scores (reference init gives ~1e-4 spreads)
        for p in m.parameters():
            p.mul_(4.0)
    return m.eval()


def _store(data, split):
    from newsrec_amd.mind import MINDStore
    news, beh, opts = data
    return MINDStore(news, beh[split], split, device=DEV, **opts)


def _users(EV, model, table, st, batch):
    """(user [n_impr, H], history ids [n_impr, his_size]) of every impression's first chunk, the store
    walked in batches of ``batch`` chunks."""
    first = st.first_chunk_host
    users, his = [], []
    for c0 in range(0, len(st), batch):
        b = min(batch, len(st) - c0)
        rows = first[(first >= c0) & (first < c0 + b)] - c0
        if len(rows) == 0:
            continue
        x = st.eval_batch(c0, b)
        r = torch.from_numpy(rows).to(DEV)
        sub = {k: x[k][r] for k in ("impr_index", "user_id", "his_id", "his_mask")}
        users.append(EV.user_reprs(model, table, sub, True).cpu().numpy())
        his.append(sub["his_id"].reshape(len(rows), -1).cpu().numpy())
    return np.concatenate(users), np.concatenate(his)


@pytest.mark.parametrize("encN,encU,H", [("mha", "mha", 384), ("cnn", "attn", 150)])
def test_end_to_end_recommend(encN, encU, H):
    from newsrec_amd import evaluate as EV
    data = load_data()
    st = _store(data, "dev")
    n_impr = len(st.grp_off_host) - 1
    assert n_impr < len(st)                                     # impressions are cut into chunks
    model = _small_model(H, encN, encU)
    table = EV.encode_news_table(model, st)
    tab = table.cpu().numpy()
    cand = np.unique(st.cand_ids.cpu().numpy())
    impressed = np.zeros(tab.shape[0], np.uint8)
    impressed[cand] = 1
    for batch in (len(st), 3):
        user, his = _users(EV, model, table, st, batch)          # computed apart from recommend
        assert user.shape == (n_impr, H)
        for candidates in ("impressed", "all"):
            ids, sc = EV.recommend(model, st, k=10, batch_impr=batch, candidates=candidates, news_table=table)
            assert ids.shape == (n_impr, 10) and sc.shape == (n_impr, 10)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
            if candidates == "impressed":
                assert np.isin(ids[ids >= 0], cand).all()
            assert (ids != 0).all()
            for g in range(n_impr):
                assert not np.isin(ids[g], his[g]).any(), g
            TU.check_properties(tab, user, ids, sc, 10, 1, impressed if candidates == "impressed" else None, his)
    user, his = _users(EV, model, table, st, len(st))
    ids3, sc3 = EV.recommend(model, st, k=10, batch_impr=len(st), exclude_history=False, news_table=table)
    TU.check_properties(tab, user, ids3.cpu().numpy(), sc3.cpu().numpy(), 10, 1, impressed)
    # defaults: the table is encoded inside, the split fits one batch
    ids2, sc2 = EV.recommend(model, st, k=10)
    TU.check_properties(tab, user, ids2.cpu().numpy(), sc2.cpu().numpy(), 10, 1, impressed, his)
    # recall metrics against a numpy recomputation
    top = ids2.cpu().numpy()
    m = EV.recall_metrics(ids2, st, ks=(5, 10))
    lab, cid, go = st.cand_labels.cpu().numpy(), st.cand_ids.cpu().numpy(), st.grp_off_host
    rec, hit = {5: [], 10: []}, {5: [], 10: []}
    for g in range(n_impr):
        clicked = set(cid[go[g]:go[g + 1]][lab[go[g]:go[g + 1]] == 1].tolist())
        if not clicked:
            continue
        for k in (5, 10):
            n = len(clicked & set(top[g, :k].tolist()))
            rec[k].append(n / len(clicked))
            hit[k].append(float(n > 0))
    assert m["n_impr_scored"] == len(rec[5]) > 0
    for k in (5, 10):
        assert m["recall@%d" % k] == round(float(np.mean(rec[k])), 4)
        assert m["hit@%d" % k] == round(float(np.mean(hit[k])), 4)
    with pytest.raises(ValueError):
        EV.recommend(model, _store(data, "train"), k=10)
