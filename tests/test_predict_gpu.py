"""prediction.txt on the device (csrc/predict.hip, evaluate.rank_ordinal / format_predictions /
write_predictions / test) against the definition, bit for bit:

  ranks   ss.rankdata(1 - np.asarray(p.tolist()), method="ordinal") per impression (the stable argsort
          of the f64 key where scipy is missing), over group sizes around every wave multiple and
          score families with distinct values, heavy ties, 1 - p key collisions and special values
  text    str(index) + " [" + ",".join(str(r) ...) + "]\\n" per impression, line numbers crossing digit
          boundaries, empty groups first / middle / last, G = 0
  slabs   write_predictions with several slab sizes gives the same file
  errors  NaN scores, groups above the cap, wrong dtypes, non-contiguous inputs
  e2e     evaluate.test on the synthetic test split equals the lines built from eval_fast's scores
  golden  tests/golden/prediction_ref.npz (written with scipy) on a machine without scipy
"""
import os

import numpy as np
import pytest
import torch

import predict_util as PU
from mind_util import load_data

pytestmark = pytest.mark.gpu

DEV = "cuda"
FAMILIES = ("distinct", "ties", "sigmoid12", "special")
FIXED = [0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1025]


def _sizes():
    r = np.random.default_rng(7).integers(1, 301, 200).tolist()
    return FIXED + r[:100] + [0] + r[100:] + [0]          # empty groups: first, middle, last


def _scores(family, sizes, rng):
    n = int(sum(sizes))
    if family == "distinct":
        return rng.permutation(np.linspace(0.001, 0.999, n)).astype(np.float32)
    if family == "ties":
        return rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 0.9], np.float32), n)
    logits = rng.normal(0.0, 12.0, n).astype(np.float32)
    p = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
    if family == "special":
        # every group of 7 or more holds 0.0, -0.0, 1.0, 1.5, -2.0, inf, -inf at random positions
        special = np.array([0.0, -0.0, 1.0, 1.5, -2.0, np.inf, -np.inf], np.float32)
        o = 0
        for s in sizes:
            if s >= 7:
                p[o + rng.choice(s, 7, replace=False)] = special
            o += s
    return p


@pytest.fixture(scope="module")
def cases():
    """family -> (preds fp32, offsets, expected rank lists); built once, never modified."""
    sizes = _sizes()
    off = PU.offsets(sizes)
    out = {}
    for k, fam in enumerate(FAMILIES):
        p = _scores(fam, sizes, np.random.default_rng(100 + k))
        out[fam] = (p, off, PU.group_ranks(p, off))
    return out


def _dev(p, off):
    return torch.from_numpy(p).to(DEV), torch.from_numpy(off).to(DEV)


def _text(t):
    return bytes(t.cpu().numpy().tobytes()).decode("ascii")


@pytest.mark.parametrize("family", FAMILIES)
def test_ranks_match_definition(cases, family):
    from newsrec_amd.evaluate import rank_ordinal
    p, off, want = cases[family]
    rank, line_len = rank_ordinal(*_dev(p, off), first_line=1)
    assert rank.dtype == torch.int32 and line_len.dtype == torch.int64
    got = rank.cpu().numpy()
    for g, w in enumerate(want):
        np.testing.assert_array_equal(got[off[g]:off[g + 1]], np.asarray(w, np.int64), err_msg="group %d" % g)
    assert line_len.cpu().tolist() == [len(s) for s in PU.lines(want, 1)]


def test_sigmoid_family_has_key_collisions(cases):
    """The family is there for the 1 - p collisions: a descending-fp32-score order must differ."""
    p, off, want = cases["sigmoid12"]
    differ = 0
    for g, w in enumerate(want):
        x = p[off[g]:off[g + 1]]
        naive = np.empty(len(x), np.int64)
        naive[np.argsort(-x.astype(np.float64), kind="stable")] = np.arange(1, len(x) + 1)
        differ += naive.tolist() != w
    assert differ > 0


def test_collision_vector():
    from newsrec_amd.evaluate import format_predictions, rank_ordinal
    p, off = _dev(PU.COLLISION, np.array([0, 6], np.int64))
    rank, line_len = rank_ordinal(p, off)
    assert rank.cpu().tolist() == PU.COLLISION_RANKS == [5, 6, 3, 4, 1, 2]
    assert line_len.cpu().tolist() == [len("1 [5,6,3,4,1,2]\n")]
    assert _text(format_predictions(p, off)) == "1 [5,6,3,4,1,2]\n"


def test_special_values_group():
    from newsrec_amd.evaluate import rank_ordinal
    x = np.array([0.0, -0.0, 1.0, 1.5, -2.0, np.inf, -np.inf], np.float32)
    rank, _ = rank_ordinal(*_dev(x, np.array([0, 7], np.int64)))
    assert rank.cpu().tolist() == [int(r) for r in PU.ranks_expected(x)] == [4, 5, 3, 2, 6, 1, 7]


@pytest.mark.parametrize("first_line", [1, 9, 99, 999_999])
def test_format_matches_python(cases, first_line):
    from newsrec_amd.evaluate import format_predictions, rank_ordinal
    for family in FAMILIES:
        p, off, want = cases[family]
        ls = PU.lines(want, first_line)
        dp, doff = _dev(p, off)
        assert _text(format_predictions(dp, doff, first_line)) == "".join(ls), family
        _, line_len = rank_ordinal(dp, doff, first_line)
        assert line_len.cpu().tolist() == [len(s) for s in ls], family


def test_format_rank_digit_boundaries(cases):
    """The 1025-candidate group's ranks cross 9/10, 99/100 and 999/1000; its line alone."""
    from newsrec_amd.evaluate import format_predictions
    p, off, want = cases["distinct"]
    g = FIXED.index(1025)
    x = p[off[g]:off[g + 1]]
    assert sorted(want[g]) == list(range(1, 1026))
    got = _text(format_predictions(*_dev(x, np.array([0, 1025], np.int64)), first_line=3))
    assert got == PU.lines([want[g]], 3)[0]


def test_format_empty_inputs():
    from newsrec_amd.evaluate import format_predictions, rank_ordinal
    none = torch.empty(0, dtype=torch.float32, device=DEV)
    t = format_predictions(none, torch.zeros(1, dtype=torch.int64, device=DEV))
    assert t.dtype == torch.uint8 and t.numel() == 0 and t.is_cuda
    rank, line_len = rank_ordinal(none, torch.zeros(1, dtype=torch.int64, device=DEV))
    assert rank.numel() == 0 and line_len.numel() == 0
    # only empty groups
    assert _text(format_predictions(none, torch.zeros(4, dtype=torch.int64, device=DEV), 9)) == "9 []\n10 []\n11 []\n"


def test_format_entry_rejects_bad_arguments():
    from newsrec_amd import _lib as L
    rank = torch.ones(3, dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 3], dtype=torch.int64, device=DEV)
    loff = torch.tensor([0, 10], dtype=torch.int64, device=DEV)
    text = torch.zeros(16, dtype=torch.uint8, device=DEV)
    P, S = L.ptr, L.stream_ptr(rank)
    lib = L.load()
    assert lib.nr_format_prediction(P(rank), P(off), P(loff), 0, 1, P(text), 0, S) == 0        # G == 0: no launch
    assert lib.nr_format_prediction(P(rank), P(off), P(loff), -1, 1, P(text), 16, S) == -1000
    assert lib.nr_format_prediction(P(rank), P(off), P(loff), 1, 1, P(text), -1, S) == -1000
    assert lib.nr_format_prediction(P(rank), None, P(loff), 1, 1, P(text), 16, S) == -1001
    assert lib.nr_format_prediction(P(rank), P(off), None, 1, 1, P(text), 16, S) == -1001
    assert lib.nr_format_prediction(P(rank), P(off), P(loff), 1, 1, None, 16, S) == -1001
    assert lib.nr_format_prediction(P(rank), P(off), P(loff), 1, 1, P(text), 4, S) == -1003    # < "N []\n"
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ll = torch.zeros(1, dtype=torch.int64, device=DEV)
    pr = torch.zeros(3, dtype=torch.float32, device=DEV)
    assert lib.nr_rank_ordinal(P(pr), P(off), 0, 1, 0, P(rank), P(ll), P(st), S) == 0
    assert lib.nr_rank_ordinal(P(pr), P(off), -1, 1, 3, P(rank), P(ll), P(st), S) == -1000
    assert lib.nr_rank_ordinal(P(pr), None, 1, 1, 3, P(rank), P(ll), P(st), S) == -1001
    assert lib.nr_rank_ordinal(None, P(off), 1, 1, 3, P(rank), P(ll), P(st), S) == -1001
    assert lib.nr_rank_ordinal(P(pr), P(off), 1, 1, 3, P(rank), P(ll), None, S) == -1001
    assert lib.nr_rank_ordinal(P(pr), P(off), 1, 1, L.RANK_MAX_GROUP + 1, P(rank), P(ll), P(st), S) == -1002
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(text.sum().item()) == 0


def test_format_stops_at_text_bytes():
    """A text_bytes smaller than the lines need: nothing is stored at or past it."""
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import rank_ordinal
    p, off = _dev(np.linspace(0.1, 0.9, 40).astype(np.float32), np.array([0, 20, 40], np.int64))
    rank, line_len = rank_ordinal(p, off)
    loff = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(line_len, 0)])
    total = int(loff[-1].item())
    want = "".join(PU.lines(PU.group_ranks(p.cpu().numpy(), off.cpu().numpy()), 1))
    assert total == len(want)
    for cut in (total - 1, total - 7, int(loff[1].item()) + 2, 11):
        text = torch.full((total + 8,), 255, dtype=torch.uint8, device=DEV)
        L.call("nr_format_prediction", L.ptr(rank), L.ptr(off), L.ptr(loff), 2, 1, L.ptr(text), cut, L.stream_ptr(rank))
        got = text.cpu().numpy()
        assert bytes(got[:cut].tobytes()).decode("ascii") == want[:cut] and (got[cut:] == 255).all(), cut


def test_unaligned_text_buffer(cases):
    """Lines start at every byte phase of the destination: the same text at base offsets 1, 2, 3."""
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import rank_ordinal
    p, off, want = cases["ties"]
    dp, doff = _dev(p, off)
    rank, line_len = rank_ordinal(dp, doff)
    loff = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(line_len, 0)])
    total = int(loff[-1].item())
    expect = "".join(PU.lines(want, 1))
    for shift in (1, 2, 3):
        buf = torch.full((total + 8,), 255, dtype=torch.uint8, device=DEV)
        text = buf[shift:shift + total]
        L.call("nr_format_prediction", L.ptr(rank), L.ptr(doff), L.ptr(loff), len(want), 1, L.ptr(text), total,
               L.stream_ptr(rank))
        got = buf.cpu().numpy()
        assert bytes(got[shift:shift + total].tobytes()).decode("ascii") == expect
        assert (got[:shift] == 255).all() and (got[shift + total:] == 255).all()


def test_write_predictions_slabs(cases, tmp_path):
    from newsrec_amd.evaluate import write_predictions
    p, off, want = cases["sigmoid12"]
    expect = "".join(PU.lines(want, 1)).encode("ascii")
    dp, doff = _dev(p, off)
    for name, kw in (("default", {}), ("s64", {"slab_bytes": 64}), ("s4096", {"slab_bytes": 4096})):
        path = str(tmp_path / name / "deeper" / "prediction.txt")      # the parent directory is created
        n = write_predictions(path, dp, doff, **kw)
        assert n == os.path.getsize(path) == len(expect), name
        with open(path, "rb") as f:
            assert f.read() == expect, name


def test_nan_raises_before_the_file_exists(cases, tmp_path):
    from newsrec_amd.evaluate import format_predictions, rank_ordinal, write_predictions
    p, off, _ = cases["distinct"]
    p = p.copy()
    p[int(off[-2]) - 3] = np.nan
    dp, doff = _dev(p, off)
    path = str(tmp_path / "nan" / "prediction.txt")
    with pytest.raises(ValueError, match="NaN"):
        write_predictions(path, dp, doff)
    assert not os.path.exists(path)
    with pytest.raises(ValueError, match="NaN"):
        rank_ordinal(dp, doff)
    with pytest.raises(ValueError, match="NaN"):
        format_predictions(dp, doff)


def test_group_above_cap_raises():
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import rank_ordinal
    assert L.RANK_MAX_GROUP >= 4096
    n = L.RANK_MAX_GROUP + 1
    p = torch.rand(n + 5, device=DEV)
    off = torch.tensor([0, 5, n + 5], dtype=torch.int64, device=DEV)
    with pytest.raises(L.HipError):
        rank_ordinal(p, off)
    # an understated max_group: the launch flags the group instead of ranking it
    rank = torch.zeros(n + 5, dtype=torch.int32, device=DEV)
    ll = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("nr_rank_ordinal", L.ptr(p), L.ptr(off), 2, 1, 5, L.ptr(rank), L.ptr(ll), L.ptr(st), L.stream_ptr(p))
    assert int(st.item()) == L.RANK_GROUP_TOO_LARGE
    assert sorted(rank[:5].cpu().tolist()) == [1, 2, 3, 4, 5] and int(rank[5:].abs().sum().item()) == 0


def test_group_at_cap():
    """The largest admitted group, with every score equal (ranks follow position: 1 .. cap)."""
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import rank_ordinal
    n = L.RANK_MAX_GROUP
    p = torch.full((n,), 0.5, device=DEV)
    rank, line_len = rank_ordinal(p, torch.tensor([0, n], dtype=torch.int64, device=DEV))
    assert torch.equal(rank.cpu(), torch.arange(1, n + 1, dtype=torch.int32))
    assert int(line_len.item()) == len(PU.lines([list(range(1, n + 1))], 1)[0])


def test_argument_checks():
    from newsrec_amd import _lib as L
    from newsrec_amd.evaluate import format_predictions, rank_ordinal, write_predictions
    p = torch.rand(8, device=DEV)
    off = torch.tensor([0, 3, 8], dtype=torch.int64, device=DEV)
    for fn in (rank_ordinal, format_predictions):
        with pytest.raises(L.HipError):
            fn(p.double(), off)
        with pytest.raises(L.HipError):
            fn(p, off.to(torch.int32))
        with pytest.raises(L.HipError):
            fn(torch.rand(16, device=DEV)[::2], off)
        with pytest.raises(L.HipError):
            fn(p, torch.tensor([0, 0, 3, 3, 8, 8], dtype=torch.int64, device=DEV)[::2])
        with pytest.raises(L.HipError):
            fn(p.cpu(), off)
        with pytest.raises(L.HipError):
            fn(p.view(2, 4), off)
    with pytest.raises(L.HipError):
        write_predictions("unused", p.double(), off)
    for bad in ([0, 3, 7], [1, 3, 8], [0, 5, 3, 8]):                   # not CSR offsets over the 8 scores
        with pytest.raises(ValueError):
            rank_ordinal(p, torch.tensor(bad, dtype=torch.int64, device=DEV))
    assert not os.path.exists("unused")


def _small_model(H=384, encN="mha", encU="mha"):
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


@pytest.mark.parametrize("encN,encU,H", [("mha", "mha", 384), ("cnn", "attn", 150)])
def test_end_to_end_prediction_file(tmp_path, encN, encU, H):
    from newsrec_amd import evaluate
    data = load_data()
    st = _store(data, "test")
    assert len(st) > len(st.grp_off_host) - 1          # impressions are cut into chunks by impr_size
    model = _small_model(H, encN, encU)
    path = str(tmp_path / "results" / "prediction.txt")
    assert evaluate.test(model, st, path, batch_impr=3) == path
    preds, labels, grp = evaluate.eval_fast(model, st, batch_impr=3)
    assert labels is None
    go = st.grp_off_host
    want = "".join(PU.lines(PU.group_ranks(preds.cpu().numpy(), go), 1))
    with open(path, "rb") as f:
        assert f.read().decode("ascii") == want
    assert want.count("\n") == len(go) - 1 and want.startswith("1 [")
    # a dev store is accepted, a train store is not
    dpath = str(tmp_path / "dev.txt")
    assert evaluate.test(model, _store(data, "dev"), dpath) == dpath and os.path.getsize(dpath) > 0
    with pytest.raises(ValueError):
        evaluate.test(model, _store(data, "train"), str(tmp_path / "train.txt"))
    assert not os.path.exists(str(tmp_path / "train.txt"))


def test_golden_text():
    from newsrec_amd.evaluate import format_predictions
    z = np.load(PU.GOLDEN)
    got = format_predictions(*_dev(z["preds"], z["grp_off"]), first_line=int(z["first_line"]))
    np.testing.assert_array_equal(got.cpu().numpy(), z["text"])
