"""Global-norm gradient clipping and the non-finite step guard of FusedAdam: nr_grad_norm_multi
against the float64 reference of tests/clip_util.py (value, bit-reproducibility, row flags, the
scale formula), nr_adam_multi_clip against the existing Adam entries at the same scale (bitwise),
and FusedAdam(max_grad_norm=..., skip_nonfinite=...) against torch's clip_grad_norm_ + Adam, over
skipped steps, inside a captured graph and at model level."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clip_util import RTOL, clips, close, norm_ref, read_state, scale_ref
from newsrec_amd import kernels as K

INF, NAN = float("inf"), float("nan")


def _mixed(n, gen):
    """randn with each element's magnitude drawn from {1, 1e-2, 1e-4}."""
    mag = torch.tensor([1.0, 1e-2, 1e-4])[torch.randint(0, 3, (n,), generator=gen)]
    return torch.randn(n, generator=gen) * mag


def _ent(g, flags=None):
    """A norm-only entry: parameter and moments are never read."""
    return (g, g, g, g, 1e-3, 1) + ((flags,) if flags is not None else ())


def _state_of(entries, grad_scale=1.0, max_norm=INF, state=None):
    state = K.clip_state("cuda") if state is None else state
    K.grad_norm_multi(entries, grad_scale, max_norm, state)
    return state


_CACHE = {}


def _grads(name):
    """The gradient lists of the value tests (CUDA tensors), built once and never modified."""
    if name in _CACHE:
        return _CACHE[name]
    gen = torch.Generator().manual_seed(11)
    if name.startswith("n="):
        out = [_mixed(int(name[2:]), gen).cuda()]
    elif name == "unaligned":
        n = 3 * 4096 + 5
        out = [_mixed(n + 1, gen).cuda()[1:]]          # base one element past a 16-B boundary
        assert out[0].data_ptr() % 16 == 4 and out[0].is_contiguous()
    else:   # "list70": 70 ragged tensors and one of 30522 * 3 elements: at least three launches
        sizes = [int(n) for n in torch.randint(1, 9000, (70,), generator=gen)] + [30522 * 3]
        out = [_mixed(n, gen).cuda() for n in sizes]
    _CACHE[name] = out
    return out


VALUE_CASES = ["n=0", "n=1", "n=3", "n=4095", "n=4096", "n=4097", "unaligned", "list70"]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("case", VALUE_CASES)
def test_norm_value(case, grad_scale):
    gs = _grads(case)
    st = read_state(_state_of([_ent(g) for g in gs], grad_scale))
    want = norm_ref(gs, grad_scale)
    print("norm %r reference %r" % (st["norm"], want))
    assert close(st["norm"], want), (st["norm"], want)
    assert st["scale"] == grad_scale and st["nonfinite"] == 0 and st["nonfinite_total"] == 0
    if case == "n=0":
        assert st["norm"] == 0.0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_zero_gradients(grad_scale):
    gs = [torch.zeros(n, device="cuda") for n in (5, 4096, 4097 * 3)]
    for max_norm in (INF, 2.0):
        st = read_state(_state_of([_ent(g) for g in gs], grad_scale, max_norm))
        assert st["norm"] == 0.0 and st["scale"] == grad_scale and st["nonfinite"] == 0


def test_count_zero():
    st = read_state(_state_of([], 0.5, 2.0))
    assert st["norm"] == 0.0 and st["scale"] == 0.5 and st["nonfinite"] == 0


def test_reproducible():
    ents = [_ent(g) for g in _grads("list70")]
    first = _state_of(ents, 0.5, 2.0).cpu()
    for _ in range(4):
        assert torch.equal(_state_of(ents, 0.5, 2.0).cpu(), first)
    assert read_state(first)["scale"] < 0.5           # (it clipped: the scale is a computed number)


def _flagged_table():
    """V = 3001, E = 150 through functions._LocalRowGrad: its dense buffer and per-row flags."""
    if "table" not in _CACHE:
        from newsrec_amd import functions as F
        torch.manual_seed(1)
        V, E = 3001, 150
        table = torch.nn.Parameter(torch.randn(V, E, device="cuda"))
        h = F._LocalRowGrad()
        rows = torch.randint(0, V, (32,), device="cuda")
        assert h(table, rows, torch.randn(32, E, device="cuda"))
        buf, flags, _ = table._nr_row_touched
        assert 0 < int(flags.sum()) <= 32
        _CACHE["table"] = (table, h, buf, flags)
    return _CACHE["table"][2:]


def test_row_flags_local_row_grad():
    buf, flags = _flagged_table()
    with_flags = _state_of([_ent(buf, flags)], 1.0, 2.0).cpu()
    without = _state_of([_ent(buf)], 1.0, 2.0).cpu()
    assert torch.equal(with_flags, without)
    assert close(read_state(with_flags)["norm"], norm_ref([buf]))


@pytest.mark.parametrize("rlen", [1, 2, 3, 5])
def test_row_flags_short_rows(rlen):
    torch.manual_seed(2)
    rows = 4096
    flags = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    flags[1::4] = 1
    g = torch.randn(rows, rlen, device="cuda") * flags[:, None].float()
    with_flags = _state_of([_ent(g, flags)], 1.0, 2.0).cpu()
    without = _state_of([_ent(g)], 1.0, 2.0).cpu()
    assert torch.equal(with_flags, without)
    assert close(read_state(with_flags)["norm"], norm_ref([g]))


def test_unflagged_rows_are_not_read():
    """V = 512, E = 8 on an aligned base: no float4 straddles a row, so rows flagged zero must not be
    loaded at all -- they hold NaN here."""
    torch.manual_seed(3)
    V, E = 512, 8
    flags = (torch.rand(V, device="cuda") < 0.3).to(torch.uint8)
    assert 0 < int(flags.sum()) < V
    g = torch.randn(V, E, device="cuda")
    assert g.data_ptr() % 16 == 0
    want = norm_ref([g[flags.bool()]])
    g[~flags.bool()] = NAN
    st = read_state(_state_of([_ent(g, flags)], 1.0, 2.0))
    assert math.isfinite(st["norm"]) and st["nonfinite"] == 0
    assert close(st["norm"], want), (st["norm"], want)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("max_norm", ["inf", "1e9", "half", "2.0", "0.0"])
def test_scale(max_norm, grad_scale):
    gs = _grads("list70")
    nref = norm_ref(gs, grad_scale)
    mx = 0.5 * nref if max_norm == "half" else float(max_norm)
    st = read_state(_state_of([_ent(g) for g in gs], grad_scale, mx))
    assert close(st["norm"], nref)
    if not clips(st["norm"], mx):
        assert max_norm in ("inf", "1e9")
        assert np.float32(st["scale"]).tobytes() == np.float32(grad_scale).tobytes()
    else:
        assert max_norm in ("half", "2.0", "0.0")
        want = scale_ref(nref, grad_scale, mx)
        print("scale %r reference %r" % (st["scale"], want))
        assert close(st["scale"], want), (st["scale"], want)
        if mx == 0.0:
            assert st["scale"] == 0.0


def _adam_sets(data):
    """(grads, flags) of the clipped-Adam comparison."""
    if data == "list70":
        return _grads("list70"), None
    buf, flags = _flagged_table()
    return [buf], flags


@pytest.mark.parametrize("data", ["list70", "table"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("device_steps", [False, True])
def test_clipped_adam_is_adam_at_that_scale(device_steps, weight_decay, data):
    grads, flags = _adam_sets(data)
    gen = torch.Generator().manual_seed(5)
    p0 = [torch.randn(g.shape, generator=gen).cuda() for g in grads]
    m0 = [(torch.randn(g.shape, generator=gen).abs() * 0.01).cuda() for g in grads]
    v0 = [(torch.randn(g.shape, generator=gen).abs() * 0.001).cuda() for g in grads]
    state = _state_of([_ent(g, flags) for g in grads], 0.5, 0.5 * norm_ref(grads, 0.5))
    s = read_state(state)["scale"]
    assert 0.2 < s < 0.3                               # clipped to half: 0.5 * 0.5
    lr = torch.full((), 1e-3, device="cuda") if device_steps else 1e-3
    outs = []
    for clipped in (False, True):
        p, m, v = ([t.clone() for t in ts] for ts in (p0, m0, v0))
        steps = [torch.full((), 2, dtype=torch.int64, device="cuda") if device_steps else 3 for _ in grads]
        ents = [(pp, g, mm, vv, lr, st) + ((flags,) if flags is not None else ())
                for pp, g, mm, vv, st in zip(p, grads, m, v, steps)]
        for _ in range(2):
            if clipped:
                K.adam_multi_clip(ents, 0.9, 0.999, 1e-8, weight_decay, state, honor_skip=True,
                                  advance_steps=device_steps)
            else:
                K.adam_multi(ents, 0.9, 0.999, 1e-8, weight_decay, float(s), advance_steps=device_steps)
        outs.append((p, m, v, steps))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    if device_steps:
        assert all(int(x) == 4 and int(y) == 4 for x, y in zip(outs[0][3], outs[1][3]))
    assert not torch.equal(outs[1][0][0], p0[0])
    assert K.self_cleaning_check("cuda") == []


def _assign(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.clone().to(p.device)


def test_torch_parity():
    from newsrec_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(0)
    shapes = [(1000, 77), (3,), (4097,)]
    ps = [torch.randn(s, generator=gen) for s in shapes]
    # |g| ~ 285 * 10^-k: steps k = 0, 1, 2 clip at 2.0, step k = 3 does not
    gs = [[torch.randn(s, generator=gen) * 10.0 ** -k for s in shapes] for k in range(4)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [p.clone().cuda().requires_grad_(True) for p in ps]
    o1 = torch.optim.Adam(ref, lr=1e-3)
    o2 = FusedAdam(mine, lr=1e-3, max_grad_norm=2.0)
    norms = []
    for step in range(4):
        _assign(ref, gs[step])
        _assign(mine, gs[step])
        kept = [q.grad.clone() for q in mine]
        torch.nn.utils.clip_grad_norm_(ref, 2.0)
        o1.step()
        o2.step()
        st = o2.clip_stats()
        norms.append(st["norm"])
        assert close(st["norm"], norm_ref(gs[step]))
        assert float(o2.grad_norm) == st["norm"] and o2.grad_norm.is_cuda and o2.grad_norm.dim() == 0
        for q, k in zip(mine, kept):                   # step() never writes a gradient
            assert torch.equal(q.grad, k)
    assert any(n + 1e-6 > 2.0 for n in norms) and any(n + 1e-6 < 2.0 for n in norms), norms
    for p, q in zip(ref, mine):
        torch.testing.assert_close(q.detach().cpu(), p.detach(), rtol=0, atol=1e-6)


def _opt_snapshot(opt, params):
    """Parameters, moments, step counts (clones / ints) of an optimizer."""
    out = []
    for p in params:
        st = opt.state[p]
        step = st["step"]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                    int(step.item()) if torch.is_tensor(step) else int(step)))
    return out


def _same(a, b):
    for (p, m, v, s), (p2, m2, v2, s2) in zip(a, b):
        if not (torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2) and s == s2):
            return False
    return True


@pytest.mark.parametrize("bad", ["inf_last", "nan_first"])
@pytest.mark.parametrize("capturable", [False, True])
def test_skip_nonfinite(capturable, bad):
    from newsrec_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(4)
    shapes = [(300, 7), (3,), (4097,)]
    ps = [torch.randn(s, generator=gen) for s in shapes]
    gs = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(3)]
    if bad == "inf_last":
        gs[1][-1].view(-1)[-1] = INF
    else:
        gs[1][0].view(-1)[0] = NAN
    mine = [p.clone().cuda().requires_grad_(True) for p in ps]
    twin = [p.clone().cuda().requires_grad_(True) for p in ps]
    kw = dict(lr=1e-3, capturable=capturable, max_grad_norm=2.0, skip_nonfinite=True)
    o1, o2 = FusedAdam(mine, **kw), FusedAdam(twin, **kw)
    _assign(mine, gs[0])
    o1.step()
    after1 = _opt_snapshot(o1, mine)
    assert all(s == 1 for *_, s in after1)
    _assign(mine, gs[1])
    o1.step()
    assert _same(_opt_snapshot(o1, mine), after1)
    st = o1.clip_stats()
    assert st["nonfinite"] == 1 and st["nonfinite_total"] == 1
    _assign(mine, gs[2])
    o1.step()
    for step in (0, 2):                                # the twin never sees step 2
        _assign(twin, gs[step])
        o2.step()
    assert _same(_opt_snapshot(o1, mine), _opt_snapshot(o2, twin))
    st = o1.clip_stats()
    assert st["nonfinite"] == 0 and st["nonfinite_total"] == 1
    assert not _same(_opt_snapshot(o1, mine), after1)
    assert K.self_cleaning_check("cuda") == []


def test_no_skip_follows_torch():
    """skip_nonfinite=False: an inf element makes the norm inf and the scale 0, as torch's clip does
    -- the inf element's product is NaN, every other gradient reads as zero."""
    from newsrec_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(6)
    shapes = [(300, 7), (3,), (4097,)]
    ps = [torch.randn(s, generator=gen) for s in shapes]
    gs = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(2)]
    gs[1][2][1234] = INF
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [p.clone().cuda().requires_grad_(True) for p in ps]
    o1 = torch.optim.Adam(ref, lr=1e-3)
    o2 = FusedAdam(mine, lr=1e-3, max_grad_norm=2.0)
    for step in range(2):
        _assign(ref, gs[step])
        _assign(mine, gs[step])
        torch.nn.utils.clip_grad_norm_(ref, 2.0)
        o1.step()
        o2.step()
    st = o2.clip_stats()
    assert st["norm"] == INF and st["scale"] == 0.0 and st["nonfinite"] == 1
    nans = 0
    for p, q in zip(ref, mine):
        p, q = p.detach(), q.detach().cpu()
        assert torch.equal(torch.isnan(p), torch.isnan(q))
        nans += int(torch.isnan(p).sum())
        ok = ~torch.isnan(p)
        torch.testing.assert_close(q[ok], p[ok], rtol=0, atol=1e-6)
    assert nans == 1


def test_graph_replay_is_bitwise_eager():
    from newsrec_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(8)
    shapes = [(300, 7), (3,), (4097,), (2 * 4096,)]
    ps = [torch.randn(s, generator=gen) for s in shapes]
    # two warm-up steps and four replays; replay 2 carries an inf, replays 0 / 3 clip, replay 1 does not
    mags = [1.0, 1.0, 1.0, 1e-3, 1.0, 1.0]
    gs = [[torch.randn(s, generator=gen) * mag for s in shapes] for mag in mags]
    gs[4][1][2] = INF
    graphed = [p.clone().cuda().requires_grad_(True) for p in ps]
    eager = [p.clone().cuda().requires_grad_(True) for p in ps]
    kw = dict(lr=1e-3, capturable=True, max_grad_norm=2.0, skip_nonfinite=True)
    og, oe = FusedAdam(graphed, **kw), FusedAdam(eager, **kw)
    for p in graphed:
        p.grad = torch.zeros_like(p)                   # the static gradient buffers
    for step in range(2):
        for p, g in zip(graphed, gs[step]):
            p.grad.copy_(g)
        og.step()
        _assign(eager, gs[step])
        oe.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    # (a capture records and does not run: the state is still the one after the warm-up steps)
    assert _same(_opt_snapshot(og, graphed), _opt_snapshot(oe, eager))
    seen = []
    for step in range(2, 6):
        for p, g in zip(graphed, gs[step]):
            p.grad.copy_(g)
        graph.replay()
        _assign(eager, gs[step])
        oe.step()
        torch.cuda.synchronize()
        assert _same(_opt_snapshot(og, graphed), _opt_snapshot(oe, eager)), step
        assert torch.equal(og._clip_state().cpu(), oe._clip_state().cpu()), step
        seen.append(og.clip_stats())
    assert [s["nonfinite"] for s in seen] == [0, 0, 1, 0] and seen[-1]["nonfinite_total"] == 1
    assert seen[0]["scale"] < 1.0 and seen[1]["scale"] == 1.0 and seen[3]["scale"] < 1.0
    assert [s for *_, s in _opt_snapshot(og, graphed)] == [5] * len(shapes)   # six steps, one skipped
    assert K.self_cleaning_check("cuda") == []


def test_model_level():
    from golden_util import Golden
    from model_util import build_model, load_golden_params
    from newsrec_amd.manager import get_optim, train_step
    g = Golden("nrms")
    model = build_model(g.encN, g.encU, g.hidden, vocab=int(g["meta.vocab"]))
    load_golden_params(model, g)
    model.train()
    opt = get_optim(model, max_grad_norm=2.0)
    assert opt.max_grad_norm == 2.0 and not opt.skip_nonfinite
    versions = {}
    real_step = opt.step

    def step(*a, **kw):
        versions.update({n: p.grad._version for n, p in model.named_parameters() if p.grad is not None})
        return real_step(*a, **kw)
    opt.step = step
    train_step(model, opt, g.inputs("cuda"))
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    st = opt.clip_stats()
    want = norm_ref(list(grads.values()))
    assert want > 0 and close(st["norm"], want), (st["norm"], want)
    table = "embedding.bert_word_embedding.weight"
    assert versions and all(grads[n]._version == v for n, v in versions.items())
    assert grads[table]._version == versions[table]
    # the row flags the backward published for the word table are still valid after the step
    # (optim.FusedAdam's own test of them)
    rt = getattr(dict(model.named_parameters())[table], "_nr_row_touched", None)
    assert rt is not None and rt[0]() is grads[table] and rt[2] == grads[table]._version


def test_sharded_table_with_clipping_is_refused():
    from newsrec_amd.optim import FusedAdam
    p = torch.randn(64, 8, device="cuda", requires_grad=True)
    p.grad = torch.randn_like(p)
    p._nr_shard = (0, 32)
    for kw in (dict(max_grad_norm=2.0), dict(skip_nonfinite=True)):
        with pytest.raises(NotImplementedError):
            FusedAdam([p], **kw).step()
    FusedAdam([p]).step()                              # unclipped: the sharded update as before
