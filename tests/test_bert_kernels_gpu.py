"""The BERT tower's kernels (csrc/bert.hip) called directly -- K.bert_add_ln_fwd / _bwd, K.bert_embed_fwd /
_bwd with the table-gradient chain behind it (K.embedding_bwd with padding_idx, K.colsum over the [nseq,
L*H] and [T, H] views), K.embedding_fwd, K.tanh_bwd, K.bert_attn_fwd / _bwd -- against the float64
references of tests/bert_util.py under the device dropout replayed bit for bit (oracle.restatement.
BertDropout).

Every matrix has a leading dimension wider than its row with NaN in the padding and every output starts
as NaN: the padding must come back NaN bit for bit and every valid element written.  dgamma / dbeta
start from PRELOAD and must come back as PRELOAD + gradient.  The backward always runs on the statistics
its own forward saved.

The bar is that of tests/test_mha_pool_gpu.py and tests/test_attn_pool_gpu.py: with e32 = max|ref32 -
ref64| of the same reference in float32 on the CPU, err <= 32 e32 + 32 * 2^-24 * max|ref64| per tensor, a
bar that may itself never exceed 1e-4 * max|ref64|; f32 and bf16x6 alike.  Plain bf16 keeps the bar of
tests/test_bert_gpu.py, 3e-2 * max(1, max|ref64|).  dq, dk, dv are compared block by block (each with
its own e32), max|ref64| being that of the one tensor dqkv they are stored in: at L = 1 the softmax has
one element, dq and dk are zero in the reference and a rounding residue of dv's size in the kernels (D =
dctx . ctx and dP = dctx . v are formed by different sums).  Onto a preloaded dgamma / dbeta one atomic
per workgroup lands, each rounding at the magnitude of preload + sum instead of that of the sum: that
many times 2^-24 * PRELOAD is allowed on top of the bar.  Every case prints its err / e32 ratios
("bert-ratio" lines, pytest -s).

ml holds what include/newsrec_hip.h documents, (row max of the masked scaled scores, 1 / row sum of exp(s -
max)), in all three arithmetics: it is checked against exactly that on every sequence but the fully
masked one (maximum finfo.min).  No kernel defect was found.

Measured on an MI355X at this commit (five runs; the atomic sums vary a little between runs), the
largest err / e32 of any case per output -- no output needed a multiplier above 32, the largest err /
bar of any fp32-class line was 0.29 (dq at L = 65), of any bf16 line 0.18:
  add-LN   out 1.6  mean 4.1  rstd 3.7  dres 1.6  dx 1.8  dgamma 6.6  dbeta 8.5 (both at T = 4101)
  embed    out 1.4  mean 3.4  rstd 2.5  ds 2.3  dgamma 10.8  dbeta 11.8 (both at T = 4101)
           dword 2.0  dpos 2.3  dtype0 2.1
  attn     ctx 1.9  max 1.4  1/sum 1.5  dq 2.0  dk 1.9  dv 1.8 (f32 and bf16x6)
  tanh     dx 1.0

One-line value errors tried on scratch builds of csrc/bert.hip, each run once against this module:
  * pscale dropped from the add-LN forward and backward together: the 8 p0.1 cases of test_add_ln_widths,
    test_add_ln_long, test_add_ln_one_row, test_add_ln_device_rng_key;
  * pscale dropped from the embeddings' forward and backward together: the 8 p0.1 cases of
    test_embed_widths, test_embed_position_wraps[p0.1], test_embed_long, _one_row, _eps, _device_rng_key;
  * the - m1 term dropped from the LayerNorm backward: every add-LN and embed case that runs a backward;
  * in the add-LN backward's loop, mean / rstd read after the prefetch: test_add_ln_long alone (dres, dx of
    rows 0 .. 4, the rows computed after their successor's prefetch, and dgamma);
  * the attention dropout's element index built from the query's index inside a 128-query chunk, in the
    forward and both backward kernels alike: the 10 p0.1 cases of test_attention_vs_reference at L = 129
    and 257 (f32, bf16x6, bf16) and the 3 of test_attention_layout, none at L <= 128;
  * the 1/8 score scale dropped from dQ: 94 of the 100 cases of test_attention_vs_reference (all but six at
    L = 1, where dq is zero), test_attention_layout, _mask_dtypes, _device_rng_key;
  * eps left out of rstd: test_add_ln_eps and test_embed_eps alone (BERT's 1e-12 is invisible in float32).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_util import (add_ln_reference, attn_inputs, attn_mask, attn_reference, bert_dropout, embed_inputs,
                       embed_reference, ln_inputs)
from test_attn_pool_gpu import _leave_no_blocks_behind  # noqa: F401  (module-scope autouse: empty_cache at the end)

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
F64, F32 = torch.float64, torch.float32
SEED, EPS, P_DROP, PRELOAD = 77, 1e-12, 0.1, 0.5
MULT = {}      # output -> a multiplier of e32 above 32 (see the module docstring); none needed

# NV = ceil(H / 256) = 1..4 at a multiple of 256, just under it (a partial last float4 chunk: some lanes
# of the last j have c >= H) and just over it (one lane in the last j); H = 4: one lane of the wave
WIDTHS = [4, 252, 256, 260, 512, 768, 772, 1024]
# ceil(L / 32) = 1..4 waves at, under and over a multiple of 32; 128 | 129 and 256 | 257 the query-chunk
# edges of the four- and eight-wave workgroups
LENGTHS = [1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 257]
ATTN_CASES = [(L, h, prec, p) for L in LENGTHS for h in (1, 3) for prec in ("f32", "bf16x6") for p in (0.0, P_DROP)]
ATTN_CASES += [(L, h, "bf16", p) for L in (32, 97, 257) for h in (1, 3) for p in (0.0, P_DROP)]


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _padded(t, pad):
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def _vec(n, fill=NAN, tail=3):
    buf = _nan(n + tail)
    buf[:n] = fill
    return buf, buf[:n]


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _matrix_ok(o, names, width):
    for name in names:
        assert _all_nan_bits(o[name][:, width:]), "%s: written past column %d" % (name, width)
        assert torch.isfinite(o[name][:, :width]).all(), "%s: elements not written, or non-finite values" % name


def _vector_ok(o, sizes):
    for name, w in sizes:
        assert _all_nan_bits(o[name][w:]), "%s: written past element %d" % (name, w)
        assert torch.isfinite(o[name][:w]).all(), "%s: elements not written, or non-finite values" % name


def compare(tag, what, items, prec="f32", slack=None):
    """items: (name, got, ref64, ref32[, max|ref64| to take instead of this tensor's own])."""
    late = []
    for name, got, want, w32, *rest in items:
        got = got.double().reshape(want.shape)
        scale = rest[0] if rest else want.abs().max().item()
        e32 = (w32.double() - want).abs().max().item()
        err = (got - want).abs().max().item()
        if prec == "bf16":
            bar = 3e-2 * max(1.0, scale)
        else:
            bar = MULT.get(name, 32) * e32 + 32 * 2.0 ** -24 * scale
            assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        print("bert-ratio %s %s %s %-12s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (tag, what, prec, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        if not err <= bar + (slack or {}).get(name, 0.0):
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))
    assert not late, "%s %s: %s" % (tag, what, "; ".join(late))


def _drop_args(c, rng, seed, offset):
    """The case's own host key (seed, offset) unless the test overrides it."""
    return dict(p_drop=c.p, seed=c.seed if seed is None else seed, offset=c.offset if offset is None else offset, rng=rng)


def _ln_slack(T, preload):
    """One atomic per workgroup of four rows, at most 1024 workgroups (ln_bwd_grid)."""
    adds = min((T + 3) // 4, 1024)
    return {k: adds * 2.0 ** -24 * abs(preload) for k in ("add.dgamma", "add.dbeta", "embed.dgamma", "embed.dbeta")}


# ---------------------------------------------------------------------- LayerNorm(dropout(x) + res)

@functools.lru_cache(maxsize=None)
def ln_case(T, H, p, seed=SEED, offset=None, eps=EPS):
    inp = ln_inputs(T, H, 1000 * H + T)
    d = bert_dropout(seed, T, H, 1, p)
    if offset is not None:      # the dense site moved to ``offset``
        d.site[2] = offset
    keep = d.dense(0, 0, 0, T) if p else None
    ref = {dt: add_ln_reference(inp["x"], inp["res"], inp["gamma"], inp["beta"], eps, keep, p, dout=inp["dout"], dtype=dt)
           for dt in (F64, F32)}
    return types.SimpleNamespace(T=T, H=H, p=p, inp=inp, keep=keep, ref=ref, seed=seed, offset=d.site[2], eps=eps,
                                 tag="add-T%d-H%d-p%g" % (T, H, p))


def run_add_ln(c, rng=None, seed=None, offset=None, preload=PRELOAD):
    from newsrec_amd import kernels as K
    T, H, inp = c.T, c.H, c.inp
    x, res = _padded(inp["x"], 4), _padded(inp["res"], 8)
    gamma, beta = inp["gamma"].cuda(), inp["beta"].cuda()
    out, stats = _nan(T, H + 4), _vec(2 * T)
    drop = _drop_args(c, rng, seed, offset)
    K.bert_add_ln_fwd(x, res, gamma, beta, c.eps, out[:, :H], stats[1], **drop)
    dout = _padded(inp["dout"], 8)
    dres, dx = _nan(T, H + 8), _nan(T, H + 4)
    dgamma, dbeta = _vec(H, preload), _vec(H, preload)
    K.bert_add_ln_bwd(x, res, gamma, stats[1], dout, dres[:, :H], dx[:, :H], dgamma[1], dbeta[1], **drop)
    torch.cuda.synchronize()
    o = dict(out=out, stats=stats[0], dres=dres, dx=dx, dgamma=dgamma[0], dbeta=dbeta[0])
    return {k: t.cpu() for k, t in o.items()}


def _ln_items(fam, c, o, rows, grads, preload):
    T, H = c.T, c.H
    r64, r32 = c.ref[F64], c.ref[F32]
    st = o["stats"][:2 * T].reshape(T, 2)
    items = [(fam + ".out", o["out"][rows, :H], r64["out"][rows], r32["out"][rows]),
             (fam + ".mean", st[rows, 0], r64["stats"][rows, 0], r32["stats"][rows, 0]),
             (fam + ".rstd", st[rows, 1], r64["stats"][rows, 1], r32["stats"][rows, 1])]
    items += [("%s.%s" % (fam, g), o[g][rows, :H], r64[g][rows], r32[g][rows]) for g in grads]
    if rows == slice(None):
        items += [("%s.%s" % (fam, g), o[g][:H].double() - preload, r64[g], r32[g]) for g in ("dgamma", "dbeta")]
    return items


def check_add_ln(c, o, what, preload=PRELOAD):
    T, H = c.T, c.H
    _matrix_ok(o, ("out", "dres", "dx"), H)
    _vector_ok(o, (("stats", 2 * T), ("dgamma", H), ("dbeta", H)))
    if c.keep is not None:
        assert (o["dx"][:, :H][~c.keep] == 0).all(), "dx is not zero where the dropout drops"
    if T > 4096:   # the second trip of the backward's grid-stride loop, and the rows of the first trip whose
        # arithmetic runs after the prefetch of their successor in the second, each named on its own
        compare(c.tag, what + "-rows4096+", _ln_items("add", c, o, slice(4096, T), ("dres", "dx"), preload))
        compare(c.tag, what + "-rows<%d" % (T - 4096), _ln_items("add", c, o, slice(0, T - 4096), ("dres", "dx"), preload))
    compare(c.tag, what, _ln_items("add", c, o, slice(None), ("dres", "dx"), preload), slack=_ln_slack(T, preload))


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("H", WIDTHS)
def test_add_ln_widths(H, p):
    """T = 5: a full workgroup of four rows and a partial one."""
    c = ln_case(5, H, p)
    check_add_ln(c, run_add_ln(c), "vs-ref")


def test_add_ln_long():
    """T = 4101 at H = 260 (NV = 2): 1026 workgroups of rows against the backward's cap of 1024 (CUs x
    occupancy is above it on the MI355X), so rows 4096 .. 4100 are the loop's second trip, fetched by the
    prefetch of the first."""
    c = ln_case(4101, 260, P_DROP)
    check_add_ln(c, run_add_ln(c), "vs-ref")


def test_add_ln_one_row():
    c = ln_case(1, 768, P_DROP)
    check_add_ln(c, run_add_ln(c), "vs-ref")


def test_add_ln_eps():
    """BERT's eps of 1e-12 is below float32's resolution of a variance near 1: an eps of 0.25 shows
    that the argument reaches rstd."""
    c = ln_case(5, 260, P_DROP, eps=0.25)
    assert (c.ref[F64]["stats"][:, 1] - ln_case(5, 260, P_DROP).ref[F64]["stats"][:, 1]).abs().min() > 1e-2
    check_add_ln(c, run_add_ln(c), "eps")


def test_add_ln_device_rng_key():
    """Host (seed, offset) and the device pair rng = (seed, base) with offset added on the device give
    identical bits; another offset gives another mask."""
    c = ln_case(5, 260, P_DROP)
    host = run_add_ln(c)
    base, k = c.offset - 33, 33
    rng = torch.tensor([c.seed, base], dtype=torch.int64, device="cuda")
    dev = run_add_ln(c, rng=rng, seed=1, offset=k)
    for name in ("out", "stats", "dres", "dx"):      # (dgamma / dbeta: two atomics onto the preload, either order)
        assert _bits_equal(host[name], dev[name]), name
    check_add_ln(c, dev, "rng")
    other = ln_case(5, 260, P_DROP, offset=c.offset + 1)
    assert not torch.equal(other.keep, c.keep)
    o = run_add_ln(other)
    check_add_ln(other, o, "offset+1")
    assert ((o["dx"][:, :c.H] == 0) == ~other.keep).all() and ((host["dx"][:, :c.H] == 0) == ~c.keep).all()


# ---------------------------------------------------------------------- embeddings

V_EMBED = 11


@functools.lru_cache(maxsize=None)
def embed_case(nseq, L, H, p, P=None, seed=SEED, offset=None, eps=EPS):
    T = nseq * L
    P = L + 2 if P is None else P
    inp = embed_inputs(nseq, L, H, V_EMBED, P, 1000 * H + 10 * nseq + L)
    d = bert_dropout(seed, T, H, 1, p)
    if offset is not None:      # the embedding site moved to ``offset``
        d.site[0] = offset
    keep = d.embed(0, T) if p else None
    ref = {dt: embed_reference(inp["word"], inp["pos"], inp["type"][0], inp["ids"], inp["gamma"], inp["beta"], eps, keep,
                               p, dout=inp["dout"], dtype=dt) for dt in (F64, F32)}
    return types.SimpleNamespace(nseq=nseq, L=L, T=T, H=H, P=P, p=p, inp=inp, keep=keep, ref=ref, seed=seed, offset=d.site[0],
                                 eps=eps, tag="embed-%dx%d-H%d-p%g" % (nseq, L, H, p))


def run_embed(c, ids=None, status=None, rng=None, seed=None, offset=None, preload=PRELOAD, bwd=True):
    """nr_bert_embed_fwd, nr_bert_embed_bwd on its stats, then the table gradients as newsrec_amd/bert.py
    forms them from the contiguous ds: embedding_bwd with padding_idx 0 and the two colsums."""
    from newsrec_amd import kernels as K
    nseq, L, T, H, inp = c.nseq, c.L, c.T, c.H, c.inp
    word, pos, typ = inp["word"].cuda(), inp["pos"].cuda(), inp["type"].cuda()
    gamma, beta = inp["gamma"].cuda(), inp["beta"].cuda()
    ids = (inp["ids"] if ids is None else ids).reshape(-1).cuda()
    out, stats = _nan(T, H + 4), _vec(2 * T)
    drop = _drop_args(c, rng, seed, offset)
    K.bert_embed_fwd(word, pos, typ[0], ids, nseq, L, gamma, beta, c.eps, out[:, :H], stats[1], status=status, **drop)
    res = dict(out=out, stats=stats[0])
    if bwd:
        dout = _padded(inp["dout"], 8)
        ds = _nan(T, H + 4)
        dgamma, dbeta = _vec(H, preload), _vec(H, preload)
        K.bert_embed_bwd(word, pos, typ[0], ids, nseq, L, gamma, stats[1], dout, ds[:, :H], dgamma[1], dbeta[1], **drop)
        dsc = ds[:, :H].contiguous()
        # accumulated into: zero, with one more row of NaN behind (and the unused type row 1) as the guard
        dword, dpos, dtyp = (_nan(n + 1, H) for n in (V_EMBED, c.P, 1))
        dword[:V_EMBED] = 0
        dpos[:c.P] = 0
        dtyp[0] = 0
        K.embedding_bwd(dsc, ids, dword[:V_EMBED], padding_idx=0)
        K.colsum(dsc.view(nseq, L * H), nseq, L * H, dpos[:c.P].view(-1))
        K.colsum(dsc, T, H, dtyp[0])
        res.update(ds=ds, dgamma=dgamma[0], dbeta=dbeta[0], dword=dword, dpos=dpos, dtyp=dtyp)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in res.items()}


def check_embed(c, o, what, preload=PRELOAD):
    T, H, L, P = c.T, c.H, c.L, c.P
    _matrix_ok(o, ("out", "ds"), H)
    _vector_ok(o, (("stats", 2 * T), ("dgamma", H), ("dbeta", H)))
    for name, n in (("dword", V_EMBED), ("dpos", P), ("dtyp", 1)):
        assert _all_nan_bits(o[name][n:]) and torch.isfinite(o[name][:n]).all(), name + ": the guard row was written"
    if c.keep is not None:
        assert (o["out"][:, :H][~c.keep] == 0).all(), "out is not zero where the dropout drops"
    assert (o["dword"][0] == 0).all(), "the padding row of dword is not zero"
    assert (o["dpos"][L:P] == 0).all(), "dpos rows past L are not zero"
    if T > 4096:
        compare(c.tag, what + "-rows4096+", _ln_items("embed", c, o, slice(4096, T), ("ds",), preload))
    r64, r32 = c.ref[F64], c.ref[F32]
    items = _ln_items("embed", c, o, slice(None), ("ds",), preload)
    items += [("embed.dword", o["dword"][:V_EMBED], r64["dword"], r32["dword"]),
              ("embed.dpos", o["dpos"][:P], r64["dpos"], r32["dpos"]),
              ("embed.dtype0", o["dtyp"][0], r64["dtype0"], r32["dtype0"])]
    compare(c.tag, what, items, slack=_ln_slack(T, preload))


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("H", WIDTHS)
def test_embed_widths(H, p):
    c = embed_case(1, 5, H, p)
    check_embed(c, run_embed(c), "vs-ref")


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
def test_embed_position_wraps(p):
    """3 x 7: t % L wraps twice, and dpos sums over the sequences."""
    c = embed_case(3, 7, 260, p)
    ids = c.inp["ids"].view(-1)
    assert (ids == 0).any() and ids.unique().numel() < ids.numel()     # the padding id and duplicates
    check_embed(c, run_embed(c), "vs-ref")


def test_embed_long():
    """4101 sequences of one token at H = 8 (one position row): rows 4096 .. 4100 are the second trip of
    the backward's grid-stride loop; every word row but the padding row takes some 400 atomic adds."""
    c = embed_case(4101, 1, 8, P_DROP, P=1)
    check_embed(c, run_embed(c), "vs-ref")


def test_embed_one_row():
    c = embed_case(1, 1, 768, P_DROP)
    check_embed(c, run_embed(c), "vs-ref")


def test_embed_eps():
    c = embed_case(3, 7, 260, P_DROP, eps=0.25)
    assert (c.ref[F64]["stats"][:, 1] - embed_case(3, 7, 260, P_DROP).ref[F64]["stats"][:, 1]).abs().min() > 1e-2
    check_embed(c, run_embed(c), "eps")


def test_embed_device_rng_key():
    c = embed_case(3, 7, 260, P_DROP, offset=4242)
    host = run_embed(c)
    rng = torch.tensor([c.seed, 4200], dtype=torch.int64, device="cuda")
    dev = run_embed(c, rng=rng, seed=1, offset=42)
    for name in ("out", "stats", "ds"):
        assert _bits_equal(host[name], dev[name]), name
    check_embed(c, dev, "rng")
    other = embed_case(3, 7, 260, P_DROP)        # offset site[0] = 0
    assert not torch.equal(other.keep, c.keep)
    o = run_embed(other, bwd=False)
    assert ((o["out"][:, :c.H] == 0) == ~other.keep).all() and ((host["out"][:, :c.H] == 0) == ~c.keep).all()


def test_embed_status():
    """An id of V and an id of -1 OR 2 into the status word and take the row of id 0; a clean batch
    leaves the word zero."""
    c = embed_case(3, 7, 260, P_DROP)
    bad, zeroed = c.inp["ids"].clone(), c.inp["ids"].clone()
    bad[1, 2], bad[2, 5] = V_EMBED, -1
    zeroed[1, 2], zeroed[2, 5] = 0, 0
    st_bad, st_zero, st_clean = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    o_bad = run_embed(c, ids=bad, status=st_bad, bwd=False)
    o_zero = run_embed(c, ids=zeroed, status=st_zero, bwd=False)
    run_embed(c, status=st_clean, bwd=False)
    assert st_bad.item() == 2 and st_zero.item() == 0 and st_clean.item() == 0
    assert _bits_equal(o_bad["out"], o_zero["out"]) and _bits_equal(o_bad["stats"], o_zero["stats"])
    assert torch.isfinite(o_bad["out"][:, :c.H]).all()


def test_embedding_fwd_bitwise():
    from newsrec_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    table = torch.randn(13, 260, generator=g).cuda()
    idx = torch.tensor([3, 0, 12, 3, 7, 0, 12, 12, 1], device="cuda")
    out = _nan(idx.numel() + 1, 260)
    K.embedding_fwd(table, idx, out[:idx.numel()])
    torch.cuda.synchronize()
    assert torch.equal(out[:idx.numel()], table[idx]) and _all_nan_bits(out[idx.numel():])


# ---------------------------------------------------------------------- tanh backward

@pytest.mark.parametrize("rows,cols", [(7, 768), (3, 4)])
def test_tanh_bwd(rows, cols):
    from newsrec_amd import kernels as K
    g = torch.Generator().manual_seed(rows)
    y = torch.tanh(torch.randn(rows, cols, generator=g))
    dy = torch.randn(rows, cols, generator=g)
    dx = _nan(rows, cols + 4)
    K.tanh_bwd(_padded(y, 4), _padded(dy, 8), dx[:, :cols])
    torch.cuda.synchronize()
    o = {"dx": dx.cpu()}
    _matrix_ok(o, ("dx",), cols)
    want = {dt: dy.to(dt) * (1 - y.to(dt) ** 2) for dt in (F64, F32)}
    compare("tanh-%dx%d" % (rows, cols), "vs-ref", [("tanh.dx", o["dx"][:, :cols], want[F64], want[F32])])


# ---------------------------------------------------------------------- attention

@functools.lru_cache(maxsize=None)
def attn_case(L, heads, p, seed=SEED, offset=None):
    mask = attn_mask(L)
    nseq, H = mask.shape[0], heads * 64
    T = nseq * L
    inp = attn_inputs(nseq, L, heads, 100 * L + heads)
    d = bert_dropout(seed, T, H, heads, p)
    if offset is not None:      # the attention site moved to ``offset``
        d.site[1] = offset
    keep = d.attn(0, 0, nseq, L) if p else None
    ref = {dt: attn_reference(inp["q"], inp["k"], inp["v"], mask, heads, keep, p, dctx=inp["dctx"], dtype=dt)
           for dt in (F64, F32)}
    return types.SimpleNamespace(L=L, heads=heads, nseq=nseq, T=T, H=H, p=p, mask=mask, inp=inp, keep=keep, ref=ref,
                                 seed=seed, offset=d.site[1], tag="attn-L%d-h%d-p%g" % (L, heads, p))


def _layout(H, layout):
    """-> columns of Q, K, V in the stored row and the row's width.  default: [Q | K | V | pad 8];
    vqk: [V | pad 4 | Q | pad 4 | K | pad 4] (voff negative, koff not heads * 64)."""
    return (0, H, 2 * H, 3 * H + 8) if layout == "default" else (H + 4, 2 * H + 8, 0, 3 * H + 12)


def run_attn(c, prec, layout="default", mask=None, rng=None, seed=None, offset=None, keep=False):
    from newsrec_amd import _lib as Lb, kernels as K
    mode = {"f32": Lb.GEMM_F32, "bf16x6": Lb.GEMM_BF16X6, "bf16": Lb.GEMM_BF16}[prec]
    T, H, heads, inp = c.T, c.H, c.heads, c.inp
    qo, ko, vo, width = _layout(H, layout)
    buf, dbuf = _nan(T, width), _nan(T, width)
    for col, name in ((qo, "q"), (ko, "k"), (vo, "v")):
        buf[:, col:col + H] = inp[name].cuda()
    off = {} if layout == "default" else dict(koff=ko - qo, voff=vo - qo)
    m = (c.mask if mask is None else mask).cuda()
    ctx, ml = _nan(T, H + 4), _vec(2 * T * heads)
    drop = _drop_args(c, rng, seed, offset)
    if keep:    # the forward stores its dropout keep bits, the backward reads them instead of hashing
        drop["keep"] = K.bert_attn_keep_buffer(c.nseq, c.L, heads, "cuda")
    K.bert_attn_fwd(buf[:, qo:], heads, m, c.nseq, c.L, ctx[:, :H], ml[1], prec=mode, **off, **drop)
    K.bert_attn_bwd(buf[:, qo:], heads, m, c.nseq, c.L, ctx[:, :H], ml[1], _padded(inp["dctx"], 8), dbuf[:, qo:],
                    prec=mode, **off, **drop)
    torch.cuda.synchronize()
    return {"ctx": ctx.cpu(), "ml": ml[0].cpu(), "dqkv": dbuf.cpu()}


def check_attn(c, o, what, prec, layout="default"):
    T, H, heads, L = c.T, c.H, c.heads, c.L
    qo, ko, vo, width = _layout(H, layout)
    _matrix_ok(o, ("ctx",), H)
    _vector_ok(o, (("ml", 2 * T * heads),))
    stored = torch.zeros(width, dtype=torch.bool)
    for col in (qo, ko, vo):
        stored[col:col + H] = True
    assert _all_nan_bits(o["dqkv"][:, ~stored]), "dqkv: written outside the Q / K / V columns"
    assert torch.isfinite(o["dqkv"][:, stored]).all(), "dqkv: Q / K / V columns not written, or non-finite values"
    r64, r32 = c.ref[F64], c.ref[F32]
    # ml against (row max, 1 / row sum) but for the fully masked sequence 2, whose maximum is finfo.min
    rows = torch.ones(c.nseq, L, dtype=torch.bool)
    rows[2] = False
    assert c.mask[2].sum() == 0 and (c.mask.sum(1) == 0).sum() == 1
    rows = rows.reshape(-1)
    ml = o["ml"][:2 * T * heads].reshape(T, heads, 2)
    gmax = max(r64[g].abs().max().item() for g in ("dq", "dk", "dv"))
    items = [("attn.ctx", o["ctx"][:, :H], r64["ctx"], r32["ctx"]),
             ("attn.m", ml[rows, :, 0], r64["m"][rows], r32["m"][rows]),
             ("attn.il", ml[rows, :, 1], r64["il"][rows], r32["il"][rows])]
    items += [("attn." + g, o["dqkv"][:, col:col + H], r64[g], r32[g], gmax) for g, col in (("dq", qo), ("dk", ko), ("dv", vo))]
    compare(c.tag, what, items, prec=prec)


@pytest.mark.parametrize("L,heads,prec,p", ATTN_CASES, ids=["L%d-h%d-%s-p%g" % c for c in ATTN_CASES])
def test_attention_vs_reference(L, heads, prec, p):
    c = attn_case(L, heads, p)
    check_attn(c, run_attn(c, prec), "vs-ref", prec)


# the smallest shapes that reach: a single-slot keep word; two key tiles on the short route; the last short
# length; the first long length; two query chunks of the four-wave dQ pass beside one eight-wave chunk; two
# eight-wave chunks
KEEP_SHAPES = [(1, 1), (33, 3), (96, 3), (97, 3), (129, 3), (257, 3)]


@pytest.mark.parametrize("L,heads", KEEP_SHAPES, ids=["L%d-h%d" % c for c in KEEP_SHAPES])
@pytest.mark.parametrize("prec", ["bf16x6", "bf16"])
def test_attention_keep_bits(prec, L, heads):
    """The route the BERT tower runs: the bf16-MFMA forward stores the dropout keep bits (K.bert_attn_keep_buffer)
    and both backward kernels read them instead of re-hashing every probability's counter.  Against the float64
    reference at the bar of every other attention case, and bit for bit the hashed run of the same case: the
    masks are the same either way and the arithmetic after the mask is identical."""
    c = attn_case(L, heads, P_DROP)
    o = run_attn(c, prec, keep=True)
    check_attn(c, o, "keep-bits", prec)
    h = run_attn(c, prec)
    for name in ("ctx", "ml", "dqkv"):
        assert _bits_equal(o[name], h[name]), "%s: stored keep bits vs the hash" % name


def test_attention_keep_bits_f32_rejected():
    """The f32 forward stores no keep bits: a keep buffer with prec = f32 is refused before any launch."""
    from newsrec_amd import _lib as Lb, kernels as K
    c = attn_case(33, 3, P_DROP)
    buf = torch.zeros(c.T, 3 * c.H, device="cuda")
    ctx, ml = torch.zeros(c.T, c.H, device="cuda"), torch.zeros(2 * c.T * c.heads, device="cuda")
    with pytest.raises(Lb.HipError, match="invalid argument 7"):
        K.bert_attn_fwd(buf, c.heads, c.mask.cuda(), c.nseq, c.L, ctx, ml, prec=Lb.GEMM_F32,
                        keep=K.bert_attn_keep_buffer(c.nseq, c.L, c.heads, "cuda"), **_drop_args(c, None, None, None))


@pytest.mark.parametrize("prec", ["f32", "bf16x6", "bf16"])
def test_attention_layout(prec):
    """qkv rows stored [V | pad | Q | pad | K | pad] (the entries take Q at the row pointer, so it is the
    view from Q on that is passed: voff is negative, koff is H + 4), every leading dimension padded, ctx
    NaN-filled: the same values as the default layout bit for bit, dqkv stored at exactly the Q / K / V
    columns.  L = 129: two query chunks of the four-wave workgroups."""
    c = attn_case(129, 3, P_DROP)
    o = run_attn(c, prec, layout="vqk")
    check_attn(c, o, "layout", prec, layout="vqk")
    d = run_attn(c, prec)
    H = c.H
    assert _bits_equal(o["ctx"], d["ctx"]) and _bits_equal(o["ml"], d["ml"])
    for a, b in zip(_layout(H, "vqk")[:3], _layout(H, "default")[:3]):
        assert _bits_equal(o["dqkv"][:, a:a + H], d["dqkv"][:, b:b + H])


@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
def test_attention_mask_dtypes(prec):
    c = attn_case(33, 3, P_DROP)
    outs = {}
    for dtype in (torch.int64, torch.uint8, torch.float64, torch.float32):
        m = c.mask.to(dtype)
        if dtype.is_floating_point:
            m = m * torch.where(torch.arange(c.L) % 2 == 0, 2.5, -1.0).to(dtype)
        elif dtype == torch.int64:
            m = m << 40                   # nonzero only above bit 32
        outs[dtype] = run_attn(c, prec, mask=m)
        check_attn(c, outs[dtype], "mask-" + str(dtype).split(".")[1], prec)
    for dtype, o in outs.items():
        for name in ("ctx", "ml", "dqkv"):
            assert _bits_equal(o[name], outs[torch.int64][name]), "%s with a %s mask" % (name, dtype)


@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
def test_attention_device_rng_key(prec):
    c = attn_case(33, 3, P_DROP)
    host = run_attn(c, prec)
    rng = torch.tensor([c.seed, c.offset - 9], dtype=torch.int64, device="cuda")
    dev = run_attn(c, prec, rng=rng, seed=1, offset=9)
    for name in host:
        assert _bits_equal(host[name], dev[name]), name
    other = attn_case(33, 3, P_DROP, offset=c.offset + 1)
    assert not torch.equal(other.keep, c.keep)
    check_attn(other, run_attn(other, prec), "offset+1", prec)
