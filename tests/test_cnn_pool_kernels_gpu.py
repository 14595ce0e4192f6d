"""The CNN news encoder's word-attention head (csrc/cnn_keypool.hip: K.cnn_keypool_fwd / K.cnn_keypool_bwd,
nr_cnn_keypool_workspace) and the learned-query pooling of the user encoders (csrc/seq_pool.hip:
K.seq_pool_fwd / K.seq_pool_bwd) called directly, against the float64 references
cnn_pool_util.cnn_keypool_reference and pool_util.attn_pool_reference (no LayerNorm, no dropout) on tiled
pool_mask(L) batches: the empty sequence, length 1, full, L - 1, L / 2, holes, length 2, only the last slot.
tests/test_cnn_keypool_gpu.py and tests/test_seq_pool_gpu.py keep the workload's own shapes.

Which kernels a case launches
  test_cnn_keypool_small[NB-H-prec-k0/k1...]   NB = Hp / 32 in 1 .. 5, two widths per NB (H = 32 NB: no
      padding; H = 32 (NB - 1) + 1: 31 of the last wave's columns padding; NB = 1: H = 32, 1, 20), prec in
      f32 / bf16x6 / bf16, k1 = the forward stores K and the backward reads it:
        forward   cnn_keypool_fwd_kernel<NB, 0> (f32), cnn_keypool_fwd_planes_kernel<NB, 3> (bf16x6) and
                  <NB, 1> (bf16): 15 instantiations, each with and without the K output
        backward  cnn_keypool_bwd_kernel<NB, NP, SK> for NP in 0, 3, 1 and SK = k1: 30 instantiations (the
                  dWq partition of 8 - NB waves: kb-major ranges for bf16x6, round-robin otherwise), then
                  cnn_keypool_reduce1_kernel (G = 16 partials: slices of 2, the tail loop alone) and
                  cnn_keypool_reduce2_kernel
      16 titles; L cycles over 1, 2, 15, 16, 17, 31, 32 within each NB (every NB meets all seven), the mask
      dtype over bool, u8, int64, float32, float64 (every prec meets all five), dz present / absent.
  test_cnn_keypool_grid[NB-nseq-prec]   NB = 1 (H = 20) and NB = 5 (H = 150) at L = 5, all three precs:
      nseq = 1, 7 (fewer partials than reduce1's 8 slices: empty slices), 70 (slices of 8 and 9 partials: the
      unrolled loop and the tail), 3 CUs + 5 (past the forward's cap of three workgroups per CU and the
      backward's of one: unequal numbers of titles per workgroup, the register prefetch of the next title;
      G = CUs).  Every output compared; the backward called twice, its parameter gradients bit-identical.
  test_cnn_keypool_empty / test_cnn_keypool_workspace   nseq = 0 (the forward writes nothing; the backward
      launches one idle workgroup and the reduce kernels store zeros), the workspace size, and -1003 with one
      float less (nothing written).
  test_seq_pool_wave[L-D-...]   nseq = 1026 (two waves of the last workgroup idle):
        seq_pool_fwd_kernel<32> / seq_pool_bwd_kernel<32>   L in 1, 8, 9, 31, 32
        seq_pool_fwd_kernel<64> / seq_pool_bwd_kernel<64>   L in 33, 63, 64
      D in 1, 3, 6, 150, 253, 256 (each template meets D % 4 = 0, 1, 2, 3); a tied key, a separate tanh key
      and a separate key with key_tanh = 0 in both templates, dz present and absent for tied and separate
      keys; and seq_pool_bwd_kernel<32> at nseq = 4 * 1024 + 3, L = 2, D = 6: the grid capped at 1024
      workgroups, a second strided round.
  test_seq_pool_workgroup[L-D-...]   nseq = 8: seq_pool_wg_fwd_kernel<NF> / seq_pool_wg_bwd_kernel<NF>
        NF = 1  D in 5, 150, 256      NF = 2  D in 257, 510, 512      NF = 4  D in 513, 1021, 1024
      L cycles over 1, 7, 8, 9, 63, 64 within each NF; the same three key forms, dz present and absent.
  Both seq_pool forms: qn = D, and qn < D on zero-padded columns; every ld = round4(D) + 4; dout one float
  off 16-B alignment with row stride qn + 1; dq accumulated onto seeded non-zero values with a NaN tail; the
  mask dtype cycles so that wave<32>, wave<64> and the workgroup forward and backward each meet all five.

Every buffer a kernel writes is a view inside a NaN-filled block with a spare row above and below and spare
columns (cnn_keypool: ldc = Hp + 4, ldn = Hp + 1, lddc = Hp + 1, lddn = H + 3 with dnews one float off 16-B
alignment, lddz = H + 1, ldk = Hp + 4): after the call the padding is NaN bit for bit, every element inside
the view is finite, and wherever the float64 and the float32 reference are both exactly zero (masked slots,
the empty sequence, the ReLU gate of dc, L = 1) so is the kernel's output -- as are the columns at or past
H of news, dc, K and dbq and the rows and columns at or past H of dwq.  Every buffer a kernel reads carries NaN
in its padding columns and spare rows (a read outside the view poisons the result), and is unchanged after
the call.

The bar is tied to the reference: the same reference evaluated in float32 on the CPU differs from float64 by
e32 = max|ref32 - ref64| per tensor, and with f32 and bf16x6 products the kernels must stay within
MULT * e32 + 32 * 2^-24 * max|ref64| with MULT = 32 (the convention of tests/test_mha_attn_kernels_gpu.py),
a bar that may itself never exceed 1e-4 * max|ref64|; where max|ref64| is 0 the output must be exactly 0.
With bf16 products the bar is the 3e-2 * max|ref64| of tests/test_cnn_keypool_gpu.py.  seq_pool's dq is
compared after its start is taken off, and the bar gains the rounding of the accumulating additions onto
that start: one per workgroup, each at most 2^-24 of a running value that never exceeds |start| + the sum of
the sequences' |shares| (dq_slack).  Every case prints its err / e32 ratios ("cnn-pool-ratio" lines,
pytest -s).

Where 32 e32 alone would pass the cap (dq of the wave cases: the float32 twin sums 1026 sequences in a row)
the bar is the cap, 1e-4 * max|ref64|.

Measured on an MI355X at this commit, the largest err / e32 of any case, per kernel family and output -- no
output needed a multiplier above 32 (MULT is empty), the largest err / bar of any line was 0.12 (0.48 with
bf16 products):
  cnn_keypool f32      news 1.6  probs 1.3  K 1.2  dc 1.6  dwq 2.5  dbq 5.2 (H = 1)  dq 2.2  dconv_b 1.8
  cnn_keypool bf16x6   news 1.7  probs 2.2  K 1.4  dc 1.3  dwq 1.6  dbq 4.7 (H = 1)  dq 1.5  dconv_b 1.8
  cnn_keypool bf16     err / max|ref64| at most: news 1.5e-3  probs 1.8e-3  K 1.4e-2  dc 1.7e-3  dwq 6.6e-3
                       dbq 1.3e-2  dq 4.5e-3  dconv_b 8.6e-4
  seq_pool wave<32>    out 2.7  probs 1.4  dx 1.2  dk 1.3  dq 0.7
  seq_pool wave<64>    out 1.2  probs 1.0  dx 1.0  dk 1.0  dq 0.5
  seq_pool wg<1>       out 2.8  probs 1.9  dx 1.2  dk 2.7  dq 1.3
  seq_pool wg<2>       out 1.0  probs 0.8  dx 1.0  dk 2.0  dq 1.1
  seq_pool wg<4>       out 0.7  probs 0.6  dx 1.0  dk 0.9  dq 1.1
Every case passed as the kernels stand: none of the arms listed above hid a fault.

One-line errors tried on scratch builds of the two sources (none changes an address or a launch), each
caught:
  cnn_keypool.hip
    the C > 0 gate of dc dropped                        all 66 small and 24 grid cases (dc, dconv_b)
    a dWq wave's last block skipped at NB = 3 and 4     round-robin form: 12 of the 16 f32 / bf16 small cases
                                                        of NB = 3, 4 (the others have L = 1, where dwq is zero)
                                                        and the workspace case Hp = 96; kb-major form: all 8
                                                        bf16x6 small cases of NB = 3, 4; no case of another NB
    p = e without the 1 / sum, both forward kernels     79 small and grid cases, the 3 workspace cases
    reduce1's tail loop dropped after the unrolled one  the 6 grid cases with nseq = 70, no other
  seq_pool.hip
    * g.scale dropped in the wave backward              10 of the 13 wave cases (the others: L = 1, and qn = 1
                                                        where the scale is 1)
    the workgroup forward pools row min(l, L - 1) with  15 of the 18 workgroup cases: all but L = 64
      that row's p for l >= L
    key_tanh ignored in both backward kernels           all 11 cases with a separate tanh key, no other
    ld4 without the selects past D (but the first)      all 23 cases with D % 4 != 0 (the NaN padding columns
                                                        poison the scores), no case with D % 4 == 0
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from cnn_pool_util import cnn_keypool_inputs, cnn_keypool_reference, seq_pool_dq_per_seq, typed_mask
from newsrec_amd import _lib as LIB
from pool_util import attn_pool_inputs, attn_pool_reference

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
F64, F32 = torch.float64, torch.float32
MASK_DTYPES = (torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64)
PRECS = (("f32", LIB.GEMM_F32), ("bf16x6", LIB.GEMM_BF16X6), ("bf16", LIB.GEMM_BF16))
MULT = {}      # "family.output" -> a multiplier of e32 above 32 (see the module docstring)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_blocks_behind():
    """The later modules of the suite see the caching allocator as they would without this one (a test
    of tests/test_row_grad_gpu.py depends on which block a freed gradient's successor gets)."""
    yield
    grid_case.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------- buffers

def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Framed:
    """A [rows, cols] view (``v``) inside a NaN block with a spare row above and below and ``pad`` spare
    columns, so that the view's row stride is cols + pad; ``data`` (CPU, at most [rows, cols]) fills its top
    left corner and zeros the rest of the view."""

    def __init__(self, rows, cols, pad, data=None):
        self.rows, self.cols = rows, cols
        self.buf = _nan(rows + 2, cols + pad)
        self.v = self.buf[1:rows + 1, :cols]
        if data is not None:
            self.v.zero_()
            self.v[:data.shape[0], :data.shape[1]] = data.to(F32).cuda()
        self.before = self.buf.clone()

    def frame_untouched(self):
        return (_all_nan_bits(self.buf[0]) and _all_nan_bits(self.buf[self.rows + 1])
                and _all_nan_bits(self.buf[:, self.cols:]))

    def unchanged(self):
        return _same_bits(self.buf, self.before)


class Vec:
    """n floats (``v``) inside a flat NaN buffer, four NaN floats before (the view stays 16-B aligned) and
    three after; ``data`` fills the front of the view and zeros its rest."""

    def __init__(self, n, data=None):
        self.n = n
        self.buf = _nan(n + 7)
        self.v = self.buf[4:4 + n]
        if data is not None:
            self.v.zero_()
            self.v[:data.numel()] = data.reshape(-1).to(F32).cuda()
        self.before = self.buf.clone()

    def frame_untouched(self):
        return _all_nan_bits(self.buf[:4]) and _all_nan_bits(self.buf[4 + self.n:])

    def unchanged(self):
        return _same_bits(self.buf, self.before)


class OffRows:
    """[rows, cols] read-only rows of stride ``ld`` whose first element sits one float past a 16-B boundary,
    inside a flat NaN buffer (more than a row of NaN before and after)."""

    def __init__(self, data, ld):
        rows, cols = data.shape
        assert ld >= cols
        self.buf = _nan((rows + 2) * ld + 8)
        assert self.buf.data_ptr() % 16 == 0
        start = ld + (1 - ld) % 4
        self.v = self.buf.as_strided((rows, cols), (ld, 1), start)
        assert self.v.data_ptr() % 16 == 4
        self.v.copy_(data.to(F32).cuda())
        self.before = self.buf.clone()

    def unchanged(self):
        return _same_bits(self.buf, self.before)


# ---------------------------------------------------------------------- checks

def compare(family, tag, pairs, ref, late, bf16=False):
    """pairs: (name, got, key into the references[, slack added to the bar]).  Prints the ratio line of each
    and collects the misses in ``late``: the bar (and its own 1e-4 cap), and the exact zeros."""
    for name, got, key, *slack in pairs:
        want, w32 = ref[F64][key], ref[F32][key].double()
        got = got.double().cpu().reshape(want.shape)
        scale = want.abs().max().item()
        e32 = (w32 - want).abs().max().item()
        err = (got - want).abs().max().item()
        if bf16:
            bar = 3e-2 * scale
        else:
            bar = min(MULT.get("%s.%s" % (family, name), 32) * e32 + 32 * 2.0 ** -24 * scale, 1e-4 * scale)
        print("cnn-pool-ratio %s %s %-7s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (family, tag, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        if not torch.isfinite(got).all():
            late.append("%s: unwritten or non-finite values" % name)
            continue
        zero = (want == 0) & (w32 == 0)
        if not (got[zero] == 0).all():
            late.append("%s: %d values are not exactly zero where the references are (largest %.3e)"
                        % (name, int((got[zero] != 0).sum()), got[zero].abs().max().item()))
        if scale == 0:
            continue
        if not err <= bar + sum(slack):
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))


# ---------------------------------------------------------------------- nr_cnn_keypool_*

KP_LENGTHS = (1, 2, 15, 16, 17, 31, 32)
KP_WIDTHS = {1: (32, 1, 20), 2: (64, 33), 3: (96, 65), 4: (128, 97), 5: (160, 129)}


def _kp_cases():
    out = []
    for nb in range(1, 6):
        i = 0
        for H in KP_WIDTHS[nb]:
            for pname, _ in PRECS:
                for save_k in (False, True):
                    out.append((nb, H, pname, save_k, KP_LENGTHS[i % 7], MASK_DTYPES[len(out) % 5],
                                (i // 2 + i) % 2 == 1))
                    i += 1
    return out


KP_CASES = _kp_cases()
for _p, _ in PRECS:         # every prec meets every mask dtype; every NB every length
    assert {c[5] for c in KP_CASES if c[2] == _p} == set(MASK_DTYPES)
for _nb in range(1, 6):
    assert {c[4] for c in KP_CASES if c[0] == _nb} == set(KP_LENGTHS)
    assert {(c[2], c[3]) for c in KP_CASES if c[0] == _nb} == {(p, k) for p, _ in PRECS for k in (False, True)}
assert {(c[3], c[6]) for c in KP_CASES} == {(a, b) for a in (False, True) for b in (False, True)}


def _kp_id(c):
    return "NB%d-H%d-%s-k%d-L%d-%s-dz%d" % (c[0], c[1], c[2], c[3], c[4], str(c[5]).split(".")[1], c[6])


def kp_case(nb, H, L, nseq, mdt, with_dz, start=0):
    """Seeded inputs, the mask and the float64 / float32 references of one keypool case."""
    Hp = 32 * nb
    assert 32 * (nb - 1) < H <= Hp
    mask = typed_mask(L, nseq, mdt, start=start)
    inp = cnn_keypool_inputs(nseq, L, H, 1000 * H + 10 * L + nseq)
    ref = {dt: cnn_keypool_reference(inp["C"], inp["wq"], inp["bq"], inp["q"], mask, inp["dnews"],
                                     inp["dz"] if with_dz else None, dtype=dt) for dt in (F64, F32)}
    return types.SimpleNamespace(nb=nb, Hp=Hp, H=H, L=L, n=nseq, T=nseq * L, mask=mask, inp=inp, ref=ref,
                                 with_dz=with_dz)


@functools.lru_cache(maxsize=None)
def grid_case(nb, H, nseq, mdt):
    """The grid-size cases share their references among the three precs."""
    return kp_case(nb, H, 5, nseq, mdt, True, start=2)


class KpOperands:
    """The padded operands of one case on the device, each inside its NaN frame."""

    def __init__(self, c):
        Hp, H = c.Hp, c.H
        self.C = Framed(c.T, Hp, 4, c.inp["C"])                       # ldc = Hp + 4, zero from H to Hp
        wq = torch.zeros(Hp, Hp)
        wq[:H, :H] = c.inp["wq"]
        self.wq = Vec(Hp * Hp, wq)
        self.bq = Vec(Hp, c.inp["bq"])
        self.q = Vec(H, c.inp["q"])
        self.mask = c.mask.cuda().reshape(-1).contiguous()
        self.mask_before = self.mask.clone()
        self.dnews = OffRows(c.inp["dnews"], H + 3)
        self.dz = Framed(c.T, H, 1, c.inp["dz"]) if c.with_dz else None
        self.wq2 = self.wq.v.view(Hp, Hp)

    def unchanged(self):
        ops = [self.C, self.wq, self.bq, self.q, self.dnews] + ([self.dz] if self.dz else [])
        return all(o.unchanged() for o in ops) and torch.equal(self.mask, self.mask_before)


def kp_forward(c, ops, prec, save_k):
    """One nr_cnn_keypool_fwd into framed NaN buffers and the checks every forward must pass."""
    from newsrec_amd import kernels as K
    news, probs = Framed(c.n, c.Hp, 1), Vec(c.T)
    kout = Framed(c.T, c.Hp, 4) if save_k else None
    K.cnn_keypool_fwd(ops.C.v, ops.wq2, ops.bq.v, ops.q.v, ops.mask, c.n, c.L, news.v, probs.v, qn=c.H, prec=prec,
                      kout=kout.v if save_k else None)
    torch.cuda.synchronize()
    assert ops.unchanged(), "the forward changed its inputs"
    assert news.frame_untouched(), "news: written outside its %d x %d view" % (c.n, c.Hp)
    assert probs.frame_untouched(), "probs: written outside its %d floats" % c.T
    assert kout is None or kout.frame_untouched(), "K: written outside its %d x %d view" % (c.T, c.Hp)
    return news, probs, kout


def kp_backward(c, ops, prec, probs, kin):
    """One nr_cnn_keypool_bwd into framed NaN buffers (the parameter gradients start NaN: they are stored)."""
    from newsrec_amd import kernels as K
    dc = Framed(c.T, c.Hp, 1)
    dwq, dbq, dq, dcb = Vec(c.Hp * c.Hp), Vec(c.Hp), Vec(c.H), Vec(c.H)
    before = probs.buf.clone(), (kin.buf.clone() if kin is not None else None)
    K.cnn_keypool_bwd(ops.C.v, ops.wq2, ops.bq.v, ops.q.v, c.n, c.L, c.H, probs.v, ops.dnews.v, dc.v,
                      dwq.v.view(c.Hp, c.Hp), dbq.v, dq.v, dcb.v, dz=ops.dz.v if ops.dz else None, prec=prec,
                      kin=kin.v if kin is not None else None)
    torch.cuda.synchronize()
    assert ops.unchanged() and _same_bits(before[0], probs.buf), "the backward changed its inputs"
    assert kin is None or _same_bits(before[1], kin.buf), "the backward changed K"
    for name, t in (("dc", dc), ("dwq", dwq), ("dbq", dbq), ("dq", dq), ("dconv_b", dcb)):
        assert t.frame_untouched(), "%s: written outside its view" % name
    return {"dc": dc.v, "dwq": dwq.v.view(c.Hp, c.Hp), "dbq": dbq.v, "dq": dq.v, "dconv_b": dcb.v}


def kp_check(c, pname, tag, news, probs, kout, grads):
    """Every output against the references, and the exact zeros at or past H."""
    H = c.H
    late = []
    pairs = [("news", news.v[:, :H], "news"), ("probs", probs.v, "probs")]
    past = [("news", news.v[:, H:])]
    if kout is not None:
        pairs.append(("K", kout.v[:, :H], "K"))
        past.append(("K", kout.v[:, H:]))
    if grads is not None:
        pairs += [("dc", grads["dc"][:, :H], "dc"), ("dwq", grads["dwq"][:H, :H], "dwq"),
                  ("dbq", grads["dbq"][:H], "dbq"), ("dq", grads["dq"], "dq"), ("dconv_b", grads["dconv_b"], "dconv_b")]
        past += [("dc", grads["dc"][:, H:]), ("dwq rows", grads["dwq"][H:]), ("dwq columns", grads["dwq"][:, H:]),
                 ("dbq", grads["dbq"][H:])]
    compare("kp-" + pname, tag, pairs, c.ref, late, bf16=pname == "bf16")
    for name, t in past:
        if not (t == 0).all():
            late.append("%s at or past H is not exactly zero" % name)
    empty = ((c.mask != 0).sum(1) == 0).nonzero().flatten().tolist()
    for s in empty:
        if not (news.v[s] == 0).all():
            late.append("news of the fully masked title %d is not zero" % s)
    assert not late, "; ".join(late)


@pytest.mark.parametrize("key", KP_CASES, ids=[_kp_id(c) for c in KP_CASES])
def test_cnn_keypool_small(key):
    nb, H, pname, save_k, L, mdt, with_dz = key
    c = kp_case(nb, H, L, 16, mdt, with_dz)
    ops = KpOperands(c)
    prec = dict(PRECS)[pname]
    news, probs, kout = kp_forward(c, ops, prec, save_k)
    grads = kp_backward(c, ops, prec, probs, kout)
    kp_check(c, pname, _kp_id(key), news, probs, kout, grads)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


GRID = [(nb, H, which, pname) for nb, H in ((1, 20), (5, 150)) for which in ("1", "7", "70", "3cus+5")
        for pname, _ in PRECS]


@pytest.mark.parametrize("nb,H,which,pname", GRID, ids=["NB%d-n%s-%s" % (g[0], g[2], g[3]) for g in GRID])
def test_cnn_keypool_grid(nb, H, which, pname):
    """Grid sizes around the reduce kernels' slices and the persistent loops' caps; the backward twice."""
    nseq = 3 * _cus() + 5 if which == "3cus+5" else int(which)
    i = GRID.index((nb, H, which, pname))
    c = grid_case(nb, H, nseq, MASK_DTYPES[(i // 3) % 5])
    ops = KpOperands(c)
    prec = dict(PRECS)[pname]
    save_k = i % 2 == 1
    news, probs, kout = kp_forward(c, ops, prec, save_k)
    grads = kp_backward(c, ops, prec, probs, kout)
    kp_check(c, pname, "NB%d-n%d-k%d" % (nb, nseq, save_k), news, probs, kout, grads)
    again = kp_backward(c, ops, prec, probs, kout)
    for name in ("dwq", "dbq", "dq", "dconv_b", "dc"):
        assert _same_bits(grads[name], again[name]), "%s differs between two calls" % name


def raw_forward(c, ops, nseq, prec, news, probs, kout):
    """nr_cnn_keypool_fwd itself (the wrapper sizes its checks by nseq; these tests pass another)."""
    from newsrec_amd import kernels as K
    mp, mdt = K.mask_arg(ops.mask, ops.mask.numel())
    p = LIB.ptr
    return LIB.load().nr_cnn_keypool_fwd(p(ops.C.v), ops.C.v.stride(0), p(ops.wq2), p(ops.bq.v), p(ops.q.v), c.H, mp, mdt,
                                         nseq, c.L, c.Hp, 1.0 / c.H ** 0.5, prec, p(news.v), news.v.stride(0),
                                         p(probs.v), p(kout.v), kout.v.stride(0), LIB.stream_ptr(ops.C.v))


def raw_backward(c, ops, nseq, prec, probs, out, ws, ws_floats, kin=None):
    """nr_cnn_keypool_bwd itself with the caller's workspace; out = (dc, dwq, dbq, dq, dconv_b)."""
    p = LIB.ptr
    dc, dwq, dbq, dq, dcb = out
    return LIB.load().nr_cnn_keypool_bwd(p(ops.C.v), ops.C.v.stride(0), p(ops.wq2), p(ops.bq.v), p(ops.q.v), c.H, nseq,
                                         c.L, c.Hp, c.H, 1.0 / c.H ** 0.5, prec, p(probs.v), p(ops.dnews.v),
                                         ops.dnews.v.stride(0), p(ops.dz.v) if ops.dz else None,
                                         ops.dz.v.stride(0) if ops.dz else 0, p(dc.v), dc.v.stride(0), p(dwq.v),
                                         p(dbq.v), p(dq.v), p(dcb.v), p(ws), ws_floats,
                                         p(kin.v) if kin is not None else None,
                                         kin.v.stride(0) if kin is not None else 0, LIB.stream_ptr(ws))


def _kp_outputs(c):
    return Framed(c.T, c.Hp, 1), Vec(c.Hp * c.Hp), Vec(c.Hp), Vec(c.H), Vec(c.H)


@pytest.mark.parametrize("nb,H", [(1, 20), (3, 96), (5, 150)])
def test_cnn_keypool_empty(nb, H):
    """nseq = 0 over operands of two titles: the forward returns before a launch (news, probs and K stay
    NaN); the backward launches one workgroup without titles and STORES zeros to dwq, dbq, dq and dconv_b (dc
    stays NaN), as include/newsrec_hip.h states."""
    c = kp_case(nb, H, 5, 2, torch.int64, True)
    ops = KpOperands(c)
    need = LIB.load().nr_cnn_keypool_workspace(0, c.Hp)
    for pname, prec in PRECS:
        news, probs, kout = Framed(c.n, c.Hp, 1), Vec(c.T), Framed(c.T, c.Hp, 4)
        assert raw_forward(c, ops, 0, prec, news, probs, kout) == 0
        torch.cuda.synchronize()
        for t in (news, probs, kout):
            assert _all_nan_bits(t.buf), "the forward of no titles wrote something"
        for kin in (None, kout):
            out = _kp_outputs(c)
            ws = _nan(need + 16)
            assert raw_backward(c, ops, 0, prec, probs, out, ws, need, kin=kin) == 0
            torch.cuda.synchronize()
            assert ops.unchanged()
            assert _all_nan_bits(out[0].buf), "dc written without a title"
            assert _all_nan_bits(ws[need:]), "the workspace was written past its stated size"
            for name, t in zip(("dwq", "dbq", "dq", "dconv_b"), out[1:]):
                assert t.frame_untouched() and (t.v == 0).all(), "%s is not stored as zeros" % name


@pytest.mark.parametrize("Hp", [32, 96, 160])
def test_cnn_keypool_workspace(Hp):
    """nr_cnn_keypool_workspace = (min(nseq, CUs) + 8) * (Hp^2 + 3 Hp) floats; the backward with one float
    less returns -1003 and writes nothing."""
    lib = LIB.load()
    cus = _cus()
    nws = Hp * Hp + 3 * Hp
    for nseq in (1, 7, 8, cus - 1, cus, cus + 1, 3 * cus + 5, 1 << 33):
        assert lib.nr_cnn_keypool_workspace(nseq, Hp) == (min(nseq, cus) + 8) * nws, nseq
    assert lib.nr_cnn_keypool_workspace(0, Hp) == 9 * nws          # the idle workgroup's partial
    H = Hp - 3
    c = kp_case(Hp // 32, H, 5, 7, torch.int64, False)
    ops = KpOperands(c)
    news, probs, _ = kp_forward(c, ops, LIB.GEMM_F32, False)
    need = lib.nr_cnn_keypool_workspace(c.n, Hp)
    ws = _nan(need + 16)
    out = _kp_outputs(c)
    assert raw_backward(c, ops, c.n, LIB.GEMM_F32, probs, out, ws, need - 1) == -1003
    torch.cuda.synchronize()
    for t in out:
        assert _all_nan_bits(t.buf), "a refused call wrote an output"
    assert _all_nan_bits(ws), "a refused call wrote its workspace"
    assert raw_backward(c, ops, c.n, LIB.GEMM_F32, probs, out, ws, need) == 0
    torch.cuda.synchronize()
    assert _all_nan_bits(ws[need:]), "the workspace was written past its stated size"
    late = []
    compare("kp-f32", "ws-Hp%d" % Hp, [("dwq", out[1].v.view(Hp, Hp)[:H, :H], "dwq"), ("dq", out[3].v, "dq")], c.ref,
            late)
    assert not late, "; ".join(late)


# ---------------------------------------------------------------------- nr_seq_pool_*

SP_MODES = ("tied", "tanh", "lin")        # K = X; a separate key stored as its tanh; a separate key, key_tanh = 0


def _r4(D):
    return (D + 3) // 4 * 4


def _qn_of(D, less):
    """qn = D, or a few features fewer."""
    return D if not less or D == 1 else (D - 3 if D > 4 else D - 1)


def _sp_wave_cases():
    out = []
    for lds in (((1, 256), (8, 150), (9, 253), (31, 3), (32, 6), (8, 1)),
                ((33, 253), (63, 6), (64, 3), (33, 256), (63, 1), (64, 150))):
        for i, (L, D) in enumerate(lds):
            out.append((1026, L, D, _qn_of(D, i in (2, 5)), SP_MODES[i % 3], i % 2 == 0, MASK_DTYPES[i % 5]))
    out.append((4 * 1024 + 3, 2, 6, 6, "tanh", True, torch.float64))     # the backward's second strided round
    return out


def _sp_wg_cases():
    out = []
    for nf, ds in ((1, (5, 150, 256)), (2, (257, 510, 512)), (4, (513, 1021, 1024))):
        for i, L in enumerate((1, 7, 8, 9, 63, 64)):
            D = ds[i % 3]
            out.append((8, L, D, _qn_of(D, i in (1, 5)), SP_MODES[(i + i // 3) % 3], i % 2 == 0,
                        MASK_DTYPES[(len(out) + nf) % 5]))
    return out


SP_WAVE, SP_WG = _sp_wave_cases(), _sp_wg_cases()
for _fam in ([c for c in SP_WAVE if c[1] <= 32], [c for c in SP_WAVE if c[1] > 32], SP_WG):
    assert {c[6] for c in _fam} == set(MASK_DTYPES)
    assert {c[4] for c in _fam} == set(SP_MODES)
    assert {(c[4] == "tied", c[5]) for c in _fam} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c[2] == c[3] for c in _fam} == {False, True}
for _fam in ([c for c in SP_WAVE if c[1] <= 32], [c for c in SP_WAVE if c[1] > 32]):
    assert {c[2] % 4 for c in _fam} == {0, 1, 2, 3}
for _nf in (1, 2, 4):
    assert {c[1] for c in SP_WG if (c[2] + 255) // 256 in ((_nf,) if _nf < 4 else (3, 4))} == {1, 7, 8, 9, 63, 64}


def _sp_id(c):
    return "n%d-L%d-D%d-qn%d-%s-dz%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], str(c[6]).split(".")[1])


def _sp_family(nseq, L, D):
    if D > 256 or nseq < 1024:
        return "sp-wg%d" % (1 if D <= 256 else 2 if D <= 512 else 4)
    return "sp-wave%d" % (32 if L <= 32 else 64)


def run_seq_pool(key):
    from newsrec_amd import kernels as K
    nseq, L, D, qn, mode, with_dz, mdt = key
    T, ld = nseq * L, _r4(D) + 4
    family, tag = _sp_family(nseq, L, D), _sp_id(key)
    mask = typed_mask(L, nseq, mdt)
    inp = attn_pool_inputs(nseq, L, D, 100 * L + D)
    for k in ("x", "key", "q", "dout"):              # zero-padded columns from qn to D
        inp[k][..., qn:] = 0
    keyt = None if mode == "tied" else inp["key"]
    scale = 1.0 / qn ** 0.5
    ref = {dt: attn_pool_reference(inp["x"], keyt, inp["q"], mask, None, None, None, 0, scale, mode == "tanh",
                                   dout=inp["dout"], dz=inp["dz"] if with_dz else None, dtype=dt) for dt in (F64, F32)}
    g = torch.Generator().manual_seed(D)
    dq0 = torch.randn(qn, generator=g) * 0.5

    x = Framed(T, D, ld - D, inp["x"])
    kk = Framed(T, D, ld - D, keyt) if keyt is not None else None
    q = Vec(qn, inp["q"][:qn])
    m = mask.cuda().reshape(-1).contiguous()
    out, probs = Framed(nseq, D, ld - D), Vec(T)
    K.seq_pool_fwd(x.v, q.v, m, nseq, L, D, out.v, probs.v, key=kk.v if kk else None, scale=scale, qn=qn)
    torch.cuda.synchronize()
    reads = [x, q] + ([kk] if kk else [])
    assert all(t.unchanged() for t in reads), "the forward changed its inputs"
    assert out.frame_untouched(), "out: written outside its %d x %d view" % (nseq, D)
    assert probs.frame_untouched(), "probs: written outside its %d floats" % T

    dout = OffRows(inp["dout"][:, :qn], qn + 1)
    dz = Framed(T, D, ld - D, inp["dz"]) if with_dz else None
    dx = Framed(T, D, ld - D)
    dk = Framed(T, D, ld - D) if kk else None
    dq = Vec(qn, dq0)
    pb = probs.buf.clone()
    K.seq_pool_bwd(x.v, q.v, m, nseq, L, D, probs.v, dout.v, dx.v, dq.v, key=kk.v if kk else None,
                   dk=dk.v if dk else None, key_tanh=mode == "tanh", dz=dz.v if dz else None, scale=scale, qn=qn)
    torch.cuda.synchronize()
    reads += [dout] + ([dz] if dz else [])
    assert all(t.unchanged() for t in reads) and _same_bits(pb, probs.buf), "the backward changed its inputs"
    assert dx.frame_untouched(), "dx: written outside its view"
    assert dk is None or dk.frame_untouched(), "dk: written outside its view"
    assert dq.frame_untouched(), "dq: written past qn"

    # dq: one accumulating addition per workgroup onto the start (dq_slack of the module docstring)
    per = seq_pool_dq_per_seq(inp["x"], keyt, inp["q"], ref[F64]["probs"], inp["dout"], scale)[:, :qn]
    adds = nseq if family.startswith("sp-wg") else min((nseq + 3) // 4, 1024)
    dq_slack = adds * 2.0 ** -24 * (dq0.double().abs() + per.abs().sum(0)).max().item()
    for r in ref.values():
        r["dq"] = r["dq"][:qn]
    pairs = [("out", out.v, "out"), ("probs", probs.v, "probs"), ("dx", dx.v, "dx"),
             ("dq", dq.v.double().cpu() - dq0.double(), "dq", dq_slack)]
    if dk is not None:
        pairs.append(("dk", dk.v, "dk"))
    late = []
    compare(family, tag, pairs, ref, late)
    if not (out.v[0] == 0).all():
        late.append("out of the empty sequence is not zero")
    assert not late, "; ".join(late)


@pytest.mark.parametrize("key", SP_WAVE, ids=[_sp_id(c) for c in SP_WAVE])
def test_seq_pool_wave(key):
    assert _sp_family(*key[:3]).startswith("sp-wave")
    run_seq_pool(key)


@pytest.mark.parametrize("key", SP_WG, ids=[_sp_id(c) for c in SP_WG])
def test_seq_pool_workgroup(key):
    assert _sp_family(*key[:3]).startswith("sp-wg")
    run_seq_pool(key)
