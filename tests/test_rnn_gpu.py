"""The recurrent kernels (csrc/rnn.hip) called directly, K.rnn_fwd / K.rnn_bwd with gx supplied by
the test (no GEMM in the path), against the float64 reference of tests/rnn_util.py, and the autograd
wrapper RNNUserFn through RNN_User_Encoder / LSTUR_User_Encoder at a width that pads (150) and one
that does not (64), against oracle.restatement.

Which kernel a case launches (nr_rnn_fwd / nr_rnn_bwd dispatch on H alone):
  H == 150         rnn_fwd_reg_kernel<150,4,88> / rnn_bwd_reg_kernel<150,4>  (LSTM)
                   rnn_fwd_reg_kernel<150,3,150> / rnn_bwd_reg_kernel<150,3> (GRU)
  H != 150         rnn_fwd_kernel / rnn_bwd_kernel, one hidden unit per thread for H <= 256
                   (3, 64, 160 here), two for H > 256 (257, 512)

The bar of the kernel-level cases is tied to the reference: the same reference evaluated in float32
on the CPU differs from float64 by e32 = max|ref32 - ref64| per tensor, and the kernel must stay
within 32 e32 + 32 * 2^-24 * max|ref64| (the fast-exponential sigmoid and another summation order
compound over the steps as float32 rounding does; the additive floor covers a luckily tiny e32).
That bar may itself never exceed 1e-4 * max|ref64|, the level of the model tests.  Every case
prints its err / e32 ratios ("rnn-ratio" lines, pytest -s).  Measured on an MI355X, the largest
ratio of any case and tensor: 1.6 on the reg kernels (both cells), 3.6 (LSTM) and 8.9 (GRU, dgi at
H = 257) on the generic ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from rnn_util import gates_per_cell, rnn_inputs, rnn_reference

NAN = float("nan")
PAD_GX, PAD_H, PAD_DG = 5, 3, 7      # leading dimensions wider than the row by these many floats

REG = dict(H=150, N=50, lens=(0, 1, 50, 49, 7, 23))
GEN_LENS = (0, 1, 9, 8, 4, 2)
N1_LENS = (0, 1, 1)

# reverse, mask dtype (None: no mask, every sequence runs all N steps), h0 (none | rows: [B, H] without
# h0_idx | idx: a table through h0_idx with a repeated id and id 0), b_hh given, dgh given for the LSTM
# (the GRU needs it), dh0 requested
VARIANTS = {
    "fwd": dict(reverse=False, mask=torch.uint8, h0="none", bias=True, dgh=True, dh0=False),
    "rev": dict(reverse=True, mask=torch.float64, h0="rows", bias=True, dgh=False, dh0=True),
    "lstur": dict(reverse=True, mask=None, h0="idx", bias=True, dgh=False, dh0=True),
    "nobias": dict(reverse=False, mask=torch.int64, h0="rows", bias=False, dgh=True, dh0=True),
    "rev_nobias": dict(reverse=True, mask=torch.float32, h0="none", bias=False, dgh=True, dh0=True),
}
ALL = tuple(VARIANTS)


def _shapes():
    out = [(REG["H"], REG["N"], REG["lens"], v) for v in ALL]                       # reg kernels
    out += [(H, 9, GEN_LENS, v) for H in (64, 257) for v in ALL]                     # generic, 1 and 2 units/thread
    out += [(H, 9, GEN_LENS, v) for H in (3, 160, 512) for v in ("fwd", "rev")]
    out += [(H, 1, N1_LENS, v) for H in (150, 64) for v in ("fwd", "rev", "lstur")]  # N = 1
    return out


CASES = [(cell,) + s for cell in ("lstm", "gru") for s in _shapes()]
TABLE_IDX = (2, 0, 2, 3, 1, 0)       # h0_idx: a repeated id and id 0 within the first three (B = 3 at N = 1)


def _cell_code(cell):
    from newsrec_amd import _lib as L
    return L.CELL_LSTM if cell == "lstm" else L.CELL_GRU


def _nan(rows, cols):
    return torch.full((rows, cols), NAN, device="cuda")


def _padded(t, pad):
    """t on the device inside a NaN buffer ``pad`` columns wider; -> (buffer, the view holding t)."""
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def prefix_mask(lens, N, dtype=torch.uint8):
    m = torch.zeros(len(lens), N, dtype=dtype)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


def holes_mask(lens, N, dtype=torch.uint8):
    """The same count of ones per row at seeded random slots; not a prefix wherever 0 < len < N."""
    g = torch.Generator().manual_seed(1234)
    m = prefix_mask(lens, N, dtype)
    for b, n in enumerate(lens):
        if 0 < n < N:
            while bool((m[b, :n] != 0).all()):
                m[b] = m[b][torch.randperm(N, generator=g)]
    return m


def run_kernels(cell, H, N, lens, inp, reverse, mask, h0, h0_idx, bias, dgh, dh0):
    """One nr_rnn_fwd and one nr_rnn_bwd (on the forward's own saved tensors, as RNNUserFn runs them)
    into NaN-filled buffers -> {name: the whole buffer on the CPU, the padding columns included}."""
    from newsrec_amd import kernels as K
    c, G, B = _cell_code(cell), gates_per_cell(cell), len(lens)
    GH = G * H
    _, gx = _padded(inp["gx"], PAD_GX)
    whh = inp["w_hh"].cuda()
    bhh = inp["b_hh"].cuda() if bias else None
    gates, hprev = _nan(B * N, 4 * H), _nan(B * N, H)
    cprev = _nan(B * N, H) if cell == "lstm" else None
    hout = _nan(B, H + PAD_H)
    h0_d = _padded(h0, PAD_H)[1] if h0 is not None else None
    idx_d = h0_idx.cuda() if h0_idx is not None else None
    mask_d = mask.cuda() if mask is not None else None
    K.rnn_fwd(c, gx, whh.t().contiguous(), bhh, B, N, H, gates, hprev, cprev, hout[:, :H], h0=h0_d, h0_idx=idx_d,
              mask=mask_d, reverse=reverse)
    _, dhout = _padded(inp["dhout"], PAD_H)
    dgi = _nan(B * N, GH + PAD_DG)
    dgh_b = _nan(B * N, GH + PAD_DG) if (dgh or cell == "gru") else None
    dh0_b = _nan(B, H + PAD_H) if dh0 else None
    K.rnn_bwd(c, whh, gates, hprev, cprev, B, N, H, dhout, dgi[:, :GH], dgh=dgh_b[:, :GH] if dgh_b is not None else None,
              dh0=dh0_b[:, :H] if dh0_b is not None else None, mask=mask_d, reverse=reverse)
    torch.cuda.synchronize()
    out = dict(hout=hout, gates=gates, hprev=hprev, cprev=cprev, dgi=dgi, dgh=dgh_b, dh0=dh0_b)
    return {k: v.cpu() for k, v in out.items() if v is not None}


def _setup(cell, H, N, lens, variant):
    v = VARIANTS[variant]
    B = len(lens)
    if v["mask"] is None:
        lens = (N,) * B
    seed = 1000 * H + 10 * N + (7 if cell == "gru" else 0) + ALL.index(variant)
    inp = rnn_inputs(cell, B, N, H, seed, table_rows=4 if v["h0"] == "idx" else None)
    h0 = inp["h0"] if v["h0"] != "none" else None
    h0_idx = torch.tensor(TABLE_IDX[:B]) if v["h0"] == "idx" else None
    h0_rows = None if h0 is None else (h0[h0_idx] if h0_idx is not None else h0)
    mask = prefix_mask(lens, N, v["mask"]) if v["mask"] is not None else None
    run = lambda m=mask: run_kernels(cell, H, N, lens, inp, v["reverse"], m, h0, h0_idx, v["bias"], v["dgh"], v["dh0"])
    return v, lens, inp, h0_rows, run


def check_layout(out, cell, H, N, lens, reverse, inp, h0_rows):
    """The exact properties: nothing written past a row's valid width, everything inside it written,
    the rows of steps that do not run exactly zero, and len == 0 passes h0 / dhout through bit for bit."""
    GH = gates_per_cell(cell) * H
    for name, width in (("hout", H), ("gates", 4 * H), ("hprev", H), ("cprev", H), ("dgi", GH), ("dgh", GH), ("dh0", H)):
        if name in out:
            assert torch.isnan(out[name][:, width:]).all(), "%s: written past column %d" % (name, width)
            assert torch.isfinite(out[name][:, :width]).all(), "%s: unwritten or non-finite values" % name
    for b, n in enumerate(lens):
        rows = [b * N + (N - 1 - t if reverse else t) for t in range(n, N)]
        for name, width in (("gates", 4 * H), ("hprev", H), ("cprev", H), ("dgi", GH), ("dgh", GH)):
            if name in out and rows:
                assert (out[name][rows, :width] == 0).all(), "%s: padded rows of sequence %d not zero" % (name, b)
        if n == 0:
            want = h0_rows[b] if h0_rows is not None else torch.zeros(H)
            assert _bits_equal(out["hout"][b, :H], want), "hout of the empty sequence %d is not its h0" % b
            if "dh0" in out:
                assert _bits_equal(out["dh0"][b, :H], inp["dhout"][b]), "dh0 of the empty sequence %d is not dhout" % b


@pytest.mark.parametrize("cell,H,N,lens,variant", CASES,
                         ids=["%s-H%d-N%d-%s" % (c[0], c[1], c[2], c[4]) for c in CASES])
def test_kernels_vs_reference(cell, H, N, lens, variant):
    v, lens, inp, h0_rows, run = _setup(cell, H, N, lens, variant)
    out = run()
    check_layout(out, cell, H, N, lens, v["reverse"], inp, h0_rows)
    GH = gates_per_cell(cell) * H
    if cell == "lstm" and v["dgh"]:
        assert _bits_equal(out["dgh"], out["dgi"]), "LSTM: dgh differs from dgi"

    bias = inp["b_hh"] if v["bias"] else None
    ref = {dt: rnn_reference(cell, inp["gx"], inp["w_hh"], bias, h0_rows, lens, v["reverse"], dhout=inp["dhout"], dtype=dt)
           for dt in (torch.float64, torch.float32)}
    late = []
    for name, width in (("hout", H), ("gates", 4 * H), ("hprev", H), ("cprev", H), ("dgi", GH), ("dgh", GH), ("dh0", H)):
        if name not in out:
            continue
        want = ref[torch.float64][name]
        scale = want.abs().max().item()
        e32 = (ref[torch.float32][name].double() - want).abs().max().item()
        bar = 32 * e32 + 32 * 2.0 ** -24 * scale
        err = (out[name][:, :width].double() - want).abs().max().item()
        print("rnn-ratio %s-H%d-N%d-%s %-5s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (cell, H, N, variant, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        if not err <= bar:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))
    assert not late, "; ".join(late)

    again = run()                      # no floating-point atomics: a second call gives the same bits
    for name in out:
        assert _bits_equal(out[name], again[name]), "%s differs between two calls" % name


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("H,N,lens", [(150, 50, REG["lens"]), (64, 9, GEN_LENS), (257, 9, GEN_LENS)],
                         ids=["reg-H150", "generic-H64", "generic-H257"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_mask_dtypes_and_holes(cell, H, N, lens, reverse):
    """len = count of nonzero mask[b, :], whatever the dtype and wherever the ones sit: every mask form
    gives the bits of the uint8 prefix mask (which test_kernels_vs_reference holds to the reference)."""
    B = len(lens)
    inp = rnn_inputs(cell, B, N, H, 77 + H + reverse)
    run = lambda m: run_kernels(cell, H, N, lens, inp, reverse, m, inp["h0"], None, True, True, True)
    base = run(prefix_mask(lens, N))
    check_layout(base, cell, H, N, lens, reverse, inp, inp["h0"])
    holes = holes_mask(lens, N)
    assert not torch.equal(holes, prefix_mask(lens, N)) and torch.equal(holes.sum(1), prefix_mask(lens, N).sum(1))
    forms = {
        "bool": prefix_mask(lens, N, torch.bool),
        "int64": prefix_mask(lens, N, torch.int64),
        "float64": prefix_mask(lens, N, torch.float64),
        "float32": prefix_mask(lens, N, torch.float32),
        "float64 [B,N,1]": prefix_mask(lens, N, torch.float64).unsqueeze(-1),     # as _his_mask_rows is fed
        "float64 [B*N]": prefix_mask(lens, N, torch.float64).reshape(B * N),      # as it returns
        "holes uint8": holes,
        "holes float64 (values 2.5, -1)": holes.double() * torch.where(torch.arange(N) % 2 == 0, 2.5, -1.0),
        "holes int64 (value 1 << 40)": holes.long() << 40,                        # nonzero only above bit 32
    }
    for form, m in forms.items():
        got = run(m)
        for name in base:
            assert _bits_equal(got[name], base[name]), "%s: %s differs from the uint8 prefix mask's" % (form, name)


# ---------------------------------------------------------------------- the autograd wrapper

@pytest.fixture(params=["bf16x6", "f32"])
def gemm_prec(request):
    """Both GEMM arithmetics, as in tests/test_model_gpu.py."""
    from newsrec_amd import _lib as Lb, kernels as Kn
    old = Kn.set_gemm_precision(Lb.GEMM_BF16X6 if request.param == "bf16x6" else Lb.GEMM_F32)
    yield request.param
    Kn.set_gemm_precision(old)


MB, MN, MLENS = 4, 12, (1, 12, 5, 0)
USER_NUM = 6
USER_ID = (3, 5, 3, 2)               # a duplicate id ...
USER_KEEP = (1, 0, 1, 1)             # ... and a dropped one (-> row 0)


def _encoder(enc, hidden):
    """The user encoder on the device with seeded parameters at the goldens' scales
    (tests/golden/params.py), and the same parameters in float64 under the oracle's names."""
    from newsrec_amd import encoders as E
    from model_util import Cfg
    from params import param_std
    kind = enc.split("_")[0]
    m = Cfg("cnn", kind, hidden, descend_history=enc.endswith("descend"), user_num=USER_NUM)
    mod = (E.LSTUR_User_Encoder if kind == "lstur" else E.RNN_User_Encoder)(m).cuda()
    g = torch.Generator().manual_seed(hidden + len(enc))
    P = {}
    with torch.no_grad():
        for n, p in mod.named_parameters():
            v = torch.randn(p.shape, generator=g) * float(param_std(n, tuple(p.shape)))
            if "userEmbedding" in n:
                v[0] = 0.0
            p.copy_(v)
            P["encoderU." + n] = v.double().requires_grad_()
    return mod, P, g


@pytest.mark.parametrize("hidden", [64, 150])
@pytest.mark.parametrize("enc", ["lstm", "lstm_descend", "gru", "gru_descend", "lstur"])
def test_user_encoder_modules(enc, hidden, gemm_prec):
    """hidden 64: RNNUserFn's unpadded GEMM branches and the generic kernels; 150: the padded branches
    and the reg kernels; descend_history = reverse with a mask; lens include 0 (the oracle, like the
    kernels, then outputs h0 = 0 and no gradient)."""
    from oracle import restatement as R
    mod, P, g = _encoder(enc, hidden)
    his = torch.randn(MB, MN, hidden, generator=g)
    wgt = torch.randn(MB, 1, hidden, generator=g)
    his_mask = prefix_mask(MLENS, MN, torch.float64).unsqueeze(-1)           # [B, N, 1] f64 on the CPU
    x = his.cuda().requires_grad_()
    x64 = his.double().requires_grad_()
    if enc == "lstur":
        uid, keep = torch.tensor(USER_ID), torch.tensor(USER_KEEP)
        mod.keep_override = keep
        out = mod(x, his_mask=his_mask, user_id=uid)
        want = R.lstur_user(x64, uid, keep, P)
    else:
        out = mod(x, his_mask=his_mask)
        want = R.rnn_user(x64, his_mask, P, enc.split("_")[0], descend=enc.endswith("descend"))
    assert out.shape == (MB, 1, hidden)
    (out * wgt.cuda()).sum().backward()
    (want * wgt.double()).sum().backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(out.detach().cpu().double(), want.detach(), rtol=0, atol=1e-4)
    grads = {"input": (x.grad, x64.grad)}
    for n, p in mod.named_parameters():
        grads[n] = (p.grad, P["encoderU." + n].grad)
    assert set(grads) >= {"input", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"}
    assert (enc == "lstur") == ("userEmbedding.weight" in grads)
    for n, (got, ref) in grads.items():
        assert got is not None and ref is not None, n
        scale = ref.abs().max().item()
        assert scale > 0, n
        torch.testing.assert_close(got.cpu().double(), ref, rtol=0, atol=1e-3 * scale, msg=lambda s, n=n: n + ": " + s)
