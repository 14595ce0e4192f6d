"""Return codes of the entry points of csrc/score_adam.hip for invalid (and empty) arguments, as
include/newsrec_hip.h documents them.  Every argument check, and every empty case (B = 0, n = 0,
rows = 0, cols = 0), returns before any HIP call, so the entries run through ctypes on a machine
without a GPU: the operands sit on a 16-B-aligned HOST buffer that no case ever dereferences (the
mechanism of test_gemm_args_cpu.py).  No case here passes a complete valid non-empty argument list:
that would launch.

-1000 is a bad size / mode, -1001 a NULL pointer, -1002 (nr_adam) a pointer off a 16-byte boundary."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
MAXC = 16 * 1024                                 # the scorer's LDS cap on C
BAD, NULL, ALIGN, OK = -1000, -1001, -1002, 0


def _call(name, args):
    """The raw return code (L.call raises on a non-zero one)."""
    return getattr(L.load(), name)(*args)


def _with(base, **kw):
    a = dict(base)
    for k in kw:
        assert k in a, k
    a.update(kw)
    return a


def _cases(base, bad=(), null=(), ok=()):
    """[(id, args dict, expected code)]: each entry of ``bad`` / ``ok`` is a dict of overrides, each
    name in ``null`` a pointer argument set to NULL."""
    def label(kw):   # the buffer's address changes from run to run: a test id names it "P"
        return ", ".join("%s=%s" % (k, "P" if v is P else v) for k, v in kw.items())

    out = []
    for kw in bad:
        out.append((label(kw), _with(base, **kw), BAD))
    for name in null:
        out.append((name + "=NULL", _with(base, **{name: None}), NULL))
    for kw in ok:
        out.append((label(kw) + " -> OK", _with(base, **kw), OK))
    return out


# ---- argument lists in ABI order (dict order is the call order); the stream is NULL everywhere
SCORE_FWD = dict(cdd=P, ldc=8, cdd_idx=None, user=P, ldu=8, B=2, C=5, H=8, mode=L.SCORE_LOG_SOFTMAX, logits=P,
                 stream=None)
SCORE_BWD = dict(cdd=P, ldc=8, user=P, ldu=8, logits=P, dlogits=P, B=2, C=5, H=8, mode=L.SCORE_SIGMOID, dcdd=P,
                 lddc=8, duser=P, lddu=8, stream=None)
NLL_FWD = dict(cdd=P, ldc=8, user=P, ldu=8, label=P, B=2, C=5, H=8, logits=P, loss=P, work=P, stream=None)
NLL_BWD = dict(cdd=P, ldc=8, user=P, ldu=8, logits=P, label=P, dloss=P, dlogits=P, B=2, C=5, H=8, dcdd=P, lddc=8,
               duser=P, lddu=8, stream=None)
ADAM = dict(param=P, grad=P + 64, exp_avg=P + 128, exp_avg_sq=P + 192, n=8, lr=1e-3, beta1=0.9, beta2=0.999,
            eps=1e-8, weight_decay=0.0, step=1, step_dev=None, grad_scale=1.0, stream=None)
EMB_FWD = dict(table=P, V=10, E=8, idx=P, n=4, out=P, stream=None)
EMB_BWD = dict(dout=P, V=10, E=3, idx=P, n=4, padding_idx=0, dtable=P, stream=None)
ROWS_ADD = dict(dout=P, ldo=8, V=10, E=8, idx=P, n=4, padding_idx=-1, dtable=P, ldt=8, stream=None)
XS_FWD = dict(x=P, mask=P, mask_dtype=L.MASK_I64, rows=3, cols=5, out=P, stream=None)
XS_BWD = dict(y=P, dy=P, rows=3, cols=5, dx=P, stream=None)
GATHER = dict(src=P, lds=8, V=10, idx=P, n=4, cols=8, dst=P, ldd=8, stream=None)
TRANSPOSE = dict(src=P, lds=8, rows=4, cols=8, dst=P, ldd=4, stream=None)
COLSUM = dict(x=P, ldx=8, rows=4, cols=8, out=P, work=P, stream=None)
COLSUM_WS = dict(x=P, ldx=8, rows=4, cols=8, out=P, work=P, tick=P, stream=None)

_SCORE_BAD = (dict(B=-1), dict(C=0), dict(C=-3), dict(C=MAXC + 1), dict(H=0))
_MODE_BAD = (dict(mode=-1), dict(mode=3))

TABLE = {
    "nr_score_fwd": _cases(
        SCORE_FWD, bad=_SCORE_BAD + _MODE_BAD, null=("cdd", "user", "logits"),
        ok=(dict(B=0), dict(B=0, C=MAXC), dict(B=0, cdd_idx=P))),
    "nr_score_bwd": _cases(
        SCORE_BWD, bad=_SCORE_BAD + _MODE_BAD, null=("cdd", "user", "logits", "dlogits", "dcdd", "duser"),
        ok=(dict(B=0), dict(B=0, C=MAXC))),
    # the fused loss has no empty case: the mean over B = 0 impressions is refused
    "nr_score_nll_fwd": _cases(
        NLL_FWD, bad=_SCORE_BAD + (dict(B=0), dict(B=2 ** 31)),
        null=("cdd", "user", "label", "logits", "loss", "work")),
    "nr_score_nll_bwd": _cases(
        NLL_BWD, bad=_SCORE_BAD, null=("cdd", "user", "logits", "label", "dcdd", "duser"),
        ok=(dict(B=0), dict(B=0, C=MAXC), dict(B=0, dloss=None, dlogits=None))),
    "nr_adam": _cases(
        ADAM, bad=(dict(n=-1), dict(step=0), dict(step=-2)), null=("param", "grad", "exp_avg", "exp_avg_sq"),
        ok=(dict(n=0), dict(n=0, step=0, step_dev=P))),
    "nr_embedding_fwd": _cases(
        EMB_FWD, bad=(dict(V=0), dict(E=0), dict(E=3), dict(E=6), dict(n=-1)), null=("table", "idx", "out"),
        ok=(dict(n=0),)),
    "nr_embedding_bwd": _cases(
        EMB_BWD, bad=(dict(V=0), dict(E=0), dict(n=-1)), null=("dout", "idx", "dtable"), ok=(dict(n=0),)),
    "nr_rows_add_ordered": _cases(
        ROWS_ADD, bad=(dict(V=0), dict(E=0), dict(n=-1), dict(n=(1 << 20) + 1), dict(ldo=7), dict(ldt=7)),
        null=("dout", "idx", "dtable"), ok=(dict(n=0),)),
    "nr_xsoftmax_fwd": _cases(
        XS_FWD, bad=(dict(rows=-1), dict(cols=-1), dict(mask_dtype=-1), dict(mask_dtype=4)),
        null=("x", "mask", "out"), ok=(dict(rows=0), dict(cols=0))),
    "nr_xsoftmax_bwd": _cases(
        XS_BWD, bad=(dict(rows=-1), dict(cols=-1)), null=("y", "dy", "dx"), ok=(dict(rows=0), dict(cols=0))),
    "nr_gather_rows_f32": _cases(
        GATHER, bad=(dict(n=-1), dict(cols=-1), dict(V=0), dict(lds=7), dict(ldd=7)), null=("src", "idx", "dst"),
        ok=(dict(n=0), dict(cols=0))),
    "nr_transpose_f32": _cases(
        TRANSPOSE, bad=(dict(rows=-1), dict(cols=-1), dict(lds=7), dict(ldd=3), dict(rows=65535 * 64 + 1, ldd=1 << 23),
                        dict(cols=(1 << 31) + 1, lds=1 << 32)),
        null=("src", "dst"), ok=(dict(rows=0), dict(cols=0))),
    "nr_colsum": _cases(
        COLSUM, bad=(dict(rows=-1), dict(cols=-1), dict(ldx=7)), null=("x", "out", "work"),
        ok=(dict(rows=0), dict(cols=0), dict(rows=0, work=None), dict(cols=0, work=None))),
    "nr_colsum_ws": _cases(
        COLSUM_WS, bad=(dict(rows=-1), dict(cols=-1), dict(ldx=7)), null=("x", "out", "work", "tick"),
        ok=(dict(rows=0), dict(cols=0), dict(rows=0, work=None, tick=None), dict(cols=0, work=None, tick=None))),
}

ALL = [(name, cid, args, want) for name, cases in TABLE.items() for cid, args, want in cases]


@pytest.mark.parametrize("name,cid,args,want", ALL, ids=["%s: %s" % (c[0], c[1]) for c in ALL])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    assert _call(name, list(args.values())) == want


def test_adam_alignment_rule():
    """nr_adam reads float4: each of the four pointers must sit on a 16-byte boundary (-1002), checked
    after the sizes and the NULL pointers and before the empty case."""
    for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
        for off in (4, 8, 12):
            assert _call("nr_adam", list(_with(ADAM, **{k: ADAM[k] + off}).values())) == ALIGN, (k, off)
        assert _call("nr_adam", list(_with(ADAM, n=0, **{k: ADAM[k] + 4}).values())) == ALIGN, k
    assert _call("nr_adam", list(_with(ADAM, n=-1, param=P + 4).values())) == BAD
    assert _call("nr_adam", list(_with(ADAM, grad=None, param=P + 4).values())) == NULL


def test_sizes_are_checked_before_pointers():
    """Code 0 wins over code 1: a bad size with a NULL pointer reports the size."""
    assert _call("nr_score_fwd", list(_with(SCORE_FWD, C=MAXC + 1, cdd=None).values())) == BAD
    assert _call("nr_score_bwd", list(_with(SCORE_BWD, C=MAXC + 1, duser=None).values())) == BAD
    assert _call("nr_score_nll_bwd", list(_with(NLL_BWD, C=MAXC + 1, label=None).values())) == BAD
    assert _call("nr_gather_rows_f32", list(_with(GATHER, lds=7, src=None).values())) == BAD
    # ... and a NULL pointer over the empty case
    assert _call("nr_score_fwd", list(_with(SCORE_FWD, B=0, user=None).values())) == NULL
    assert _call("nr_xsoftmax_bwd", list(_with(XS_BWD, rows=0, dx=None).values())) == NULL
    assert _call("nr_colsum", list(_with(COLSUM, rows=0, out=None).values())) == NULL


def test_workspace_sizes_of_empty_problems():
    lib = L.load()
    assert lib.nr_colsum_workspace(0, 8) == 0 and lib.nr_colsum_workspace(4, 0) == 0
    assert lib.nr_colsum_workspace(-1, 8) == 0 and lib.nr_colsum_workspace(4, 8) >= 8 * 4
    assert lib.nr_score_nll_workspace(0) == 4 and lib.nr_score_nll_workspace(-5) == 4
    assert lib.nr_score_nll_workspace(7) == 4 + 2 * 7
