"""Return codes of the four GEMM entry points for invalid (and empty) arguments.  Every argument
check returns before any HIP call, so the entries run through ctypes on a machine without a GPU:
the operands sit on a 16-B-aligned HOST buffer that no case ever dereferences.

The static form is reached through nr_gemm_f32 and through nr_gemm_f32_ws with m_dev = k_dev = NULL
and max_cus = 0; the dynamic form through nr_gemm_f32_dyn, nr_gemm_f32_dyn_cus and nr_gemm_f32_ws
with max_cus = 3 or a non-null m_dev.  The two forms differ on purpose in places (a bad `prec` is
argument 12 in one and 14 in the other, K % 32 and ld % 4 are dynamic-form rules, K == 0 ...)."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
_BASE = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "operand" memory
_ROWS = _BASE + 2048                                  # a row table (never read)
_MDEV = ctypes.c_int32(4)                             # stands in for a device-resident M (never read)


def _op(layout=L.KCONTIG, mapping=L.ROWS_PLAIN, ld=32, seq_len=1, seg=1, data=_BASE):
    rows = _ROWS if mapping != L.ROWS_PLAIN else None
    return L.nr_operand(data, ld, rows, mapping, seq_len, seg, layout)


def _args(**kw):
    a = dict(M=4, N=4, K=32, A=_op(), B=_op(), C=_BASE + 1024, ldc=32, bias=None, epilogue=L.EPI_STORE,
             c_rows=None, pad_row=-1, split_k=1, prec=L.GEMM_BF16X6)
    a.update(kw)
    return a


def _call(name, *args):
    """The raw return code (L.call raises on a non-zero one)."""
    lib = L.load()
    return getattr(lib, name)(*args)


def _head(a):
    return (a["M"], a["N"], a["K"], ctypes.byref(a["A"]) if a["A"] is not None else None,
            ctypes.byref(a["B"]) if a["B"] is not None else None, a["C"], a["ldc"], a["bias"], a["epilogue"],
            ctypes.byref(a["c_rows"]) if a["c_rows"] is not None else None, a["pad_row"], a["split_k"])


def _static_codes(a):
    return {
        "nr_gemm_f32": _call("nr_gemm_f32", *_head(a), a["prec"], None),
        "nr_gemm_f32_ws": _call("nr_gemm_f32_ws", *_head(a), None, None, a["prec"], 0, None, 0, None, None, None),
    }


def _dyn_codes(a, max_cus=0):
    """The dynamic form; max_cus != 0 is the case's subject where given (then nr_gemm_f32_dyn has no say)."""
    out = {}
    if max_cus == 0:
        out["nr_gemm_f32_dyn"] = _call("nr_gemm_f32_dyn", *_head(a), None, None, a["prec"], None)
    out["nr_gemm_f32_dyn_cus"] = _call("nr_gemm_f32_dyn_cus", *_head(a), None, None, a["prec"], max_cus, None)
    out["nr_gemm_f32_ws max_cus"] = _call("nr_gemm_f32_ws", *_head(a), None, None, a["prec"], max_cus or 3, None, 0,
                                          None, None, None)
    if max_cus == 0:
        out["nr_gemm_f32_ws m_dev"] = _call("nr_gemm_f32_ws", *_head(a), ctypes.byref(_MDEV), None, a["prec"], 0,
                                            None, 0, None, None, None)
    return out


_CONV_KC = dict(M=64, N=64, K=96, A=_op(L.KCONTIG, L.ROWS_CONV3, seq_len=8, seg=20))
_CONV_MN = dict(M=64, N=64, K=96, A=_op(L.MNCONTIG, L.ROWS_CONV3, ld=64, seq_len=8, seg=20))

STATIC = [
    ("M=-1", dict(M=-1), -1000),
    ("prec=7", dict(prec=7), -1012),
    ("epilogue=11", dict(epilogue=11), -1003),
    ("A=NULL", dict(A=None), -1001),
    ("gathered A, ld=30", dict(A=_op(mapping=L.ROWS_GATHER, ld=30)), -1002),
    ("EPI_SCATTER without c_rows", dict(epilogue=L.EPI_SCATTER), -1004),
    ("EPI_STORE_GELU without aux", dict(epilogue=L.EPI_STORE_GELU), -1004),
    ("EPI_ACCUM_GATE without aux", dict(epilogue=L.EPI_ACCUM_GATE), -1004),
    ("EPI_GELU_GRAD without aux", dict(epilogue=L.EPI_GELU_GRAD), -1004),
    ("EPI_SCATTER_STORE without c_rows", dict(epilogue=L.EPI_SCATTER_STORE), -1004),
    ("split_k=2 with EPI_STORE", dict(split_k=2), -1005),
    ("M=0", dict(M=0), 0),
    ("K-contiguous CONV3 A, seg=20", _CONV_KC, -1006),
    ("MN-contiguous CONV3 A, seg=20", _CONV_MN, -1007),
]

DYN = [
    ("max_cus=-1", dict(), -1, -1015),
    ("K=33", dict(K=33), 0, -1000),
    ("prec=7", dict(prec=7), 0, -1014),
    ("plain A, ld=30", dict(A=_op(ld=30)), 0, -1002),
    ("K=0", dict(K=0), 0, 0),
    ("MN-contiguous gathered A", dict(A=_op(L.MNCONTIG, L.ROWS_GATHER)), 0, -1007),
]


@pytest.mark.parametrize("name,kw,want", STATIC, ids=[c[0] for c in STATIC])
def test_static_form_codes(name, kw, want):
    got = _static_codes(_args(**kw))
    assert got == {k: want for k in got}, name


@pytest.mark.parametrize("name,kw,max_cus,want", DYN, ids=[c[0] for c in DYN])
def test_dynamic_form_codes(name, kw, max_cus, want):
    got = _dyn_codes(_args(**kw), max_cus)
    assert got == {k: want for k in got}, name


def test_workspace_form_codes():
    a = _args()
    folded = ctypes.c_int32(0)
    ws = lambda a, m_dev, max_cus, work, n, colsum, fl: _call(
        "nr_gemm_f32_ws", *_head(a), m_dev, None, a["prec"], max_cus, work, n, colsum, fl, None)
    assert ws(a, None, 0, _BASE, -1, None, None) == -1016            # work_elems < 0
    assert ws(a, None, 0, None, 8, None, None) == -1016              # work_elems > 0 without work
    assert ws(a, None, 0, None, 0, _BASE, None) == -1017             # colsum without colsum_folded
    assert ws(a, None, 3, None, 0, _BASE, None) == -1017             # ... in the dynamic form too
    for m_dev, max_cus in ((None, 0), (None, 3), (ctypes.byref(_MDEV), 0)):
        folded.value = 5
        assert ws(_args(M=0), m_dev, max_cus, None, 0, _BASE, ctypes.byref(folded)) == 0   # M = 0: nothing to do,
        assert folded.value == 0                                     # and the flag is reset on entry
    folded.value = 5
    assert ws(_args(K=33), None, 3, None, 0, None, ctypes.byref(folded)) == -1000          # dynamic form: K % 32
    assert folded.value == 0
    assert ws(_args(K=33), ctypes.byref(_MDEV), 0, None, 0, None, None) == -1000
