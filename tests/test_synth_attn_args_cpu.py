"""Return codes of nr_synth_attn_fwd / nr_synth_attn_bwd (csrc/synth_attn.hip) for invalid and empty
arguments, as include/newsrec_hip.h documents them.  Every argument check and the nseq = 0 case return before
any HIP call, so the entries run through ctypes on a machine without a GPU: the operands sit on a 16-B-aligned
HOST buffer that no case ever dereferences (the mechanism of test_sha_attn_args_cpu.py).  No case passes a
complete valid non-empty argument list: that would launch.

-1000 is a bad size, leading dimension or alignment; -1001 a required pointer that is NULL."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
BAD, NULL, OK = -1000, -1001, 0
D, SL = 8, 5

FWD = dict(hv=P, ldh=D, w1=P, ldw1=D, b1=P + 4, w2=P + 8, b2=P + 12, nseq=3, L=SL, D=D, a1=P + 4, lda=SL, probs=P + 8,
           ctx=P, ldc=D, stream=None)
BWD = dict(hv=P, ldh=D, w1=P, ldw1=D, w2=P + 4, a1=P + 8, lda=SL, probs=P + 12, dctx=P, ldd=D, nseq=3, L=SL, D=D,
           da1=P + 4, da2=P + 8, dhv=P, lddh=D, stream=None)


def _call(name, args):
    return getattr(L.load(), name)(*args)


def _with(base, **kw):
    a = dict(base)
    for k in kw:
        assert k in a, k
    a.update(kw)
    return a


def _show(v):
    # a pointer into the buffer as "P" / "P+4": the address itself differs from run to run, and a test id
    # must not
    if isinstance(v, int) and not isinstance(v, bool) and 0 <= v - P < 4096:
        return "P" if v == P else "P+%d" % (v - P)
    return v


def _label(kw):
    return ", ".join("%s=%s" % (k, _show(v)) for k, v in kw.items())


_COMMON_BAD = (
    dict(nseq=-1), dict(nseq=2 ** 31), dict(L=0), dict(L=-1), dict(L=65, lda=68), dict(D=0), dict(D=-4), dict(D=6),
    dict(D=1028, ldh=1028, ldw1=1028), dict(ldh=D - 4), dict(ldh=D + 2), dict(ldw1=D - 4), dict(ldw1=D + 1),
    dict(lda=SL - 1), dict(lda=0), dict(hv=P + 4), dict(w1=P + 8), dict(w2=P + 2), dict(a1=P + 1), dict(probs=P + 3))
FWD_BAD = _COMMON_BAD + (dict(D=1028, ldh=1028, ldw1=1028, ldc=1028), dict(ldc=D - 4), dict(ldc=D + 1), dict(ctx=P + 8),
                         dict(b1=P + 2), dict(b2=P + 1))
BWD_BAD = _COMMON_BAD + (dict(D=1028, ldh=1028, ldw1=1028, ldd=1028, lddh=1028), dict(ldd=D - 4), dict(ldd=D + 3),
                         dict(lddh=D - 4), dict(lddh=D + 1), dict(dctx=P + 4), dict(dhv=P + 12), dict(da1=P + 2),
                         dict(da2=P + 3))
FWD_NULL = ("hv", "w1", "b1", "w2", "b2", "a1", "probs", "ctx")
BWD_NULL = ("hv", "w1", "w2", "a1", "probs", "dctx", "da1", "da2", "dhv")
_COMMON_OK = (dict(nseq=0), dict(nseq=0, L=64, lda=64, D=1024, ldh=1024, ldw1=1024), dict(nseq=0, L=1, lda=1, D=4),
              dict(nseq=0, lda=SL + 3), dict(nseq=0, ldh=D + 4, ldw1=D + 8), dict(nseq=0, L=30, lda=30),
              dict(nseq=0, L=30, lda=32))
FWD_OK = tuple(dict(kw, ldc=1024) if kw.get("D") == 1024 else kw for kw in _COMMON_OK) + (dict(nseq=0, ldc=D + 4),)
BWD_OK = tuple(dict(kw, ldd=1024, lddh=1024) if kw.get("D") == 1024 else kw for kw in _COMMON_OK) + \
    (dict(nseq=0, ldd=D + 4, lddh=D + 8),)

CASES = []
for name, base, bad, null, ok in (("nr_synth_attn_fwd", FWD, FWD_BAD, FWD_NULL, FWD_OK),
                                  ("nr_synth_attn_bwd", BWD, BWD_BAD, BWD_NULL, BWD_OK)):
    for empty in (False, True):     # the checks come before the empty case: the same codes at nseq = 0
        for kw in bad:
            if empty and "nseq" in kw:
                continue
            full = dict(kw, nseq=0) if empty else kw
            CASES.append((name, _label(full), _with(base, **full), BAD))
        for n in null:
            full = {n: None, "nseq": 0} if empty else {n: None}
            CASES.append((name, _label(full), _with(base, **full), NULL))
    for kw in ok:
        CASES.append((name, _label(kw) + " -> OK", _with(base, **kw), OK))


@pytest.mark.parametrize("name,cid,args,want", CASES, ids=["%s: %s" % (c[0], c[1]) for c in CASES])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    assert want != OK or args["nseq"] == 0, "a valid non-empty call would launch"
    assert _call(name, list(args.values())) == want


def test_sizes_are_checked_before_pointers():
    assert _call("nr_synth_attn_fwd", list(_with(FWD, L=65, lda=68, hv=None).values())) == BAD
    assert _call("nr_synth_attn_bwd", list(_with(BWD, D=6, dhv=None).values())) == BAD
    assert _call("nr_synth_attn_fwd", list(_with(FWD, ldc=D + 1, ctx=None).values())) == BAD
    assert _call("nr_synth_attn_bwd", list(_with(BWD, lda=SL - 1, da1=None).values())) == BAD


def test_wrapper_checks_raise_before_any_launch():
    """kernels.synth_attn_fwd / synth_attn_bwd refuse a wrong dtype, device, shape or size on the host."""
    import torch
    from newsrec_amd import kernels as K
    t = torch.zeros(15, 8)
    w1, b, w2 = torch.zeros(5, 8), torch.zeros(5), torch.zeros(5, 5)
    a1, pr = torch.zeros(15, 5), torch.zeros(75)
    with pytest.raises(L.HipError):
        K.synth_attn_fwd(t, w1, b, w2, b, 3, 5, 8, a1, pr, t)                    # CPU tensors
    with pytest.raises(L.HipError):
        K.synth_attn_fwd(t, w1, b, w2, b, 3, 65, 8, a1, pr, t)                   # L past the kernels' limit
    with pytest.raises(L.HipError):
        K.synth_attn_fwd(t, w1, b, w2, b, 3, 5, 6, a1, pr, t)                    # D % 4
    with pytest.raises(L.HipError):
        K.synth_attn_fwd(t, w1, b, w2, b, -1, 5, 8, a1, pr, t)                   # nseq < 0
    with pytest.raises(L.HipError):
        K.synth_attn_bwd(t, w1, w2, a1, pr, t, 3, 5, 1028, a1, a1, t)            # D past the kernels' limit
    with pytest.raises(L.HipError):
        K.synth_attn_bwd(t.double(), w1, w2, a1, pr, t, 3, 5, 8, a1, a1, t)      # float64
