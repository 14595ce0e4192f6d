"""Return codes of nr_birnn_fwd / nr_birnn_bwd (csrc/birnn.hip) for invalid and empty arguments, as
include/newsrec_hip.h documents them.  Every argument check and the nseq = 0 case return before any
HIP call, so the entries run through ctypes on a machine without a GPU: the operands sit on a
16-B-aligned HOST buffer that no case ever dereferences (the mechanism of test_score_args_cpu.py).
No case passes a complete valid non-empty argument list: that would launch.

-1000 is a bad size, -1001 a required pointer that is NULL."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
BAD, NULL, OK = -1000, -1001, 0
H = 8

FWD = dict(gx=P, ldgx=8 * H, whh_fwd=P, bhh=P, nseq=3, L=5, H=H, gates=P, hprev=P, ldh=H, hlast=P, news=P, ldn=H,
           tok=P, ldt=H, stream=None)
BWD = dict(whh_bwd=P, gates=P, nseq=3, L=5, H=H, dnews=P, lddn=H, dtok=P, lddt=H, dg=P, lddg=8 * H, stream=None)


def _call(name, args):
    return getattr(L.load(), name)(*args)


def _with(base, **kw):
    a = dict(base)
    for k in kw:
        assert k in a, k
    a.update(kw)
    return a


def _label(kw):
    return ", ".join("%s=%s" % (k, "P" if v is P else v) for k, v in kw.items())


_SIZES = (dict(nseq=-1), dict(L=0), dict(L=-2), dict(H=0), dict(H=-1), dict(H=257, ldgx=8 * 257, ldh=257, ldn=257, ldt=257))
FWD_BAD = _SIZES + (dict(ldgx=8 * H - 1), dict(ldh=H - 1), dict(ldn=H - 1), dict(ldt=H - 1))
FWD_NULL = ("gx", "whh_fwd", "gates", "hprev", "hlast", "news")
FWD_OK = (dict(nseq=0), dict(nseq=0, tok=None, ldt=0), dict(nseq=0, bhh=None), dict(nseq=0, H=256, ldgx=2048, ldh=256, ldn=256, ldt=256))
BWD_BAD = (dict(nseq=-1), dict(L=0), dict(H=0), dict(H=257, lddg=8 * 257, lddn=257, lddt=257), dict(lddg=8 * H - 1),
           dict(lddn=H - 1), dict(lddt=H - 1))
BWD_NULL = ("whh_bwd", "gates", "dg")
BWD_OK = (dict(nseq=0), dict(nseq=0, dnews=None, lddn=0), dict(nseq=0, dtok=None, lddt=0))

CASES = []
for name, base, bad, null, ok in (("nr_birnn_fwd", FWD, FWD_BAD, FWD_NULL, FWD_OK),
                                  ("nr_birnn_bwd", BWD, BWD_BAD, BWD_NULL, BWD_OK)):
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
CASES.append(("nr_birnn_bwd", "dnews=None, dtok=None", _with(BWD, dnews=None, dtok=None), NULL))
CASES.append(("nr_birnn_bwd", "dnews=None, dtok=None, nseq=0", _with(BWD, dnews=None, dtok=None, nseq=0), NULL))


@pytest.mark.parametrize("name,cid,args,want", CASES, ids=["%s: %s" % (c[0], c[1]) for c in CASES])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    assert _call(name, list(args.values())) == want


def test_sizes_are_checked_before_pointers():
    assert _call("nr_birnn_fwd", list(_with(FWD, H=257, gx=None).values())) == BAD
    assert _call("nr_birnn_bwd", list(_with(BWD, L=0, dg=None).values())) == BAD
    # an ld of a tensor that is not given is not looked at
    assert _call("nr_birnn_fwd", list(_with(FWD, nseq=0, tok=None, ldt=-5).values())) == OK
    assert _call("nr_birnn_bwd", list(_with(BWD, nseq=0, dnews=None, lddn=-5).values())) == OK


def test_wrapper_checks_raise_before_any_launch():
    """kernels.birnn_fwd / birnn_bwd refuse a wrong dtype, device or shape on the host."""
    import torch
    from newsrec_amd import kernels as K
    t = torch.zeros(15, 64)
    with pytest.raises(L.HipError):
        K.birnn_fwd(t, t, None, 3, 5, 8, t, t, t, t)            # CPU tensors
    with pytest.raises(L.HipError):
        K.birnn_fwd(t, t, None, 3, 5, 257, t, t, t, t)          # H past the kernels' limit
    with pytest.raises(L.HipError):
        K.birnn_bwd(t, t, 3, 0, 8, t, dnews=t)                  # L < 1
    assert K.birnn_gates_numel(17, 2, 150) == 2 * 2 * 2 * 38 * 320
