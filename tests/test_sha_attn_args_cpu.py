"""Return codes of nr_sha_attn_fwd / nr_sha_attn_bwd (csrc/sha_attn.hip) for invalid and empty arguments,
as include/newsrec_hip.h documents them.  Every argument check and the nseq = 0 case return before any
HIP call, so the entries run through ctypes on a machine without a GPU: the operands sit on a
16-B-aligned HOST buffer that no case ever dereferences (the mechanism of test_birnn_args_cpu.py).
No case passes a complete valid non-empty argument list: that would launch.

-1000 is a bad size, offset, leading dimension, rate, mask type or alignment; -1001 a required pointer
that is NULL."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
BAD, NULL, OK = -1000, -1001, 0
D = 8

FWD = dict(qkv=P, ldq=3 * D, koff=D, voff=2 * D, mask=P, mask_dtype=1, nseq=3, L=5, D=D, scale=0.35, p_drop=0.1,
           seed=1, offset=2, rng=None, ctx=P, ldc=D, probs=P, stream=None)
BWD = dict(qkv=P, ldq=3 * D, koff=D, voff=2 * D, mask=P, mask_dtype=1, nseq=3, L=5, D=D, scale=0.35, p_drop=0.1,
           seed=1, offset=2, rng=None, probs=P, dctx=P, ldd=D, dqkv=P, lddq=3 * D, stream=None)


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


_W = dict(ldq=3 * 1028, koff=1028, voff=2056)
_COMMON_BAD = (
    dict(nseq=-1), dict(nseq=2 ** 31), dict(L=0), dict(L=-1), dict(L=65), dict(D=0), dict(D=-4), dict(D=6),
    dict(D=1028, **_W), dict(koff=D - 4), dict(koff=D + 2, voff=2 * D + 4, ldq=3 * D + 4), dict(voff=2 * D - 4),
    dict(voff=2 * D + 2, ldq=3 * D + 4), dict(koff=-4), dict(ldq=3 * D - 4), dict(ldq=3 * D + 2),
    dict(p_drop=1.0), dict(p_drop=-0.1), dict(p_drop=float("nan")), dict(mask_dtype=4), dict(mask_dtype=-1),
    dict(qkv=P + 4))
FWD_BAD = _COMMON_BAD + (dict(ldc=D - 4), dict(ldc=D + 1), dict(ctx=P + 8))
BWD_BAD = _COMMON_BAD + (dict(ldd=D - 4), dict(ldd=D + 3), dict(lddq=3 * D - 4), dict(lddq=3 * D + 1), dict(dctx=P + 4),
                         dict(dqkv=P + 12))
FWD_NULL = ("qkv", "mask", "probs", "ctx")
BWD_NULL = ("qkv", "mask", "probs", "dctx", "dqkv")
_COMMON_OK = (dict(nseq=0), dict(nseq=0, p_drop=0.0), dict(nseq=0, L=64, D=1024, ldq=3072, koff=1024, voff=2048),
              dict(nseq=0, L=1, D=4), dict(nseq=0, koff=D + 4, voff=2 * D + 12, ldq=3 * D + 16), dict(nseq=0, rng=P),
              dict(nseq=0, mask_dtype=0), dict(nseq=0, mask_dtype=3))
FWD_OK = tuple(dict(kw, ldc=1024) if kw.get("D") == 1024 else kw for kw in _COMMON_OK) + (dict(nseq=0, ldc=D + 4),)
BWD_OK = tuple(dict(kw, ldd=1024, lddq=3072) if kw.get("D") == 1024 else
               dict(kw, lddq=kw["ldq"]) if "ldq" in kw else kw for kw in _COMMON_OK) + (dict(nseq=0, ldd=D + 4),)

CASES = []
for name, base, bad, null, ok in (("nr_sha_attn_fwd", FWD, FWD_BAD, FWD_NULL, FWD_OK),
                                  ("nr_sha_attn_bwd", BWD, BWD_BAD, BWD_NULL, BWD_OK)):
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
    assert _call(name, list(args.values())) == want


def test_sizes_are_checked_before_pointers():
    assert _call("nr_sha_attn_fwd", list(_with(FWD, L=65, qkv=None).values())) == BAD
    assert _call("nr_sha_attn_bwd", list(_with(BWD, D=6, dqkv=None).values())) == BAD


def test_wrapper_checks_raise_before_any_launch():
    """kernels.sha_attn_fwd / sha_attn_bwd refuse a wrong dtype, device, shape or size on the host."""
    import torch
    from newsrec_amd import kernels as K
    t = torch.zeros(15, 24)
    m = torch.ones(15, dtype=torch.int64)
    with pytest.raises(L.HipError):
        K.sha_attn_fwd(t, m, 3, 5, 8, t, t)                 # CPU tensors
    with pytest.raises(L.HipError):
        K.sha_attn_fwd(t, m, 3, 65, 8, t, t)                # L past the kernels' limit
    with pytest.raises(L.HipError):
        K.sha_attn_fwd(t, m, 3, 5, 6, t, t)                 # D % 4
    with pytest.raises(L.HipError):
        K.sha_attn_bwd(t, m, 3, 5, 8, t, t, t, p_drop=1.0)  # p_drop = 1
    with pytest.raises(L.HipError):
        K.sha_attn_bwd(t, m, 3, 5, 8, t, t, t, koff=4)      # k overlaps q
