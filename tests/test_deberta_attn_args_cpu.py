"""Return codes of nr_deb_attn_fwd / nr_deb_attn_bwd / nr_deb_attn_bwd_workspace (csrc/deberta_attn.hip) for
invalid and empty arguments, as include/newsrec_hip.h documents them.  Every argument check and the nseq = 0
case return before any HIP call, so the entries run through ctypes on a machine without a GPU: the operands
sit on a 16-B-aligned HOST buffer that no case ever dereferences (the mechanism of
test_synth_attn_args_cpu.py).  No case passes a complete valid non-empty argument list: that would launch.

-1000 is a bad size, offset, leading dimension, alignment or workspace size; -1001 a required pointer that is
NULL."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
BAD, NULL, OK = -1000, -1001, 0
NSEQ, SL, HEADS = 3, 5, 2
H = 64 * HEADS
WORK = 3 * HEADS * 2 * (2 * SL) * 64 * 4         # min(nseq, 512 / heads) walkers x heads x [2][2L][64] floats

_COMMON = dict(qkv=P, ldq=3 * H, hstride=192, qoff=0, koff=64, voff=128, pk=P, pq=P + 16, ldp=H, mask=P, mask_dtype=1,
               nseq=NSEQ, L=SL, heads=HEADS, scale=0.0721, p_drop=0.1, seed=1, offset=0, rng=None, probs=P + 4)
FWD = dict(_COMMON, ctx=P, ldc=H, stream=None)
BWD = dict(_COMMON, dctx=P, ldd=H, dqkv=P, lddq=3 * H, dpk=P, dpq=P + 32, lddp=H, work=P, work_bytes=WORK, stream=None)
BLOCKED = dict(hstride=64, qoff=0, koff=H, voff=2 * H)


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
    dict(nseq=-1), dict(nseq=2 ** 31), dict(nseq=2 ** 30 + 1), dict(L=0), dict(L=-1), dict(L=65), dict(heads=0),
    dict(heads=-2), dict(heads=1025), dict(heads=3), dict(ldq=3 * H - 4), dict(ldq=3 * H + 2), dict(hstride=190),
    dict(hstride=60), dict(hstride=0), dict(hstride=3 * H + 4), dict(qoff=2), dict(qoff=-4), dict(koff=66),
    dict(koff=-64), dict(voff=130), dict(voff=-4), dict(koff=60), dict(voff=64), dict(voff=124), dict(voff=132),
    dict(ldp=H - 4), dict(ldp=H + 2), dict(p_drop=-0.1), dict(p_drop=1.0), dict(p_drop=float("nan")),
    dict(mask_dtype=-1), dict(mask_dtype=4), dict(qkv=P + 4), dict(pk=P + 8), dict(pq=P + 4), dict(probs=P + 2),
    dict(BLOCKED, koff=H + 2), dict(BLOCKED, voff=2 * H + 4), dict(BLOCKED, ldq=3 * H - 4))
FWD_BAD = _COMMON_BAD + (dict(ldc=H - 4), dict(ldc=H + 1), dict(ctx=P + 8))
BWD_BAD = _COMMON_BAD + (dict(ldd=H - 4), dict(ldd=H + 3), dict(lddq=3 * H - 4), dict(lddq=3 * H + 1),
                         dict(lddp=H - 4), dict(lddp=H + 2), dict(dctx=P + 4), dict(dqkv=P + 12), dict(dpk=P + 4),
                         dict(dpq=P + 8), dict(work=P + 4), dict(work_bytes=WORK - 4), dict(work_bytes=0),
                         dict(work_bytes=-1))
FWD_NULL = ("qkv", "pk", "pq", "mask", "probs", "ctx")
BWD_NULL = ("qkv", "pk", "pq", "mask", "probs", "dctx", "dqkv", "dpk", "dpq")
_COMMON_OK = (dict(nseq=0), dict(nseq=0, L=64), dict(nseq=0, L=1), dict(nseq=0, ldq=3 * H + 8, ldp=H + 4),
              dict(BLOCKED, nseq=0), dict(nseq=0, p_drop=0.0), dict(nseq=0, heads=1), dict(nseq=0, mask_dtype=0),
              dict(nseq=0, heads=12, ldq=2304, ldp=768))
FWD_OK = tuple(dict(kw, ldc=768) if kw.get("heads") == 12 else kw for kw in _COMMON_OK) + (dict(nseq=0, ldc=H + 4),)
BWD_OK = tuple(dict(kw, ldd=768, lddq=2304, lddp=768) if kw.get("heads") == 12 else kw for kw in _COMMON_OK) + \
    (dict(nseq=0, ldd=H + 4, lddq=3 * H + 8, lddp=H + 8), dict(nseq=0, work=None, work_bytes=0))

CASES = []
for name, base, bad, null, ok in (("nr_deb_attn_fwd", FWD, FWD_BAD, FWD_NULL, FWD_OK),
                                  ("nr_deb_attn_bwd", BWD, BWD_BAD, BWD_NULL, BWD_OK)):
    for empty in (False, True):     # the checks come before the empty case: the same codes at nseq = 0
        for kw in bad:
            if empty and ("nseq" in kw or "work_bytes" in kw):     # an empty call needs no workspace
                continue
            full = dict(kw, nseq=0) if empty else kw
            CASES.append((name, _label(full), _with(base, **full), BAD))
        for n in null:
            full = {n: None, "nseq": 0} if empty else {n: None}
            CASES.append((name, _label(full), _with(base, **full), NULL))
    for kw in ok:
        CASES.append((name, _label(kw) + " -> OK", _with(base, **kw), OK))
CASES.append(("nr_deb_attn_bwd", "work=None", _with(BWD, work=None), NULL))


@pytest.mark.parametrize("name,cid,args,want", CASES, ids=["%s: %s" % (c[0], c[1]) for c in CASES])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    assert want != OK or args["nseq"] == 0, "a valid non-empty call would launch"
    assert _call(name, list(args.values())) == want


def test_sizes_are_checked_before_pointers():
    assert _call("nr_deb_attn_fwd", list(_with(FWD, L=65, qkv=None).values())) == BAD
    assert _call("nr_deb_attn_fwd", list(_with(FWD, ldc=H + 1, ctx=None).values())) == BAD
    assert _call("nr_deb_attn_bwd", list(_with(BWD, heads=0, dqkv=None).values())) == BAD
    assert _call("nr_deb_attn_bwd", list(_with(BWD, lddp=H - 4, dpk=None).values())) == BAD
    assert _call("nr_deb_attn_bwd", list(_with(BWD, work_bytes=WORK - 4, work=None).values())) == BAD


@pytest.mark.parametrize("nseq,seq_len,heads,want", [
    (3, 5, 2, WORK), (0, 5, 2, 0), (1, 1, 1, 1024), (300, 5, 2, 256 * 2 * 2 * 10 * 64 * 4),
    (42, 30, 12, 42 * 12 * 2 * 60 * 64 * 4), (1760, 30, 12, 42 * 12 * 2 * 60 * 64 * 4),
    (513, 64, 1, 512 * 2 * 128 * 64 * 4), (5, 3, 1024, 1 * 1024 * 2 * 6 * 64 * 4),
    (-1, 5, 2, BAD), (3, 0, 2, BAD), (3, 65, 2, BAD), (3, 5, 0, BAD), (3, 5, 1025, BAD), (2 ** 31, 5, 1, BAD),
    (2 ** 30, 5, 2, BAD)])
def test_workspace_query(nseq, seq_len, heads, want):
    assert L.load().nr_deb_attn_bwd_workspace(nseq, seq_len, heads) == want


def test_wrapper_checks_raise_before_any_launch():
    """kernels.deb_attn_fwd / deb_attn_bwd refuse a wrong dtype, device, shape, layout or size on the host."""
    import torch
    from newsrec_amd import kernels as K
    T = NSEQ * SL
    qkv, pk, ctx = torch.zeros(T, 3 * H), torch.zeros(2 * SL, H), torch.zeros(T, H)
    mask, pr = torch.ones(NSEQ, SL, dtype=torch.int64), torch.zeros(NSEQ * HEADS * SL * SL)
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, SL, HEADS, pr, ctx)                          # CPU tensors
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, 65, HEADS, pr, ctx)                          # L past the limit
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, -1, SL, HEADS, pr, ctx)                            # nseq < 0
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, SL, 0, pr, ctx)                              # no head
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, SL, HEADS, pr, ctx, layout=(192, 0, 32, 128))   # q and k overlap
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, SL, HEADS, pr, ctx, layout=(190, 0, 64, 128))   # hstride % 4
    with pytest.raises(L.HipError):
        K.deb_attn_fwd(qkv, pk, pk, mask, NSEQ, SL, HEADS, pr, ctx, p_drop=1.0)
    with pytest.raises(L.HipError):
        K.deb_attn_bwd(qkv.double(), pk, pk, mask, NSEQ, SL, HEADS, pr, ctx, qkv, pk, pk)    # float64
    with pytest.raises(L.HipError):
        K.deb_attn_bwd(qkv, pk, pk, mask, NSEQ, SL, HEADS, pr, ctx, qkv, pk, pk, layout=K.deb_blocked(3))   # too wide
    assert K.deb_blocked(12) == (64, 0, 768, 1536) and K.DEB_INTERLEAVED == (192, 0, 64, 128)
