"""Return codes of nr_mha_attn_fwd / nr_mha_attn_bwd (csrc/mha_attn.hip) and nr_mha_user_pool_fwd
(csrc/mha_pool.hip) for invalid and empty arguments, as include/newsrec_hip.h documents them.  Every
argument check, the (dk, dv) table lookup and the nseq = 0 case return before any HIP call, so the entries
run through ctypes on a machine without a GPU: the operands sit on a 16-B-aligned HOST buffer that no case
ever dereferences (the mechanism of test_sha_attn_args_cpu.py).  No case passes a complete valid
non-empty argument list: that would launch.

-1000 a bad size (L, heads, nseq, mask type); -1001 a required pointer that is NULL; -1002 a leading
dimension that is no multiple of 4 or narrower than its row, or a pointer off 16 B; -1003 one of dbias_k /
dbias_v without the other (the user pool: ldo narrower than heads*dv); -1008 a (dk, dv) without an
instantiation; the user pool also -1004 (prec), -1005 (y_rows), -1009 (heads*dv % 64), -1010 (LDS)."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
OK, SIZE, NULL, LD, PAIR, PREC, YROWS, GEOM, H64, LDS = 0, -1000, -1001, -1002, -1003, -1004, -1005, -1008, -1009, -1010
HEADS, DK, DV = 2, 64, 32
NQ, NV = HEADS * DK, HEADS * DV

FWD = dict(qk=P, ld_qk=NQ + 4, v=P, ld_v=NV + 4, rows=None, mask=P, mask_dtype=1, nseq=3, L=5, heads=HEADS, dk=DK,
           dv=DV, scale=0.125, out=P, ld_out=NV + 4, stream=None)
BWD = dict(qk=P, ld_qk=NQ + 4, v=P, ld_v=NV + 4, mask=P, mask_dtype=1, nseq=3, L=5, heads=HEADS, dk=DK, dv=DV,
           scale=0.125, dout=P, ld_dout=NV + 4, dqk=P, ld_dqk=NQ + 4, dvout=P, ld_dv=NV + 4, dbias_k=None,
           dbias_v=None, stream=None)
UH, UK, UV = 12, 32, 32
UPOOL = dict(y=P, ldy=UH * (UK + UV) + 4, y_rows=100, yrows=P, mask=P, mask_dtype=2, nseq=3, L=50, heads=UH, dk=UK,
             dv=UV, q=P, out=P, ldo=UH * UV, prec=0, stream=None)

# (LMAX, dk, dv) of every instantiation of mha_attn.hip's dispatch()
TABLE = ((32, 64, 32), (32, 32, 32), (32, 64, 64), (32, 64, 16), (32, 16, 16),
         (64, 32, 32), (64, 64, 64), (64, 16, 16), (64, 64, 32))


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


def _lds(base, dk, dv, heads=HEADS):
    """Every leading dimension of ``base`` exactly its row at (heads, dk, dv)."""
    nq, nv = heads * dk, heads * dv
    return {k: nq if k in ("ld_qk", "ld_dqk") else nv for k in base if k.startswith("ld_")}


# (L, dk, dv) without an instantiation: (64, 16) exists for L <= 32 only
_NO_GEOM = ((5, 48, 32), (5, 16, 32), (33, 64, 16), (64, 64, 16), (5, 32, 64), (5, 0, 0), (5, -64, -32), (5, 128, 128))
_SIZES = (dict(nseq=-1), dict(nseq=2 ** 31), dict(nseq=2 ** 40), dict(L=0), dict(L=-1), dict(L=65), dict(heads=0),
          dict(heads=-2), dict(heads=65536), dict(mask_dtype=4), dict(mask_dtype=-1))
# each case: (arguments changed, code); every one is also run at nseq = 0, where it reports the same code
FWD_CASES = [(kw, SIZE) for kw in _SIZES] + [({k: None}, NULL) for k in ("qk", "v", "mask", "out")] + [
    (kw, LD) for kw in (dict(ld_qk=NQ + 2), dict(ld_v=NV + 1), dict(ld_out=NV + 3), dict(qk=P + 4), dict(v=P + 8),
                        dict(out=P + 12), dict(ld_qk=NQ - 4), dict(ld_v=NV - 4), dict(ld_out=NV - 4), dict(ld_qk=0),
                        dict(ld_out=-4), dict(heads=3))     # heads = 3: every row is wider than its ld
] + [(dict(L=l, dk=dk, dv=dv, **_lds(FWD, dk, dv)), GEOM) for l, dk, dv in _NO_GEOM]
BWD_CASES = [(kw, SIZE) for kw in _SIZES] + [({k: None}, NULL) for k in ("qk", "v", "mask", "dout", "dqk", "dvout")] + [
    (kw, LD) for kw in (dict(ld_qk=NQ + 2), dict(ld_v=NV + 1), dict(ld_dout=NV + 3), dict(ld_dqk=NQ + 2),
                        dict(ld_dv=NV + 6), dict(qk=P + 4), dict(v=P + 8), dict(dout=P + 4), dict(dqk=P + 12),
                        dict(dvout=P + 8), dict(ld_qk=NQ - 4), dict(ld_v=NV - 4), dict(ld_dout=NV - 4),
                        dict(ld_dqk=NQ - 4), dict(ld_dv=NV - 4), dict(ld_dv=0), dict(heads=3))
] + [(kw, PAIR) for kw in (dict(dbias_k=P), dict(dbias_v=P), dict(dbias_k=P, dk=48), dict(dbias_v=P, dk=16, dv=32))
] + [(dict(L=l, dk=dk, dv=dv, **_lds(BWD, dk, dv)), GEOM) for l, dk, dv in _NO_GEOM
] + [(dict(dk=32, dv=64, dbias_k=P, dbias_v=P, **_lds(BWD, 32, 64)), GEOM)]
_UW = dict(dk=64, dv=64, ldy=12 * 128, ldo=768)
UPOOL_CASES = [(kw, SIZE) for kw in (dict(nseq=-1), dict(nseq=2 ** 31), dict(L=0), dict(L=65), dict(heads=0),
                                     dict(heads=13), dict(mask_dtype=4), dict(mask_dtype=-1))] + [
    (kw, YROWS) for kw in (dict(y_rows=0), dict(y_rows=-1), dict(y_rows=2 ** 30 // 772 + 1), dict(y_rows=2 ** 31))
] + [(kw, PREC) for kw in (dict(prec=3), dict(prec=-1))] + [({k: None}, NULL) for k in ("y", "mask", "q", "out")] + [
    (kw, LD) for kw in (dict(ldy=770), dict(y=P + 4), dict(ldy=764), dict(dk=64, dv=32))
] + [(kw, PAIR) for kw in (dict(ldo=380), dict(ldo=0), dict(dk=64, dv=64, ldy=12 * 128))
] + [(kw, H64) for kw in (dict(dv=24), dict(heads=5))
] + [(kw, LDS) for kw in (dict(L=54, **_UW), dict(L=64, **_UW))
] + [(kw, GEOM) for kw in (dict(dk=48, ldy=960), dict(heads=8, dk=64, dv=32), dict(dk=16, dv=32), dict(heads=6, dk=64, dv=64))]

CASES = []
for name, base, cases in (("nr_mha_attn_fwd", FWD, FWD_CASES), ("nr_mha_attn_bwd", BWD, BWD_CASES),
                          ("nr_mha_user_pool_fwd", UPOOL, UPOOL_CASES)):
    for kw, code in cases:
        CASES.append((name, _label(kw), _with(base, **kw), code))
        if "nseq" not in kw:     # the checks come before the empty case: the same code at nseq = 0
            CASES.append((name, _label(dict(kw, nseq=0)), _with(base, **dict(kw, nseq=0)), code))
# the largest nseq and heads pass the size check (and fail a later one: nothing may launch)
for name, base in (("nr_mha_attn_fwd", FWD), ("nr_mha_attn_bwd", BWD)):
    for kw in (dict(nseq=2 ** 31 - 1, dk=48), dict(heads=65535, dk=48, dv=32, **_lds(base, 48, 32, 65535))):
        CASES.append((name, _label(kw), _with(base, **kw), GEOM))
    # the empty batch
    for lmax, dk, dv in TABLE:
        kw = dict(nseq=0, L=lmax - 7, dk=dk, dv=dv, **_lds(base, dk, dv))
        CASES.append((name, _label(kw) + " -> OK", _with(base, **kw), OK))
    for kw in (dict(nseq=0, mask_dtype=0), dict(nseq=0, mask_dtype=3), dict(nseq=0, L=1), dict(nseq=0, L=64, dv=64, **_lds(base, 64, 64)),
               dict(nseq=0, L=32), dict(nseq=0, L=33, dk=32), dict(nseq=0, heads=65535, dk=16, dv=16, **_lds(base, 16, 16, 65535))):
        CASES.append((name, _label(kw) + " -> OK", _with(base, **kw), OK))
CASES.append(("nr_mha_attn_fwd", "nseq=0, rows=P -> OK", _with(FWD, nseq=0, rows=P), OK))
CASES.append(("nr_mha_attn_bwd", "nseq=0, dbias_k=P, dbias_v=P+16 -> OK", _with(BWD, nseq=0, dbias_k=P, dbias_v=P + 16), OK))
for kw in (dict(nseq=0), dict(nseq=0, yrows=None), dict(nseq=0, dk=64, ldy=12 * 96), dict(nseq=0, L=53, **_UW),
           dict(nseq=0, L=1, mask_dtype=0, prec=2), dict(nseq=0, L=64, prec=1, ldo=388), dict(nseq=0, y_rows=1)):
    CASES.append(("nr_mha_user_pool_fwd", _label(kw) + " -> OK", _with(UPOOL, **kw), OK))


@pytest.mark.parametrize("name,cid,args,want", CASES, ids=["%s: %s" % (c[0], c[1]) for c in CASES])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    if args["nseq"] != 0:
        assert want != OK, "a valid non-empty call would launch"
    assert _call(name, list(args.values())) == want


def test_order_of_the_checks():
    """Sizes before pointers, pointers before leading dimensions, those before the dbias pair, the pair
    before the (dk, dv) table."""
    assert _call("nr_mha_attn_fwd", list(_with(FWD, L=65, qk=None).values())) == SIZE
    assert _call("nr_mha_attn_fwd", list(_with(FWD, mask_dtype=7, out=None, ld_out=3).values())) == SIZE
    assert _call("nr_mha_attn_bwd", list(_with(BWD, nseq=-1, dqk=None).values())) == SIZE
    assert _call("nr_mha_attn_fwd", list(_with(FWD, v=None, ld_v=NV - 4).values())) == NULL
    assert _call("nr_mha_attn_bwd", list(_with(BWD, dout=None, ld_dout=3, dbias_k=P).values())) == NULL
    assert _call("nr_mha_attn_fwd", list(_with(FWD, ld_out=NV - 4, dk=48).values())) == LD
    assert _call("nr_mha_attn_bwd", list(_with(BWD, ld_dv=NV - 4, dbias_k=P).values())) == LD
    assert _call("nr_mha_attn_bwd", list(_with(BWD, dbias_v=P, dk=16, dv=16).values())) == PAIR
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, heads=13, y=None).values())) == SIZE
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, nseq=-1, y_rows=0).values())) == SIZE
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, y_rows=0, prec=9, y=None).values())) == YROWS
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, prec=9, y=None).values())) == PREC
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, q=None, ldy=770).values())) == NULL
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, ldy=764, ldo=380).values())) == LD
    assert _call("nr_mha_user_pool_fwd", list(_with(UPOOL, ldo=280, dv=24).values())) == PAIR


def test_wrappers_refuse_cpu_tensors():
    """kernels.mha_attn_fwd / mha_attn_bwd / mha_user_pool_fwd refuse host tensors before any call (their
    other checks need device tensors: tests/test_mha_attn_kernels_gpu.py)."""
    import torch
    from newsrec_amd import kernels as K
    qk, v, o = torch.zeros(15, NQ), torch.zeros(15, NV), torch.zeros(15, NV)
    m = torch.ones(3, 5, dtype=torch.int64)
    with pytest.raises(L.HipError, match="float32 CUDA tensor"):
        K.mha_attn_fwd(qk, v, m, 3, 5, HEADS, DK, DV, o)
    with pytest.raises(L.HipError, match="float32 CUDA tensor"):
        K.mha_attn_bwd(qk, v, m, 3, 5, HEADS, DK, DV, o, torch.zeros(15, NQ), torch.zeros(15, NV))
    with pytest.raises(L.HipError, match="float32 CUDA tensor"):
        K.mha_user_pool_fwd(torch.zeros(15, 768), torch.zeros(15, dtype=torch.int64), m, 3, 5, 12, 32, 32,
                            torch.zeros(384), torch.zeros(3, 384))
