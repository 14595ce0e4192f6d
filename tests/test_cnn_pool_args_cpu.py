"""Return codes of nr_cnn_keypool_fwd / nr_cnn_keypool_bwd / nr_cnn_keypool_workspace (csrc/cnn_keypool.hip)
and nr_seq_pool_fwd / nr_seq_pool_bwd (csrc/seq_pool.hip) for invalid and empty arguments, as
include/newsrec_hip.h documents them.  Every check covered here returns before any HIP call, so the entries
run through ctypes on a machine without a GPU: the operands sit on a 16-B-aligned HOST buffer that no case
ever dereferences (the mechanism of test_sha_attn_args_cpu.py and test_birnn_args_cpu.py).  No case passes a
complete valid non-empty argument list: that would launch.

-1000 is a bad size or leading dimension (for nr_seq_pool_*, also a misaligned x or key: its shape check
holds them); -1001 a required pointer that is NULL; -1002 a misaligned pointer; -1003 (forward) a bad K
output; -1004 (backward) a K input narrower than Hp.  The checks come in that order, and all of them before
the empty case.  nseq = 0 returns 0 before a launch from both seq_pool entries and from the keypool forward.
The keypool backward has no such return (it launches and stores zero gradients), and its workspace-size
check (-1003) and every valid call of nr_cnn_keypool_workspace ask the device for its CU count first: those
are in tests/test_cnn_pool_kernels_gpu.py."""
import ctypes
import os

import pytest

from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # 16-B aligned host "device" memory (never read)
BAD, NULL, ALIGN, KOUT, KIN, OK = -1000, -1001, -1002, -1003, -1004, 0
HP, H = 64, 40
D = 6                                            # round4(D) = 8

KP_FWD = dict(C=P, ldc=HP, wq=P, bq=P, q=P, qn=H, mask=P, mask_dtype=1, nseq=3, L=5, Hp=HP, scale=0.2, prec=1,
              news=P, ldn=HP, probs=P, kout=None, ldk=0, stream=None)
KP_BWD = dict(C=P, ldc=HP, wq=P, bq=P, q=P, qn=H, nseq=3, L=5, Hp=HP, H=H, scale=0.2, prec=1, probs=P, dnews=P,
              lddn=H, dz=None, lddz=0, dc=P, lddc=HP, dwq=P, dbq=P, dq=P, dconv_b=P, ws=P, ws_floats=1 << 40,
              kin=None, ldk=0, stream=None)
SP_FWD = dict(x=P, ldx=8, key=None, ldk=0, q=P, qn=D, mask=P, mask_dtype=1, nseq=3, L=5, D=D, scale=0.4, out=P,
              ldo=8, probs=P, stream=None)
SP_BWD = dict(x=P, ldx=8, key=None, ldk=0, q=P, qn=D, mask=P, mask_dtype=1, nseq=3, L=5, D=D, scale=0.4, probs=P,
              dout=P, lddo=D, dz=None, lddz=0, dx=P, lddx=8, dk=None, lddk=0, key_tanh=0, dq=P, stream=None)
BASE = {"nr_cnn_keypool_fwd": KP_FWD, "nr_cnn_keypool_bwd": KP_BWD, "nr_seq_pool_fwd": SP_FWD,
        "nr_seq_pool_bwd": SP_BWD}


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


# ---- nr_cnn_keypool_*: (arguments changed, code)
_KP_SHAPE = (dict(Hp=48), dict(Hp=0), dict(Hp=16), dict(Hp=-32), dict(Hp=192, ldc=192), dict(L=0), dict(L=33),
             dict(L=-1), dict(qn=0), dict(qn=HP + 1), dict(nseq=-1), dict(ldc=HP - 4), dict(ldc=HP + 2),
             dict(ldc=HP + 1))
KP_FWD_CASES = [(kw, BAD) for kw in _KP_SHAPE + (dict(ldn=HP - 1), dict(Hp=192, ldc=192, ldn=192))]
KP_FWD_CASES += [({n: None}, NULL) for n in ("C", "wq", "bq", "q", "mask", "news", "probs")]
KP_FWD_CASES += [(kw, ALIGN) for kw in (dict(C=P + 4), dict(C=P + 8), dict(wq=P + 4), dict(wq=P + 12))]
KP_FWD_CASES += [(kw, KOUT) for kw in (dict(kout=P, ldk=HP - 4), dict(kout=P, ldk=0), dict(kout=P, ldk=HP + 2),
                                       dict(kout=P + 4, ldk=HP), dict(kout=P + 8, ldk=HP + 4),
                                       dict(kout=P, L=32, ldk=1 << 24),            # L * ldk * 4 = 2^31
                                       dict(kout=P, L=5, ldk=(1 << 29) // 5 // 4 * 4 + 4))]
KP_BWD_CASES = [(kw, BAD) for kw in _KP_SHAPE + (dict(H=0), dict(H=HP + 1), dict(H=-1), dict(lddn=H - 1), dict(lddn=0),
                                                 dict(lddc=HP - 1), dict(dz=P, lddz=H - 1), dict(dz=P, lddz=0))]
KP_BWD_CASES += [({n: None}, NULL) for n in ("C", "wq", "bq", "q", "probs", "dnews", "dc", "dwq", "dbq", "dq",
                                             "dconv_b", "ws")]
KP_BWD_CASES += [(kw, ALIGN) for kw in (dict(C=P + 4), dict(wq=P + 8))]
KP_BWD_CASES += [(kw, KIN) for kw in (dict(kin=P, ldk=HP - 1), dict(kin=P, ldk=0), dict(kin=P + 4, ldk=HP - 4))]
# the order of the checks: a bad size hides a NULL pointer, which hides a misaligned one, which hides a bad K
KP_FWD_CASES += [(dict(L=33, C=None), BAD), (dict(C=None, wq=P + 4), NULL), (dict(wq=P + 4, kout=P, ldk=0), ALIGN)]
KP_BWD_CASES += [(dict(L=33, dc=None), BAD), (dict(ws=None, C=P + 4), NULL), (dict(C=P + 4, kin=P, ldk=0), ALIGN),
                 (dict(kin=P, ldk=0, ws_floats=0), KIN)]
KP_FWD_OK = (dict(nseq=0), dict(nseq=0, kout=P, ldk=HP + 4), dict(nseq=0, L=1, Hp=32, qn=1, ldc=36, ldn=33),
             dict(nseq=0, L=32, Hp=160, qn=160, ldc=160, ldn=161), dict(nseq=0, mask_dtype=0), dict(nseq=0, prec=0),
             dict(nseq=0, kout=P, L=32, ldk=(1 << 24) - 4))

# ---- nr_seq_pool_*
_SP_SHAPE = (dict(L=0), dict(L=65), dict(L=-1), dict(D=0), dict(D=-4), dict(D=1025, ldx=1028), dict(qn=0),
             dict(qn=D + 1), dict(qn=8), dict(ldx=4), dict(ldx=D), dict(ldx=10), dict(nseq=-1), dict(x=P + 4),
             dict(x=P + 8), dict(key=P, ldk=4), dict(key=P, ldk=D), dict(key=P, ldk=0), dict(key=P, ldk=9),
             dict(key=P + 4, ldk=8))
_KEY = dict(key=P, ldk=8, dk=P, lddk=8)
SP_FWD_CASES = [(kw, BAD) for kw in _SP_SHAPE + (dict(ldo=4), dict(ldo=D), dict(ldo=9), dict(D=1025, ldx=1028, ldo=1028))]
SP_FWD_CASES += [({n: None}, NULL) for n in ("x", "q", "mask", "out", "probs")]
SP_FWD_CASES += [(kw, ALIGN) for kw in (dict(out=P + 4), dict(out=P + 8))]
SP_FWD_CASES += [(dict(L=65, out=None), BAD), (dict(q=None, out=P + 4), NULL)]
SP_BWD_CASES = [(kw, BAD) for kw in _SP_SHAPE + (dict(lddo=D - 1), dict(lddo=0), dict(lddx=4), dict(lddx=D),
                                                 dict(lddx=10), dict(dz=P, lddz=4), dict(dz=P, lddz=D),
                                                 dict(dz=P, lddz=0), dict(dz=P, lddz=9), dict(_KEY, lddk=4),
                                                 dict(_KEY, lddk=D), dict(_KEY, lddk=0), dict(_KEY, lddk=11),
                                                 dict(_KEY, ldk=4), dict(_KEY, key=P + 8))]
SP_BWD_CASES += [({n: None}, NULL) for n in ("x", "q", "mask", "probs", "dout", "dx", "dq")]
SP_BWD_CASES += [(dict(key=P, ldk=8, lddk=8), NULL), (dict(_KEY, dk=None), NULL)]           # a key without dk
SP_BWD_CASES += [(kw, ALIGN) for kw in (dict(dx=P + 4), dict(dz=P + 4, lddz=8), dict(dz=P + 8, lddz=8),
                                        dict(_KEY, dk=P + 4), dict(dk=P + 12, lddk=8))]
SP_BWD_CASES += [(dict(D=0, dx=None), BAD), (dict(dq=None, dx=P + 4), NULL)]
_SP_OK = (dict(nseq=0), dict(nseq=0, L=1, D=1, qn=1, ldx=4), dict(nseq=0, L=64, D=1024, qn=1024, ldx=1024),
          dict(nseq=0, L=64, D=1021, qn=1000, ldx=1024), dict(nseq=0, qn=1), dict(nseq=0, mask_dtype=3),
          dict(nseq=0, key=P, ldk=12), dict(nseq=0, q=P + 4))
SP_FWD_OK = tuple(dict(kw, ldo=1024) if kw.get("D", 0) > 1000 else kw for kw in _SP_OK) + (dict(nseq=0, ldo=12),)
SP_BWD_OK = tuple(dict(kw, lddx=1024, lddo=kw["qn"]) if kw.get("D", 0) > 1000 else
                  dict(kw, dk=P, lddk=8) if "key" in kw else kw for kw in _SP_OK) + (
    dict(nseq=0, dout=P + 4, lddo=D + 1), dict(nseq=0, dz=P, lddz=12), dict(_KEY, nseq=0, key_tanh=1, lddk=12),
    dict(nseq=0, lddx=12))

CASES = []
for name, cases, ok in (("nr_cnn_keypool_fwd", KP_FWD_CASES, KP_FWD_OK), ("nr_cnn_keypool_bwd", KP_BWD_CASES, ()),
                        ("nr_seq_pool_fwd", SP_FWD_CASES, SP_FWD_OK), ("nr_seq_pool_bwd", SP_BWD_CASES, SP_BWD_OK)):
    for empty in (False, True):     # the checks come before the empty case: the same codes at nseq = 0
        for kw, want in cases:
            if empty and "nseq" in kw:
                continue
            full = dict(kw, nseq=0) if empty else kw
            CASES.append((name, _label(full), _with(BASE[name], **full), want))
    for kw in ok:
        CASES.append((name, _label(kw) + " -> OK", _with(BASE[name], **kw), OK))


@pytest.mark.parametrize("name,cid,args,want", CASES, ids=["%s: %s" % (c[0], c[1]) for c in CASES])
def test_return_code(name, cid, args, want):
    assert len(args) == len(getattr(L.load(), name).argtypes), "the case's argument list is not the ABI's"
    assert _call(name, list(args.values())) == want


@pytest.mark.parametrize("nseq,Hp", [(-1, 64), (3, 0), (3, 16), (3, 48), (3, 192), (3, -32), (0, 161),
                                     (-(1 << 40), 160)])
def test_workspace_refuses_bad_sizes(nseq, Hp):
    assert L.load().nr_cnn_keypool_workspace(nseq, Hp) == -1


def test_wrapper_checks_raise_before_any_launch():
    """kernels.cnn_keypool_* / seq_pool_* refuse a wrong device, size or layout on the host."""
    import torch
    from newsrec_amd import kernels as K
    c = torch.zeros(15, 64)
    w = torch.zeros(64, 64)
    v = torch.zeros(64)
    m = torch.ones(15, dtype=torch.int64)
    with pytest.raises(L.HipError):
        K.cnn_keypool_fwd(c, w, v, v, m, 3, 5, c, v, qn=40)                                   # CPU tensors
    with pytest.raises(L.HipError):
        K.cnn_keypool_bwd(c, w, v, v, 3, 5, 40, v, c, c, w, v, v[:40], v[:40])
    with pytest.raises(L.HipError):
        K.seq_pool_fwd(c, v, m, 3, 5, 64, c, v)
    with pytest.raises(L.HipError):
        K.seq_pool_bwd(c, v, m, 3, 5, 64, v, c, c, v)
    assert not K.cnn_keypool_supported(48, 5) and not K.cnn_keypool_supported(192, 5)
    assert not K.cnn_keypool_supported(64, 33) and not K.cnn_keypool_supported(64, 0)
    assert K.cnn_keypool_supported(32, 1) and K.cnn_keypool_supported(160, 32)
    assert not K.seq_pool_supported(1025, 5) and not K.seq_pool_supported(0, 5)
    assert not K.seq_pool_supported(8, 65) and not K.seq_pool_supported(8, 0)
    assert K.seq_pool_supported(1, 1) and K.seq_pool_supported(1024, 64)
