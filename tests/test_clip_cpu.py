"""nr_grad_norm_workspace (host arithmetic) and the argument checks of nr_grad_norm_workspace,
nr_grad_norm_multi and nr_adam_multi_clip.  Every check returns before any HIP call, so the entries
run through ctypes on a machine without a GPU: the tensors sit on a 16-B-aligned HOST buffer that
no case ever dereferences."""
import ctypes
import os

import pytest

from clip_util import CHUNK, workspace_floor
from newsrec_amd import _lib as L

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH),
                                reason="library not built (run __graft_entry__.build())")

_BUF = ctypes.create_string_buffer(4096 + 16)
_BASE = (ctypes.addressof(_BUF) + 15) & ~15
_STATE = _BASE + 2048
_TICKET = _BASE + 2064
NAN, INF = float("nan"), float("inf")


def _tensor(n=8, grad=_BASE, param=_BASE, step=1, rt=None, rlen=0):
    return L.nr_adam_tensor(param, grad, _BASE, _BASE, n, 1e-3, step, None, None, rt, rlen)


def _arr(tensors):
    a = (L.nr_adam_tensor * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        a[i] = t
    return a


def _ws(tensors, count=None):
    return L.load().nr_grad_norm_workspace(_arr(tensors) if tensors is not None else None,
                                           len(tensors) if count is None else count)


def _norm(tensors, count=None, grad_scale=1.0, max_norm=2.0, work=_BASE, work_bytes=1024, state=_STATE):
    return L.load().nr_grad_norm_multi(_arr(tensors) if tensors is not None else None,
                                       len(tensors) if count is None else count, grad_scale, max_norm, work,
                                       work_bytes, state, None)


def _clip(tensors, count=None, clip=_STATE, honor_skip=0, ticket=None):
    return L.load().nr_adam_multi_clip(_arr(tensors) if tensors is not None else None,
                                       len(tensors) if count is None else count, 0.9, 0.999, 1e-8, 0.0, clip,
                                       honor_skip, ticket, None)


def _sizes(count):
    """Ragged sizes around the chunk boundaries, deterministic."""
    pool = [0, 1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 30522 * 3, 777, 2 * CHUNK]
    return [pool[(7 * i + 3) % len(pool)] for i in range(count)]


@pytest.mark.parametrize("count", [0, 1, 33, 70])
def test_workspace_covers_one_partial_per_chunk(count):
    sizes = _sizes(count)
    got = _ws([_tensor(n) for n in sizes])
    assert got > 0 and got % 16 == 0
    assert got >= workspace_floor(sizes)
    assert got <= workspace_floor(sizes) + 16        # ... and no more than the rounding


def test_workspace_non_decreasing_in_every_n():
    sizes = _sizes(5)
    base = _ws([_tensor(n) for n in sizes])
    for i in range(len(sizes)):
        prev = base
        for add in (1, CHUNK - 1, CHUNK, 5 * CHUNK + 1):
            grown = list(sizes)
            grown[i] += add
            cur = _ws([_tensor(n) for n in grown])
            assert cur >= prev, (i, add)
            prev = cur
        assert prev > base


WS_CASES = [
    ("count<0", dict(tensors=[_tensor()], count=-1), -1000),
    ("tensors NULL", dict(tensors=None, count=2), -1000),
    ("n<0", dict(tensors=[_tensor(), _tensor(-1)]), -1001),
    ("grad NULL", dict(tensors=[_tensor(8, grad=None)]), -1002),
    ("row_len=0", dict(tensors=[_tensor(8, rt=_BASE, rlen=0)]), -1003),
    ("n % row_len", dict(tensors=[_tensor(8, rt=_BASE, rlen=3)]), -1003),
]


@pytest.mark.parametrize("name,kw,want", WS_CASES, ids=[c[0] for c in WS_CASES])
def test_list_checks(name, kw, want):
    """The list checks are shared by the workspace query and the norm entry."""
    assert _ws(kw["tensors"], kw.get("count")) == want
    assert _norm(kw["tensors"], kw.get("count")) == want


NORM_CASES = [
    ("state NULL", dict(state=None), -1004),
    ("work NULL", dict(work=None), -1005),
    ("work misaligned", dict(work=_BASE + 8), -1005),
    ("work_bytes short", dict(tensors=[_tensor(3 * CHUNK + 5)], work_bytes=24), -1005),
    ("work_bytes 0", dict(tensors=[], work_bytes=0), -1005),
    ("max_norm<0", dict(max_norm=-1.0), -1006),
    ("max_norm NaN", dict(max_norm=NAN), -1006),
    ("grad_scale NaN", dict(grad_scale=NAN), -1007),
]


@pytest.mark.parametrize("name,kw,want", NORM_CASES, ids=[c[0] for c in NORM_CASES])
def test_grad_norm_codes(name, kw, want):
    kw = dict(kw)
    assert _norm(kw.pop("tensors", [_tensor()]), **kw) == want


def test_grad_norm_checks_come_in_order():
    """The first failing check decides: the list before the state, the state before the workspace,
    the workspace before the two scalars."""
    assert _norm([_tensor(-1)], state=None, work=None, max_norm=NAN) == -1001
    assert _norm([_tensor()], state=None, work=None, max_norm=NAN) == -1004
    assert _norm([_tensor()], work=None, max_norm=NAN, grad_scale=NAN) == -1005
    assert _norm([_tensor()], max_norm=NAN, grad_scale=NAN) == -1006
    assert _ws([_tensor(3 * CHUNK + 5)]) == 32         # the byte count the "short" case sits under


CLIP_CASES = [
    ("count<0", dict(tensors=[_tensor()], count=-1), -1000),
    ("tensors NULL", dict(tensors=None, count=1), -1000),
    ("n<0", dict(tensors=[_tensor(-1)]), -1001),
    ("step<1 without step_dev", dict(tensors=[_tensor(step=0)]), -1001),
    ("grad NULL", dict(tensors=[_tensor(8, grad=None)]), -1002),
    ("param NULL", dict(tensors=[_tensor(8, param=None)]), -1002),
    ("row_len=0", dict(tensors=[_tensor(8, rt=_BASE, rlen=0)]), -1005),
    ("n % row_len", dict(tensors=[_tensor(8, rt=_BASE, rlen=3)]), -1005),
    ("clip NULL", dict(tensors=[_tensor()], clip=None), -1006),
    ("clip NULL, ticket", dict(tensors=[_tensor()], clip=None, ticket=_TICKET, honor_skip=1), -1006),
]


@pytest.mark.parametrize("name,kw,want", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_adam_multi_clip_codes(name, kw, want):
    kw = dict(kw)
    assert _clip(kw.pop("tensors"), **kw) == want
