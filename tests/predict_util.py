"""Expected prediction.txt content, built from the definition (Manager.test, utils/Manager.py:842-850):
per impression ``ss.rankdata(1 - np.asarray(pred), method="ordinal")`` over the Python floats of the
fp32 scores, and ``str(index) + " [" + ",".join(str(i) for i in rank_list) + "]" + "\\n"``."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prediction_ref.npz")

# the issue's example: 1 - p in double maps the first two scores to one key and the next two to one
# key, so position orders them; the fp32 order would swap both pairs
COLLISION = np.array([1e-30, 2e-30, 3e-10, 3.0000002e-10, 0.5, 0.5], np.float32)
COLLISION_RANKS = [5, 6, 3, 4, 1, 2]


def ranks_stable(p):
    """The scipy-free definition: a stable argsort of the f64 key 1 - p (equal keys by position)."""
    key = 1.0 - np.asarray(p, np.float32).astype(np.float64)
    order = np.argsort(key, kind="stable")
    r = np.empty(len(key), np.int64)
    r[order] = np.arange(1, len(key) + 1)
    return r


def ranks_expected(p):
    """The reference's own expression where scipy imports, the stable-argsort definition otherwise."""
    p = np.asarray(p, np.float32)
    if len(p) == 0:
        return np.zeros(0, np.int64)
    try:
        import scipy.stats as ss
    except ImportError:
        return ranks_stable(p)
    return ss.rankdata(1 - np.asarray(p.tolist()), method="ordinal")


def group_ranks(preds, off, ranks=ranks_expected):
    return [[int(r) for r in ranks(preds[off[g]:off[g + 1]])] for g in range(len(off) - 1)]


def lines(rank_lists, first_line=1):
    return [str(first_line + g) + " [" + ",".join([str(i) for i in r]) + "]" + "\n" for g, r in enumerate(rank_lists)]


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off
