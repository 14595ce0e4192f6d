"""Writes tests/golden/prediction_ref.npz: fp32 scores of a few dozen impressions, their group
offsets and the bytes of the prediction.txt that Manager.test's expression (utils/Manager.py:842-850)
gives for them, computed here with scipy:

    rank_list = scipy.stats.rankdata(1 - np.asarray(pred), method="ordinal")   # pred: Python floats
    line = str(index) + " [" + ",".join(str(i) for i in rank_list) + "]" + "\\n"

The groups cover the cases where the f64 key 1 - p collides for distinct fp32 scores (ordinal ranks
then follow position), heavy ties, empty groups, infinities, signed zeros and scores outside [0, 1].

    python tests/golden/make_prediction_golden.py
"""
import os

import numpy as np
import scipy.stats as ss

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST_LINE = 8     # lines 8 .. : the line number crosses 9 -> 10


def groups():
    rng = np.random.default_rng(20260)
    out = [np.array([1e-30, 2e-30, 3e-10, 3.0000002e-10, 0.5, 0.5], np.float32),
           np.zeros(0, np.float32),
           np.array([0.25], np.float32),
           np.array([0.0, -0.0, 1.0, 1.5, -2.0, np.inf, -np.inf, 0.0, 1.0], np.float32)]
    for n in (2, 9, 10, 11, 63, 64, 65, 101, 130):
        out.append(rng.random(n, dtype=np.float32))
    for n in (5, 37, 64, 99):
        out.append(rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 0.9], np.float32), n))
    for n in (7, 20, 37, 37, 64, 80, 129, 150):
        x = rng.normal(0.0, 12.0, n).astype(np.float32)
        out.append((1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32))
    out.append(np.zeros(0, np.float32))
    for n in (3, 12, 33):
        out.append(rng.normal(0.0, 3.0, n).astype(np.float32))     # raw scores
    out.append(np.full(70, 1e-12, np.float32) * rng.integers(1, 4, 70).astype(np.float32))
    out.append(np.zeros(0, np.float32))
    return out


def main():
    gs = groups()
    off = np.zeros(len(gs) + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in gs])
    preds = np.concatenate(gs).astype(np.float32)
    text = ""
    for k, g in enumerate(gs):
        rank_list = ss.rankdata(1 - np.asarray(g.tolist()), method="ordinal") if len(g) else []
        text += str(FIRST_LINE + k) + " [" + ",".join([str(int(i)) for i in rank_list]) + "]" + "\n"
    path = os.path.join(HERE, "prediction_ref.npz")
    np.savez_compressed(path, preds=preds, grp_off=off, first_line=np.int64(FIRST_LINE),
                        text=np.frombuffer(text.encode("ascii"), np.uint8))
    print("wrote", path, len(gs), "groups,", len(preds), "scores,", len(text), "bytes of text,",
          os.path.getsize(path), "bytes on disk")


if __name__ == "__main__":
    main()
