"""CPU-side checks of the prediction.txt path: the committed golden (written with scipy) re-derives
from its scores by the scipy-free stable-argsort definition, and the public functions refuse CPU
tensors loudly."""
import os

import numpy as np
import pytest
import torch

import predict_util as PU


def test_golden_rederives_from_stable_argsort():
    z = np.load(PU.GOLDEN)
    preds, off, first = z["preds"], z["grp_off"], int(z["first_line"])
    assert preds.dtype == np.float32 and off[0] == 0 and off[-1] == len(preds)
    want = "".join(PU.lines(PU.group_ranks(preds, off, PU.ranks_stable), first))
    assert z["text"].tobytes().decode("ascii") == want
    assert len(off) - 1 >= 24 and (np.diff(off) == 0).sum() >= 3
    # and through the reference's expression where scipy is present (the same function otherwise)
    assert "".join(PU.lines(PU.group_ranks(preds, off), first)) == want


def test_collision_vector_definition():
    assert PU.ranks_stable(PU.COLLISION).tolist() == PU.COLLISION_RANKS
    assert [int(r) for r in PU.ranks_expected(PU.COLLISION)] == PU.COLLISION_RANKS
    z = np.load(PU.GOLDEN)
    np.testing.assert_array_equal(z["preds"][:6], PU.COLLISION)
    assert z["text"].tobytes().decode("ascii").startswith("8 [5,6,3,4,1,2]\n9 []\n10 [1]\n")


def test_predict_path_fails_loudly_without_gpu(tmp_path):
    from newsrec_amd import _lib, evaluate
    p = torch.tensor([0.5, 0.25, 0.75])
    off = torch.tensor([0, 2, 3])
    with pytest.raises(_lib.HipError):
        evaluate.rank_ordinal(p, off)
    with pytest.raises(_lib.HipError):
        evaluate.format_predictions(p, off)
    path = str(tmp_path / "out" / "prediction.txt")
    with pytest.raises(_lib.HipError):
        evaluate.write_predictions(path, p, off)
    assert not os.path.exists(path)


def test_constants_match_header():
    from newsrec_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "newsrec_hip.h")).read()
    assert "#define NR_RANK_MAX_GROUP %d\n" % _lib.RANK_MAX_GROUP in hdr
    assert "NR_RANK_NAN = %d, NR_RANK_GROUP_TOO_LARGE = %d" % (_lib.RANK_NAN, _lib.RANK_GROUP_TOO_LARGE) in hdr
    assert _lib.RANK_MAX_GROUP >= 4096
