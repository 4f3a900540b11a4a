"""CPU checks of -eval --boundary-tol's host side: tol_squared and the flag's parsing and refusals, boundary_report on hand-written
counts, the argument checks of cgs_amd.boundary.score and of the entry point, and the checker of tests/boundary_ref.py against
scipy's Euclidean distance transform.  Nothing here needs a GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import boundary_ref as ref  # noqa: E402
import objects_match_ref  # noqa: E402
from cgs_amd import _lib, boundary, build, cli  # noqa: E402


def test_tol_squared():
    assert boundary.tol_squared([1.415, 1.414, 0, 128]) == [2, 1, 0, 16384]
    assert boundary.tol_squared((1,)) == [1] and boundary.tol_squared([89.1, 89.0]) == [7938, 7921]
    assert boundary.tol_squared([3, 0, 1.5]) == [9, 0, 2]                  # the order given
    assert boundary.tol_squared(np.array([2.0, 2.236, 2.237])) == [4, 4, 5]
    assert all(type(v) is int for v in boundary.tol_squared([0.5, 127.999]))
    assert boundary.tol_squared([0.001 * k for k in range(1000, 1016)]) == [1] * 16       # 16 distinct tolerances, one bound
    for bad in ((), [0.1 * k for k in range(17)], (float("nan"),), (float("inf"),), (-0.001,), (128.001,), (1.0005,), (1, 1.0), (2, 1, 2),
                1.0, None, ("a",)):
        with pytest.raises(ValueError):
            boundary.tol_squared(bad)


def test_boundary_tol_flag_parses_and_refuses():
    assert boundary.parse_boundary_tol("0-1-2-3") == [0.0, 1.0, 2.0, 3.0]
    assert boundary.parse_boundary_tol("0:3:4") == [0.0, 1.0, 2.0, 3.0]
    assert boundary.parse_boundary_tol(" 1.5-0.5 ") == [1.5, 0.5] and boundary.parse_boundary_tol("2") == [2.0]
    for bad in ("", "a", "1-", "1--2", "-1", "0-0", "1-1.0", "129", "0.0005", "0:1:0", "0:16:17", "nan", "inf", "1;2"):
        with pytest.raises(ValueError, match="--boundary-tol"):
            boundary.parse_boundary_tol(bad)
    assert cli.parse_args([]).boundary_tol == ""
    assert cli.parse_args(["-eval", "--boundary-tol", "0-1-2"]).boundary_tol == "0-1-2"
    assert cli.parse_args(["-test", "--boundary-tol", "1"]).boundary_tol == "1"
    assert cli.parse_args(["-eval", "-crf", "-objects", "--boundary-tol", "0:3:4"]).boundary_tol == "0:3:4"
    for argv in (["--boundary-tol", "1"], ["-process", "--boundary-tol", "1"], ["-train", "--boundary-tol", "0-1"],
                 ["-process", "-objects", "--boundary-tol", "1"]):
        with pytest.raises(ValueError, match="-eval"):
            cli.parse_args(argv)
    with pytest.raises(ValueError, match="--boundary-tol"):
        cli.parse_args(["-eval", "--boundary-tol", "1-1"])


def _report(rows, per, tol):
    """rows: per frame (pred_px, truth_px, hd2_pred, hd2_truth); per: per frame and tolerance (hit_pred, hit_truth, inter, union)."""
    rows, per = np.array(rows, dtype=np.int32), np.array(per, dtype=np.int32)
    return boundary.boundary_report(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], per[:, :, 0], per[:, :, 1], per[:, :, 2], per[:, :, 3], tol)


def test_boundary_report():
    # frame 0: both sides; frame 1: only the prediction has a boundary; frame 2: nothing at all; frame 3: both sides
    rows = [(10, 8, 9, 4), (5, 0, -1, -1), (0, 0, -1, -1), (4, 4, 1, 16)]
    per = [[(5, 4, 6, 20), (10, 8, 12, 18)], [(0, 0, 0, 7), (0, 0, 0, 9)], [(0, 0, 0, 0), (0, 0, 0, 0)], [(2, 4, 3, 6), (4, 4, 5, 6)]]
    rep = _report(rows, per, (0, 2.5))
    assert rep["frames"] == 4 and rep["pred_px"] == 19 and rep["truth_px"] == 12
    r0, r1 = rep["per_tol"]
    assert (r0["tol"], r0["tol2"], r1["tol"], r1["tol2"]) == (0.0, 0, 2.5, 6)
    assert (r0["hit_pred"], r0["hit_truth"], r0["band_inter"], r0["band_union"]) == (7, 8, 9, 33)
    assert r0["precision"] == 7 / 19 and r0["recall"] == 8 / 12 and r0["boundary_iou"] == 9 / 33
    assert r0["f"] == 2 * (7 / 19) * (8 / 12) / (7 / 19 + 8 / 12)
    f = lambda p, r: 2 * p * r / (p + r)
    assert r0["frame_mean_f"] == math.fsum([f(5 / 10, 4 / 8), 0.0, f(2 / 4, 4 / 4)]) / 3      # the one-sided frame counts as 0, the empty one not at all
    assert r1["precision"] == 14 / 19 and r1["recall"] == 1.0 and r1["boundary_iou"] == 17 / 33
    assert r1["frame_mean_f"] == math.fsum([1.0, 0.0, 1.0]) / 3
    assert rep["hausdorff"] == {"frames": 2, "max": 4.0, "mean": 3.5, "one_sided": 1}
    assert rep["best"] == {"index": 1, "tol": 2.5, "f": r1["f"], "boundary_iou": {"index": 1, "tol": 2.5, "value": 17 / 33},
                           "hausdorff_max": 4.0, "hausdorff_mean": 3.5}
    assert all(type(r0[k]) is int for k in ("tol2", "hit_pred", "hit_truth", "band_inter", "band_union"))
    # tensors are taken as arrays are
    t = lambda a: torch.tensor(np.array(a, dtype=np.int32))
    rows_a, per_a = np.array(rows), np.array(per)
    assert boundary.boundary_report(*(t(rows_a[:, i]) for i in range(4)), *(t(per_a[:, :, i]) for i in range(4)), (0, 2.5)) == rep

    # empty denominators: no boundary anywhere
    rep = _report([(0, 0, -1, -1)] * 2, [[(0, 0, 0, 0)]] * 2, (1,))
    r = rep["per_tol"][0]
    assert all(math.isnan(r[k]) for k in ("precision", "recall", "f", "boundary_iou", "frame_mean_f"))
    assert rep["hausdorff"]["frames"] == 0 and math.isnan(rep["hausdorff"]["max"]) and math.isnan(rep["hausdorff"]["mean"])
    assert rep["hausdorff"]["one_sided"] == 0 and rep["best"]["index"] == 0 and math.isnan(rep["best"]["f"])
    # one side empty over the whole stack: precision has a denominator, recall has none; a filled truth band still makes a union
    rep = _report([(6, 0, -1, -1)], [[(0, 0, 0, 11)]], (1,))
    r = rep["per_tol"][0]
    assert r["precision"] == 0.0 and math.isnan(r["recall"]) and math.isnan(r["f"]) and r["boundary_iou"] == 0.0 and r["frame_mean_f"] == 0.0
    assert rep["hausdorff"]["one_sided"] == 1
    # both sides there and nothing within the tolerance: F is 0, not NaN
    rep = _report([(3, 3, 50, 50)], [[(0, 0, 0, 6)]], (0,))
    assert rep["per_tol"][0]["f"] == 0.0 and rep["per_tol"][0]["frame_mean_f"] == 0.0
    # counts that cannot be
    for rows, per in (([(3, 3, 1, 1)], [[(4, 0, 0, 6)]]), ([(3, 3, 1, 1)], [[(0, 0, 7, 6)]]), ([(3, -1, 1, 1)], [[(0, 0, 0, 6)]]),
                      ([(3, 3, -1, -1)], [[(0, 0, 0, 6)]])):
        with pytest.raises(ValueError):
            _report(rows, per, (1,))
    with pytest.raises(ValueError):
        _report([(3, 3, 1, 1)], [[(0, 0, 0, 6)]], (1, 2))                  # two tolerances, one column


def test_score_argument_errors():
    z, f = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8)
    for bad in (dict(tol=()), dict(tol=(-1,)), dict(tol=(128.5,)), dict(tol=(1, 1)), dict(tol=(0.0001,)), dict(tol=1),
                dict(tol=[k for k in range(17)]), dict(tol=(float("nan"),)), dict(thresh=0.5)):
        with pytest.raises(ValueError):
            boundary.score(z, z, **bad)
    for a, b, kw in ((z, z[:1], {}), (z, z[:, :4], {}), (f, z, {}), (f, z, dict(thresh=float("nan"))), (z, f, {}), (z.long(), z, {}),
                     (z[0, 0], z[0, 0], {}), (z[None], z[None], {}), (torch.zeros(2, 65, 8, dtype=torch.uint8),) * 2 + ({},),
                     (torch.zeros(2, 8, 65, dtype=torch.bool),) * 2 + ({},), (torch.zeros(0, 8, 8, dtype=torch.uint8),) * 2 + ({},),
                     (z.numpy(), z, {}), (z, z.numpy(), {})):
        with pytest.raises(ValueError):
            boundary.score(a, b, **kw)


def test_score_has_no_cpu_path():
    """Stacks in host memory: CgsError, with or without a GPU in the machine."""
    z = torch.zeros(2, 8, 8, dtype=torch.bool)
    with pytest.raises(_lib.CgsError):
        boundary.score(z, z)
    with pytest.raises(_lib.CgsError):
        boundary.score(torch.zeros(8, 8), z[0], tol=(0, 1.5), thresh=0.5, inclusive=True, want_dist2=True)


def test_entry_point_is_declared_and_checks_its_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_boundary_score\s*\(", text)
    assert "boundary.hip" in build.SOURCES and "cgs_boundary_score" in _lib.SIGNATURES
    assert (_lib.BOUNDARY_MAX_TOL, _lib.BOUNDARY_MAX_TOL_PX) == (16, 128) == (boundary.MAX_TOL, boundary.MAX_TOL_PX)
    assert re.search(r"CGS_BOUNDARY_MAX_TOL\s*=\s*16\b", text) and re.search(r"CGS_BOUNDARY_MAX_TOL_PX\s*=\s*128\b", text)
    lib = _lib.load()
    # argument checks come before anything is launched: safe without a GPU (the pointers are never followed)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    ok = dict(pred=p, kind=_lib.OBJ_U8, truth=p, n=1, h=4, w=4, tol2=p, T=1, counts=p, dist2=None)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cgs_boundary_score(a["pred"], a["kind"], 0.5, a["truth"], a["n"], a["h"], a["w"], a["tol2"], a["T"], a["counts"],
                                      a["dist2"], None)

    for bad in (dict(pred=None), dict(truth=None), dict(tol2=None), dict(counts=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=-1),
                dict(kind=-1), dict(kind=3), dict(T=0), dict(T=17), dict(T=-1), dict(pred=p + 2, kind=_lib.OBJ_F32_GT),
                dict(pred=p + 1, kind=_lib.OBJ_F32_GE), dict(tol2=p + 2), dict(counts=p + 3), dict(dist2=p + 2)):
        assert call(**bad) == _lib.ERR_BADARG, bad
    assert call(h=65) == _lib.ERR_UNSUPPORTED and call(w=65) == _lib.ERR_UNSUPPORTED and call(h=4096, w=4096) == _lib.ERR_UNSUPPORTED
    assert call(pred=p + 1, h=65) == _lib.ERR_UNSUPPORTED                 # a byte stack may start anywhere
    for bad in (dict(h=65, T=17), dict(w=65, counts=None), dict(w=65, n=0)):
        assert call(**bad) == _lib.ERR_BADARG, bad                      # a bad argument is reported before an unsupported size


def _frames():
    """The generator frames and the hand-made shapes, with a few ragged random frames: [(name, pred, truth)]."""
    frames = [(f"generator{s}",) + objects_match_ref.generator_frame(s) for s in range(6)] + ref.hand_made()
    rs = np.random.RandomState(3)
    for h, w in ((1, 1), (1, 64), (64, 1), (5, 7), (63, 64)):
        frames.append((f"random{h}x{w}", rs.rand(h, w) < 0.5, rs.rand(h, w) < 0.5))
    return frames


def test_checker_on_cases_worked_by_hand():
    z = np.zeros((5, 6), dtype=bool)
    a = z.copy()
    a[1:4, 1:5] = True                                                     # 3 x 4: the middle two pixels are interior
    want = a.copy()
    want[2, 2:4] = False
    np.testing.assert_array_equal(ref.boundary(a), want)
    np.testing.assert_array_equal(ref.boundary(np.ones((4, 5), dtype=bool)),
                                  np.array([[1] * 5, [1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [1] * 5], dtype=bool))      # the frame edge is off
    one = z.copy()
    one[4, 5] = True
    d = ref.dist2(one)
    assert d[0, 0] == 16 + 25 and d[4, 5] == 0 and d[4, 0] == 25 and d.dtype == np.int64
    assert (ref.dist2(z) == -1).all()
    counts, dist = ref.score_frame(a, one, [0, 4, 100])
    # the predicted boundary has 10 pixels, the truth's one; the farthest predicted boundary pixel from (4,5) is (1,1): 9 + 16
    assert counts[:4].tolist() == [10, 1, 25, 2]
    assert counts[4:8].tolist() == [0, 0, 0, 11]                           # tolerance 0: nothing coincides, both bands are the boundaries
    assert counts[8:12].tolist() == [1, 1, 0, 13]                          # only (3,4), at 1 + 1; (3,3) and (2,4) are at 5.  The interior is at 1
    assert counts[12:16].tolist() == [10, 1, 0, 13]                        # everything is near: the bands are the two masks
    assert dist.shape == (2, 5, 6) and dist.dtype == np.int32


def test_checker_against_scipy_edt():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, pred, truth in _frames():
        for side, mask in (("pred", pred), ("truth", truth)):
            bnd = ref.boundary(mask)
            got = ref.dist2(bnd)
            if not bnd.any():
                assert (got == -1).all(), (name, side)
                continue
            want = np.rint(ndimage.distance_transform_edt(~bnd) ** 2).astype(np.int64)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {side}")
