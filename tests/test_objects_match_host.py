"""CPU checks of -eval -objects --match-iou's host side: the checker of tests/objects_match_ref.py against a statement in Python sets,
the flag's parsing and refusals, match_report, the argument checks of cgs_amd.objects.match and of the entry point.  Nothing here
needs a GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_match_ref  # noqa: E402
import objects_ref  # noqa: E402
from cgs_amd import _lib, build, cli, objects  # noqa: E402

MILLI = (500, 750, 950, 1000)


def _by_sets(pred, truth, milli, K):
    """The independent statement: pixel sets from np.nonzero, Python set intersection and union, Fractions."""
    h, w = pred.shape
    sets = [{a: set(zip(*np.nonzero(m == a))) for a in range(1, min(int(m.max()), K) + 1)} for m in (pred, truth)]
    counts = np.zeros(2 + 2 * len(milli), dtype=np.int32)
    counts[:2] = max(int(pred.max()), 0), max(int(truth.max()), 0)
    best = np.zeros((2, K, 4), dtype=np.int32)
    for side in (0, 1):
        for a, own in sets[side].items():
            top, row = Fraction(0), (0, 0, len(own), 0)
            for b, other in sorted(sets[1 - side].items()):
                both = own & other
                if both and Fraction(len(both), len(own | other)) > top:
                    top, row = Fraction(len(both), len(own | other)), (b, len(both), len(own), len(other))
            best[side, a - 1] = row
            for k, m in enumerate(milli):
                counts[2 + 2 * k + side] += bool(top) and top >= Fraction(m, 1000)
    return counts, best


def test_checker_against_python_sets():
    frames = []
    for seed in range(3):
        pred, truth = objects_match_ref.generator_frame(seed)
        frames += [(objects_ref.label_frame(pred, conn)[0], objects_ref.label_frame(truth, conn)[0]) for conn in (4, 8)]
    pats = objects_ref.patterns()
    lab = lambda name, conn: objects_ref.label_frame(pats[name], conn)[0]
    frames += [(lab("random0.593", 4)[:24, :24], lab("random0.45", 8)[:24, :24]), (lab("comb", 8), lab("serpentine", 8)),
               (lab("full", 8), lab("spiral", 8)), (lab("full", 4), lab("empty", 4)), (lab("checkerboard", 4)[:9, :9], lab("full", 4)[:9, :9])]
    rs = np.random.RandomState(2)
    frames += [(rs.randint(-1, 5, (5, 7)), rs.randint(-1, 4, (5, 7))), (rs.randint(0, 12, (9, 6)), rs.randint(0, 3, (9, 6)))]     # hand-made
    for pred, truth in frames:
        for K in (2, 7, 64):
            counts, best, sums = objects_match_ref.match_frame(pred, truth, MILLI, K)
            want_counts, want_best = _by_sets(pred, truth, MILLI, K)
            np.testing.assert_array_equal(counts, want_counts)
            np.testing.assert_array_equal(best, want_best)
            for k, m in enumerate(MILLI):                                  # the sums: the best IoU of every matched predicted object
                rows = [r for r in want_best[0] if r[1] > 0 and Fraction(int(r[1]), int(r[2] + r[3] - r[1])) >= Fraction(m, 1000)]
                assert sorted(sums[k]) == sorted(Fraction(int(r[1]), int(r[2] + r[3] - r[1])) for r in rows)


def test_match_iou_flag_parses_and_refuses():
    assert objects.parse_match_iou("0.5") == [0.5]
    assert objects.parse_match_iou("0.5-0.75-0.95") == [0.5, 0.75, 0.95]
    assert objects.iou_milli(objects.parse_match_iou("0.5:0.95:10")) == list(range(500, 951, 50))
    assert objects.parse_match_iou("1-0.5") == [1.0, 0.5]                  # in the order given
    a = cli.parse_args(["-eval", "-objects", "--match-iou", "0.5:0.95:10"])
    assert a.match_iou == "0.5:0.95:10" and cli.parse_args(["-eval", "-objects"]).match_iou == ""
    assert cli.parse_args(["-test", "-objects", "--match-iou", "0.5"]).eval
    seventeen = "-".join(f"{0.5 + 0.01 * k:.2f}" for k in range(17))
    assert len(objects.parse_match_iou(seventeen[:-5])) == 16
    for bad in (["-eval", "--match-iou", "0.5"], ["-process", "-objects", "--match-iou", "0.5"],
                ["-process", "-eval", "-objects", "--match-iou", "0.5"], ["-eval", "-objects", "--match-iou", "0.4"],
                ["-eval", "-objects", "--match-iou", "1.01"], ["-eval", "-objects", "--match-iou", "0.5005"],
                ["-eval", "-objects", "--match-iou", "0.5-0.75-0.5"], ["-eval", "-objects", "--match-iou", "0.5:0.5:2"],
                ["-eval", "-objects", "--match-iou", seventeen], ["-eval", "-objects", "--match-iou", "0.5-"],
                ["-eval", "-objects", "--match-iou", "0.5--0.75"], ["-eval", "-objects", "--match-iou", "a"],
                ["-eval", "-objects", "--match-iou", "0.5:0.9"], ["-eval", "-objects", "--match-iou", "0.5:0.9:0"],
                ["-eval", "-objects", "--match-iou", "nan"]):
        with pytest.raises(ValueError):
            cli.parse_args(bad)
        with pytest.raises(ValueError):
            cli.main(bad + ["--model", "nowhere"])                         # before a Handler (a GPU) is asked for


def test_match_report():
    iou = (0.5, 0.75, 1.0)
    pred_max, truth_max = [3, 0, 70, 2], [2, 1, 1, 65]
    mp = [[2, 1, 0], [0, 0, 0], [1, 1, 0], [1, 0, 0]]
    mt = [[2, 1, 0], [0, 0, 0], [1, 1, 0], [2, 0, 0]]                      # the last frame: one predicted object matched two
    r = objects.match_report(pred_max, truth_max, mp, mt, [2.5, 1.75, 0.0], iou)
    assert (r["pred_objects"], r["truth_objects"], r["overflow_frames"]) == (75, 69, 2)
    a, b, c = r["per_iou"]
    assert a == {"iou": 0.5, "matched_pred": 4, "matched_truth": 5, "fp": 71, "fn": 64, "precision": 4 / 75, "recall": 5 / 69,
                 "f1": 2 * (4 / 75) * (5 / 69) / (4 / 75 + 5 / 69), "sum_iou": 2.5, "pq": 2.5 / (4 + 71 / 2 + 64 / 2)}
    assert (b["matched_pred"], b["fp"], b["fn"], b["pq"]) == (2, 73, 67, 1.75 / (2 + 73 / 2 + 67 / 2))
    assert (c["matched_pred"], c["precision"], c["recall"], c["f1"], c["pq"]) == (0, 0.0, 0.0, None, 0.0)     # 0 / 0 in f1 only
    assert r["overflow_frames"] == 2 and objects.match_report(pred_max, truth_max, mp, mt, [2.5, 1.75, 0.0], iou, max_objects=7)["overflow_frames"] == 2
    assert objects.match_report([3, 70], [2, 1], mp[:2], mt[:2], [1.0, 1.0, 0.0], iou, max_objects=70)["overflow_frames"] == 0
    # tensors give the same
    t = objects.match_report(torch.tensor(pred_max, dtype=torch.int32), torch.tensor(truth_max, dtype=torch.int32), torch.tensor(mp, dtype=torch.int32),
                             torch.tensor(mt, dtype=torch.int32), torch.tensor([2.5, 1.75, 0.0], dtype=torch.float64), iou)
    assert t == r
    # no objects at all: every ratio has a zero denominator
    e = objects.match_report([0, 0], [0, 0], [[0], [0]], [[0], [0]], [0.0], [0.5])
    assert e == {"pred_objects": 0, "truth_objects": 0, "overflow_frames": 0, "per_iou": [
        {"iou": 0.5, "matched_pred": 0, "matched_truth": 0, "fp": 0, "fn": 0, "precision": None, "recall": None, "f1": None, "sum_iou": 0.0,
         "pq": None}]}
    # predictions but no truth: precision 0, recall null
    p = objects.match_report([2], [0], [[0]], [[0]], [0.0], [0.5])["per_iou"][0]
    assert (p["fp"], p["fn"], p["precision"], p["recall"], p["f1"], p["pq"]) == (2, 0, 0.0, None, None, 0.0)
    for bad in (dict(truth_max=[1]), dict(mp=[[1, 1, 1]]), dict(sums=[1.0]), dict(mp=[[4, 0, 0], [0, 0, 0], [0, 0, 0], [80, 0, 0]]),
                dict(iou=(0.5, 0.5, 1.0)), dict(iou=(0.4, 0.5, 1.0))):
        kw = {"pred_max": pred_max, "truth_max": truth_max, "mp": mp, "mt": mt, "sums": [2.5, 1.75, 0.0], "iou": iou, **bad}
        with pytest.raises(ValueError):
            objects.match_report(kw["pred_max"], kw["truth_max"], kw["mp"], kw["mt"], kw["sums"], kw["iou"])


def test_sum_iou_on_the_host():
    """sum_iou is plain torch: the rows of a checker's `best` give the checker's sums."""
    pred, truth = objects_match_ref.generator_frame(1)
    pl, tl = objects_ref.label_frame(pred, 8)[0][None], objects_ref.label_frame(truth, 8)[0][None]
    counts, best, sums = objects_match_ref.match(pl, tl, MILLI)
    assert sums[0] > sums[2] > 0
    got = objects.sum_iou(torch.from_numpy(best), [m / 1000 for m in MILLI])
    assert got.dtype == torch.float64 and got.shape == (4,)
    np.testing.assert_allclose(got.numpy(), sums, rtol=1e-12, atol=0)


def test_match_argument_errors():
    z = torch.zeros(2, 8, 8, dtype=torch.int32)
    for bad in (dict(iou=()), dict(iou=(0.4,)), dict(iou=(1.001,)), dict(iou=(0.5005,)), dict(iou=(0.5, 0.5)), dict(iou=0.5),
                dict(iou=[0.5 + 0.01 * k for k in range(17)]), dict(iou=(float("nan"),)), dict(max_objects=0), dict(max_objects=65),
                dict(max_objects=1.5)):
        with pytest.raises(ValueError):
            objects.match(z, z, **bad)
    for a, b in ((z, z[:1]), (z, z[:, :4]), (z.float(), z.float()), (z, z.long()), (z.bool(), z), (z[0, 0], z[0, 0]), (z[None], z[None]),
                 (torch.zeros(2, 65, 8, dtype=torch.int32),) * 2, (torch.zeros(0, 8, 8, dtype=torch.int32),) * 2, (z.numpy(), z)):
        with pytest.raises(ValueError):
            objects.match(a, b)


def test_match_has_no_cpu_path():
    """Label maps in host memory: CgsError, with or without a GPU in the machine."""
    z = torch.zeros(2, 8, 8, dtype=torch.int32)
    with pytest.raises(_lib.CgsError):
        objects.match(z, z)
    with pytest.raises(_lib.CgsError):
        objects.match(z[0], z[0], iou=(0.5, 0.75), max_objects=7, want_best=False)


def test_match_entry_point_is_declared_and_checks_its_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_objects_match\s*\(", text)
    assert "objects_match.hip" in build.SOURCES and "cgs_objects_match" in _lib.SIGNATURES
    assert (_lib.OBJ_MATCH_MAX_OBJECTS, _lib.OBJ_MATCH_MAX_IOU) == (64, 16)
    assert re.search(r"CGS_OBJ_MATCH_MAX_OBJECTS\s*=\s*64\b", text) and re.search(r"CGS_OBJ_MATCH_MAX_IOU\s*=\s*16\b", text)
    lib = _lib.load()
    # argument checks come before anything is launched: safe without a GPU (the pointers are never followed)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    ok = dict(pred=p, truth=p, n=1, h=4, w=4, K=4, iou=p, T=1, counts=p, best=None)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cgs_objects_match(a["pred"], a["truth"], a["n"], a["h"], a["w"], a["K"], a["iou"], a["T"], a["counts"], a["best"], None)

    for bad in (dict(pred=None), dict(truth=None), dict(iou=None), dict(counts=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=-1), dict(K=0),
                dict(K=-5), dict(T=0), dict(T=17), dict(T=-1), dict(pred=p + 2), dict(truth=p + 1), dict(iou=p + 2), dict(counts=p + 3),
                dict(best=p + 2)):
        assert call(**bad) == _lib.ERR_BADARG, bad
    assert call(h=65) == _lib.ERR_UNSUPPORTED and call(w=65) == _lib.ERR_UNSUPPORTED and call(K=65) == _lib.ERR_UNSUPPORTED
    assert call(h=4096, w=4096, K=4096) == _lib.ERR_UNSUPPORTED
    for bad in (dict(h=65, T=17), dict(K=65, counts=None), dict(w=65, n=0)):
        assert call(**bad) == _lib.ERR_BADARG, bad                      # a bad argument is reported before an unsupported size
