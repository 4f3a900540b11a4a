"""CPU checks of the -eval sweeps' host side: the two grid parsers, the grid's product order, curve_report, the argument checks of
cgs_amd.metrics and the CLI's refusals.  Nothing here needs a GPU."""
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

import metrics_ref  # noqa: E402
from cgs_amd import _lib, build, cli, crf, metrics  # noqa: E402


def test_thresh_grid_dash_separated_and_linspace():
    np.testing.assert_array_equal(metrics.parse_thresh_grid("0.01-0.05-0.5"), np.array([0.01, 0.05, 0.5], dtype=np.float32))
    assert metrics.parse_thresh_grid("0.05").tolist() == [float(np.float32(0.05))]
    np.testing.assert_array_equal(metrics.parse_thresh_grid("0.5-0.05-0.05"), np.array([0.5, 0.05, 0.05], dtype=np.float32))   # order kept
    np.testing.assert_array_equal(metrics.parse_thresh_grid("-0.5-1e-3--2"), np.array([-0.5, 1e-3, -2], dtype=np.float32))
    got = metrics.parse_thresh_grid("0.01:0.99:99")
    assert got.dtype == np.float32 and got.shape == (99,)
    np.testing.assert_array_equal(got, np.linspace(0.01, 0.99, 99, dtype=np.float64).astype(np.float32))
    assert metrics.parse_thresh_grid("0:1:1024").shape == (1024,)
    for bad in ("", "a-b", "0.1:0.2", "0:1:0", "0:1:1025", "nan-0.5", "0.1-", "0:1:2.5", "-".join(["0.5"] * 1025)):
        with pytest.raises(ValueError):
            metrics.parse_thresh_grid(bad)


def test_crf_grid_parser_and_reference_product_order():
    g = crf.parse_crf_grid("w1=5,22;alpha=12;it=2,10")
    assert g == {"w1": [5, 22], "alpha": [12], "beta": [3.1], "w2": [8], "gamma": [1.8], "it": [2, 10]}
    assert crf.grid_points(g) == [(5, 12, 3.1, 8, 1.8, 2), (5, 12, 3.1, 8, 1.8, 10), (22, 12, 3.1, 8, 1.8, 2), (22, 12, 3.1, 8, 1.8, 10)]
    assert crf.grid_points(crf.parse_crf_grid("")) == [tuple(crf.REFERENCE_PARAMS)]
    assert crf.GRID_KEYS == ("w1", "alpha", "beta", "w2", "gamma", "it")
    g = crf.parse_crf_grid(" it=1,2 ; gamma=1.5,2 ;w2=3,4; beta=5,6.5; alpha=7,8; w1=9,10 ")
    w1, alpha, beta, w2, gamma, it = (g[k] for k in crf.GRID_KEYS)
    want = [(a, b, c, d, e, i) for a in w1 for b in alpha for c in beta for d in w2 for e in gamma for i in it]       # main.py:1238
    assert crf.grid_points(g) == want and len(want) == 64 and want[1] == (9, 7, 5, 3, 1.5, 2)
    for bad in ("w3=1", "w1", "w1=", "w1=a", "w1=1;w1=2", "it=2.5", "it=-1", "alpha=0", "beta=-1", "gamma=0", "w1=nan", "w1=inf", "w1=1,,2"):
        with pytest.raises(ValueError):
            crf.parse_crf_grid(bad)


def test_curve_report_arithmetic():
    rs = np.random.RandomState(0)
    v = rs.rand(500).astype(np.float32)
    truth = rs.rand(500) < 0.4
    thr = np.array([0.9, 0.1, 0.5], dtype=np.float32)
    inter, union = metrics_ref.curve(v, truth, thr)
    rep = metrics.curve_report(thr, inter, union, np.count_nonzero(truth))
    assert rep["n_truth"] == np.count_nonzero(truth) and len(rep["rows"]) == 3
    for row, t in zip(rep["rows"], thr):
        on = v > t
        tp, fp, fn = np.count_nonzero(on & truth), np.count_nonzero(on & ~truth), np.count_nonzero(~on & truth)
        assert (row["thresh"], row["tp"], row["fp"], row["fn"]) == (float(t), tp, fp, fn)
        assert row["iou"] == tp / (tp + fp + fn) and row["precision"] == tp / (tp + fp) and row["recall"] == tp / (tp + fn)
        assert all(type(row[k]) is int for k in ("tp", "fp", "fn"))
    b = max(range(3), key=lambda i: rep["rows"][i]["iou"])
    assert rep["best"] == {"index": b, "thresh": float(thr[b]), "iou": rep["rows"][b]["iou"]}


def test_curve_report_ties_and_nan():
    # equal IoU: the lowest index wins
    rep = metrics.curve_report([0.3, 0.1, 0.2], [5, 6, 6], [10, 12, 12], 8)
    assert [r["iou"] for r in rep["rows"]] == [0.5, 0.5, 0.5] and rep["best"]["index"] == 0
    rep = metrics.curve_report([0.3, 0.1, 0.2], [5, 6, 6], [11, 10, 10], 8)
    assert rep["best"]["index"] == 1
    # no truth and nothing on: an empty union is NaN and ranks last; an empty precision / recall is NaN
    rep = metrics.curve_report([2.0, 0.5], [0, 0], [0, 7], 0)
    assert math.isnan(rep["rows"][0]["iou"]) and math.isnan(rep["rows"][0]["precision"]) and math.isnan(rep["rows"][0]["recall"])
    assert rep["rows"][1]["iou"] == 0.0 and rep["rows"][1]["precision"] == 0.0 and rep["best"]["index"] == 1
    rep = metrics.curve_report([2.0, 3.0], [0, 0], [0, 0], 0)
    assert rep["best"]["index"] == 0 and math.isnan(rep["best"]["iou"])
    assert metrics.best_index([float("nan"), 0.2, 0.2, 0.1]) == 1
    for bad in (([0.1], [1, 2], [3, 4], 1), ([0.1], [5], [4], 6), ([0.1], [2], [3], 5)):
        with pytest.raises(ValueError):
            metrics.curve_report(*bad)


def test_iou_curve_argument_errors():
    p, y = torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.bool)
    with pytest.raises(ValueError):
        metrics.iou_curve(p, y, [0.1, float("nan")])
    with pytest.raises(ValueError):
        metrics.iou_curve(p, y, [])
    with pytest.raises(ValueError):
        metrics.iou_curve(p, y, np.linspace(0, 1, 1025))
    with pytest.raises(ValueError):
        metrics.iou_curve(p, torch.zeros(21, dtype=torch.bool), [0.1])
    with pytest.raises(ValueError):
        metrics.iou_curve(p, y.to("meta"), [0.1])                       # a mix of devices
    with pytest.raises(ValueError):
        metrics.iou_curve(p, y.float(), [0.1])
    with pytest.raises(ValueError):
        metrics.iou_curve(p.double(), y, [0.1])


def test_iou_counts_argument_errors():
    y = torch.zeros(4, 5, dtype=torch.bool)
    with pytest.raises(ValueError):
        metrics.iou_counts(torch.zeros(21, dtype=torch.uint8), y)
    with pytest.raises(ValueError):
        metrics.iou_counts(torch.zeros(2, 10, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8))
    with pytest.raises(ValueError):
        metrics.iou_counts(torch.zeros(40, dtype=torch.uint8), y)       # two stacks, but not [2, ...]
    with pytest.raises(ValueError):
        metrics.iou_counts(torch.zeros(2, 4, 5, dtype=torch.uint8).to("meta"), y)
    with pytest.raises(ValueError):
        metrics.iou_counts(torch.zeros(2, 4, 5), y)


def test_no_cpu_path():
    """Tensors in host memory: CgsError, with or without a GPU in the machine."""
    p, y = torch.rand(4, 5), torch.zeros(4, 5, dtype=torch.bool)
    with pytest.raises(_lib.CgsError):
        metrics.iou_curve(p, y, [0.1, 0.2])
    with pytest.raises(_lib.CgsError):
        metrics.iou_counts(y, y)


def test_cli_flags_parse_and_refuse():
    a = cli.parse_args([])
    assert a.thresh_grid == "" and a.crf_grid == ""
    a = cli.parse_args(["-eval", "-crf", "--thresh-grid", "0.01-0.05-0.5", "--crf-grid", "w1=5,22;it=2,10"])
    assert a.thresh_grid == "0.01-0.05-0.5" and a.crf_grid == "w1=5,22;it=2,10"
    assert cli.parse_args(["-test", "--thresh-grid", "0:1:11"]).eval
    with pytest.raises(ValueError):
        cli.parse_args(["-process", "-crf", "--crf-grid", "w1=5,22"])
    with pytest.raises(ValueError):
        cli.parse_args(["-process", "-eval", "-crf", "--crf-grid", "w1=5,22"])
    with pytest.raises(ValueError):
        cli.main(["-process", "-crf", "--crf-grid", "w1=5,22", "--source-imgs", "nowhere"])      # before a Handler (a GPU) is asked for
    with pytest.raises(ValueError):
        cli.parse_args(["-eval", "--crf-grid", "w1=5,22"])              # no -crf
    with pytest.raises(ValueError):
        cli.parse_args(["-eval", "-crf", "--crf-grid", "w9=5"])
    with pytest.raises(ValueError):
        cli.parse_args(["-eval", "--thresh-grid", "0.1-x"])
    with pytest.raises(ValueError):
        cli.parse_args(["-process", "--thresh-grid", "0.1-0.2"])


def test_metrics_entry_points_are_declared():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_iou_curve\s*\(", text) and re.search(r"\bint cgs_iou_counts\s*\(", text)
    assert "metrics.hip" in build.SOURCES and "cgs_iou_curve" in _lib.SIGNATURES and "cgs_iou_counts" in _lib.SIGNATURES
    lib = _lib.load()
    # argument checks come before anything is launched or allocated: safe without a GPU
    assert lib.cgs_iou_curve(None, None, None, 1, 0, 1, None, None) == _lib.ERR_BADARG
    assert lib.cgs_iou_counts(None, None, 1, 1, None, None) == _lib.ERR_BADARG
