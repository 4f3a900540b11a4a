"""CPU checks of the saliency sweep's host side: the grid parser, sweep_report, the argument checks of cgs_amd.saliency and of
cgs_saliency_sweep (which come before anything is launched), the CLI's refusals, and that metrics.parse_thresh_grid gives what it
gave before its syntax parser was shared.  Nothing here needs a GPU."""
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

import saliency_ref  # noqa: E402
from cgs_amd import _lib, build, cli, metrics, saliency  # noqa: E402


def test_salience_grid_both_syntaxes_in_float64():
    got = saliency.parse_salience_grid("0.25-0.5-0.1")
    assert got.dtype == np.float64 and got.tolist() == [0.25, 0.5, 0.1]                      # order kept, 0.1 stays 0.1
    assert got[2] != float(np.float32(0.1))
    assert saliency.parse_salience_grid("0.5-0.05-0.05-1e-3-1.5").tolist() == [0.5, 0.05, 0.05, 1e-3, 1.5]
    got = saliency.parse_salience_grid("0.01:0.99:99")
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, np.linspace(0.01, 0.99, 99, dtype=np.float64))
    assert saliency.parse_salience_grid("0.001:1.5:1024").shape == (1024,)
    assert saliency.parse_salience_grid(" 0.3 ").tolist() == [0.3]


@pytest.mark.parametrize("bad", ["", "a-b", "0.1:0.2", "0.1:1:0", "0.1:1:1025", "0.1:1:2.5", "0.1-", "nan-0.5", "inf", "0.5-inf", "0",
                                 "0.5-0", "-0.5", "0.5--0.1", "0:1:11", "-".join(["0.5"] * 1025)])
def test_salience_grid_refusals(bad):
    """Malformed, empty, too long, NaN, infinite, zero and negative: the threshold is also the normaliser, it has to be above 0."""
    with pytest.raises(ValueError):
        saliency.parse_salience_grid(bad)


def test_thresh_grid_results_unchanged():
    np.testing.assert_array_equal(metrics.parse_thresh_grid("0.01-0.05-0.5"), np.array([0.01, 0.05, 0.5], dtype=np.float32))
    np.testing.assert_array_equal(metrics.parse_thresh_grid("-0.5-1e-3--2"), np.array([-0.5, 1e-3, -2], dtype=np.float32))
    got = metrics.parse_thresh_grid("0.01:0.99:99")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.linspace(0.01, 0.99, 99, dtype=np.float64).astype(np.float32))
    assert metrics.parse_thresh_grid("0:1:1024").shape == (1024,) and metrics.parse_thresh_grid("inf--inf").tolist() == [np.inf, -np.inf]
    for bad in ("", "a-b", "0.1:0.2", "0:1:0", "0:1:1025", "nan-0.5", "0.1-", "0:1:2.5", "-".join(["0.5"] * 1025)):
        with pytest.raises(ValueError, match="--thresh-grid"):
            metrics.parse_thresh_grid(bad)
    with pytest.raises(ValueError, match="--salience-grid"):
        saliency.parse_salience_grid("a-b")


def test_sweep_report_arithmetic():
    rs = np.random.RandomState(3)
    sal = rs.exponential(1e-4, (2, 64, 64)).astype(np.float32)
    preds = np.array([0.9, 0.6], dtype=np.float32)
    truth = rs.rand(2, 64, 64) < 0.4
    thr = np.array([0.9, 0.1, 0.5])
    n_truth = int(np.count_nonzero(truth))
    for salglobal in (True, False):
        inter, union, _, masks = saliency_ref.sweep(sal, preds, truth, thr, salglobal)
        rep = saliency.sweep_report(thr, inter, union, n_truth, salglobal=salglobal)
        assert set(rep) == {"n_truth", "rows", "best"} and rep["n_truth"] == n_truth and len(rep["rows"]) == 3
        for row, t, m in zip(rep["rows"], thr, masks.astype(bool)):
            tp, fp, fn = np.count_nonzero(m & truth), np.count_nonzero(m & ~truth), np.count_nonzero(~m & truth)
            assert (row["thresh"], row["tp"], row["fp"], row["fn"]) == (float(t), tp, fp, fn) and type(row["thresh"]) is float
            assert row["iou"] == tp / (tp + fp + fn) and row["precision"] == tp / (tp + fp) and row["recall"] == tp / (tp + fn)
            assert ("k" in row) == (not salglobal) and (salglobal or (row["k"] == int(4096 * t) and type(row["k"]) is int))
        b = metrics.best_index([r["iou"] for r in rep["rows"]])
        assert rep["best"] == {"index": b, "thresh": float(thr[b]), "iou": rep["rows"][b]["iou"]}
    # the threshold is not rounded to float32, an empty union is NaN and ranks last
    rep = saliency.sweep_report([0.1, 1.5], [0, 0], [7, 0], 0)
    assert rep["rows"][0]["thresh"] == 0.1 and math.isnan(rep["rows"][1]["iou"]) and rep["best"]["index"] == 0 and rep["best"]["thresh"] == 0.1
    assert saliency.frame_k([1.0 / 4096, np.nextafter(1.0 / 4096, 0.0), 4095.0 / 4096, 0.99999]).tolist() == [1, 0, 4095, 4095]
    with pytest.raises(ValueError):
        saliency.sweep_report([0.1], [5], [4], 6)


def test_argument_errors():
    sal, preds, truth = torch.zeros(2, 64, 64), torch.full((2,), 0.5), torch.zeros(2, 64, 64, dtype=torch.bool)
    bad_calls = [
        (sal, preds, truth, [], True),                                       # T = 0
        (sal, preds, truth, np.linspace(0.1, 0.9, 1025), True),
        (sal, preds, truth, [0.5, float("nan")], True),
        (sal, preds, truth, [0.5, 0.0], True),
        (sal, preds, truth, [0.5, 0.0], False),
        (sal, preds, truth, [-0.5], False),
        (sal, preds, truth, [0.5, 1.0], False),                              # int(4096 * 1.0) = 4096
        (sal.double(), preds, truth, [0.5], True),
        (sal, preds.double(), truth, [0.5], True),
        (sal, preds, truth.float(), [0.5], True),
        (torch.zeros(2, 32, 128), preds, truth, [0.5], True),                # 4096 pixels, not 64 x 64
        (torch.zeros(2, 64, 32), preds, torch.zeros(2, 64, 32, dtype=torch.bool), [0.5], True),
        (sal, torch.zeros(3), truth, [0.5], True),
        (sal, preds, torch.zeros(1, 64, 64, dtype=torch.bool), [0.5], True),
        (sal, preds, truth.to("meta"), [0.5], True),                         # a mix of devices
        (sal, preds.to("meta"), truth, [0.5], True),
        (sal, preds, None, [0.5], True),                                     # sweep scores: it needs a truth
    ]
    for a in bad_calls:
        with pytest.raises(ValueError):
            saliency.sweep(*a)
    neg = sal.clone()
    neg[1, 3, 3] = -1e-9
    with pytest.raises(ValueError, match="negative"):
        saliency.sweep(neg, preds, truth, [0.5], True)
    with pytest.raises(ValueError, match="negative"):
        saliency.post(neg, preds, 0.5, False)
    for a in ((sal, preds, 1.0, False), (sal, preds, 0.0, True), (sal, preds, [0.5, 0.6], True), (sal.double(), preds, 0.5, True),
              (sal, preds, 0.5, False, 1e-4)):                               # the last: a mean in per-frame mode
        with pytest.raises(ValueError):
            saliency.post(*a)
    with pytest.raises(ValueError):
        saliency.sweep(sal, preds, truth, [0.5], False, mean=1e-4)


def test_no_cpu_path():
    """Tensors in host memory: CgsError, with or without a GPU in the machine."""
    sal, preds, truth = torch.rand(2, 64, 64), torch.full((2,), 0.5), torch.zeros(2, 64, 64, dtype=torch.bool)
    for salglobal in (True, False):
        with pytest.raises(_lib.CgsError):
            saliency.sweep(sal, preds, truth, [0.25, 0.5], salglobal)
        with pytest.raises(_lib.CgsError):
            saliency.post(sal, preds, 0.5, salglobal)
    with pytest.raises(_lib.CgsError):
        saliency.sweep(sal, preds, truth, [0.25, 0.5], True, mean=0.5)


def test_cli_flag_parses_and_refuses():
    assert cli.parse_args([]).salience_grid == ""
    a = cli.parse_args(["-eval", "-salience", "--salience-grid", "0.25-0.5-0.75"])
    assert a.salience_grid == "0.25-0.5-0.75"
    assert cli.parse_args(["-test", "--salience-grid", "0.1:1.5:15"]).salience        # -test is -eval -salience
    assert cli.parse_args(["-eval", "-salience", "-salglobal", "", "--salience-grid", "0.25-0.99999"]).salglobal is False
    assert cli.parse_args(["-eval", "-salience", "--salience-grid", "0.5-1.0-1.5"]).salglobal                   # global: >= 1 is allowed
    for bad in (["-eval", "--salience-grid", "0.5"],                          # no -salience
                ["-salience", "--salience-grid", "0.5"],                      # no -eval
                ["--salience-grid", "0.5"],
                ["-process", "-salience", "--salience-grid", "0.5"],
                ["-process", "-eval", "-salience", "--salience-grid", "0.5"],
                ["-test", "-process", "--salience-grid", "0.5"],
                ["-eval", "-salience", "--salience-grid", "0.5-x"],
                ["-eval", "-salience", "--salience-grid", "0.5-0"],
                ["-eval", "-salience", "--salience-grid", "0:1:5"],
                ["-eval", "-salience", "-salglobal", "", "--salience-grid", "0.5-1.0"],
                ["-test", "-salglobal", "", "--salience-grid", "0.5-1.5"]):
        with pytest.raises(ValueError):
            cli.parse_args(bad)
    with pytest.raises(ValueError):
        cli.main(["-process", "-salience", "--salience-grid", "0.5", "--source-imgs", "nowhere"])    # before a Handler (a GPU) is asked for


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_saliency_sweep\s*\(", text)
    assert "saliency.hip" in build.SOURCES and "cgs_saliency_sweep" in _lib.SIGNATURES
    assert not any("fast-math" in f or f == "-Ofast" for f in build.EXTRA_FLAGS.get("saliency.hip", []))
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    fn = lib.cgs_saliency_sweep
    # argument checks come before anything is launched: safe without a GPU.  The pointers are host buffers nothing gets to read.
    import ctypes as C
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    ok_tail = (p, p, p, None)                                                # counts, scale, hard, stream
    assert fn(p, p, p, p, p, p, 0, 1, 64, 64, -1, *ok_tail) < 0              # T = 0
    assert fn(p, p, p, p, p, p, 1025, 1, 64, 64, -1, *ok_tail) < 0           # T = 1025
    assert fn(p, p, p, p, p, p, 1, 0, 64, 64, -1, *ok_tail) < 0              # n = 0
    for h, w in ((32, 128), (64, 63), (128, 128), (64, 0)):                  # 4096 pixels in another shape, and other sizes
        assert fn(p, p, p, p, p, p, 1, 1, h, w, -1, *ok_tail) < 0
    assert fn(p, p, p, p, p, p, 1, 1, 32, 128, -1, *ok_tail) == _lib.ERR_UNSUPPORTED
    assert fn(p, p, p, p, p, p, 2, 1, 64, 64, 2, *ok_tail) == _lib.ERR_BADARG          # which = T
    assert fn(p, p, p, p, p, p, 2, 1, 64, 64, -2, *ok_tail) == _lib.ERR_BADARG
    assert fn(None, p, p, p, p, p, 1, 1, 64, 64, -1, *ok_tail) == _lib.ERR_BADARG
    assert fn(p, p, p, p, None, None, 1, 1, 64, 64, -1, *ok_tail) == _lib.ERR_BADARG   # neither gscale nor k
    assert fn(p, p, p, p, p, p, 1, 1, 64, 64, -1, None, p, p, None) == _lib.ERR_BADARG # a truth and no counts
    assert fn(p, p, None, p, p, p, 1, 1, 64, 64, 0, None, p, None, None) == _lib.ERR_BADARG    # a mask asked for and nowhere to put it
    assert fn(p, p, p, p + 4, p, p, 1, 1, 64, 64, -1, *ok_tail) == _lib.ERR_BADARG     # thr is float64: 8-byte aligned
