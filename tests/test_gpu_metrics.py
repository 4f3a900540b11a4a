"""Evaluation scoring on the GPU (cgs_iou_curve / cgs_iou_counts, cgs_amd.metrics, Handler.crf's grid search, -eval --thresh-grid /
--crf-grid on the CLI) against the direct numpy form tests/metrics_ref.py.  Everything is integer: exact equality everywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import metrics_ref  # noqa: E402
from cgs_amd import cli, crf, handler, metrics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 5, 7), (2, 64, 64), (37, 64, 64)]         # 105 px: less than a workgroup, odd tail; 2 and 37 frames: several / many workgroups
SPECIAL = [0.0, 1.0, 2.0, -1.0, np.inf, -np.inf, np.nan]


def _thresholds(T, rs):
    if T == 1:
        return np.array([0.05], dtype=np.float32)
    if T == 8:                                           # unsorted, with duplicates
        return np.array([0.5, 0.05, 0.9, 0.05, 0.0, 1.0, 0.5, 0.3], dtype=np.float32)
    if T == 99:
        return np.linspace(0.01, 0.99, 99).astype(np.float32)
    thr = rs.uniform(-0.1, 1.1, T).astype(np.float32)   # 1024, unsorted, with the exact ends of a mask's range among them
    thr[:4] = [0.0, 1.0, 0.0, 1.0]
    return thr


def _stack(shape, thr, seed):
    """Uniform values with a tenth of the pixels exactly 0 / 1, pixels set exactly to thresholds, and the special values."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.05, 1.05, shape).astype(np.float32)
    flat = v.reshape(-1)
    flat[rs.rand(flat.size) < 0.05] = 0.0
    flat[rs.rand(flat.size) < 0.05] = 1.0
    at = rs.choice(flat.size, size=min(flat.size // 3, 4 * len(thr)), replace=False)
    flat[at] = thr[np.arange(len(at)) % len(thr)]        # exactly np.float32(thr): the strict and the inclusive compare differ here
    sp = rs.choice(flat.size, size=2 * len(SPECIAL), replace=False)
    flat[sp] = np.array(SPECIAL * 2, dtype=np.float32)
    truth = rs.rand(*shape) < 0.3
    return v, truth


def _curve(v, truth, thr, inclusive):
    inter, union = metrics.iou_curve(torch.from_numpy(v).to(DEV), torch.from_numpy(truth).to(DEV), thr, inclusive=inclusive)
    torch.cuda.synchronize()
    assert inter.dtype == torch.int64 and union.dtype == torch.int64 and inter.shape == (len(thr),) == union.shape
    return inter.cpu().numpy(), union.cpu().numpy()


@pytest.mark.parametrize("inclusive", [False, True], ids=["strict", "inclusive"])
@pytest.mark.parametrize("T", [1, 8, 99, 1024])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_curve_matches_numpy(shape, T, inclusive):
    thr = _thresholds(T, np.random.RandomState(T))
    v, truth = _stack(shape, thr, seed=7 * T + shape[0])
    want = metrics_ref.curve(v, truth, thr, inclusive)
    got = _curve(v, truth, thr, inclusive)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    if T == 8 and shape == SHAPES[0]:                    # the two compares do differ on this input: the test tells them apart
        other = metrics_ref.curve(v, truth, thr, not inclusive)
        assert (other[0] != want[0]).any() or (other[1] != want[1]).any()


@pytest.mark.parametrize("case", ["all_equal_mid", "all_equal_on_threshold", "bimodal", "truth_clear", "truth_set"])
def test_curve_degenerate_stacks(case):
    shape = SHAPES[2]
    rs = np.random.RandomState(3)
    thr = np.linspace(0.01, 0.99, 99).astype(np.float32)
    v, truth = _stack(shape, thr, seed=11)
    if case == "all_equal_mid":                          # one bin in the middle of the histogram takes every hit
        v = np.full(shape, 0.503, dtype=np.float32)
    elif case == "all_equal_on_threshold":
        v = np.full(shape, thr[40], dtype=np.float32)
    elif case == "bimodal":                              # exact 0 / 1: the first and the last bin only
        v = (rs.rand(*shape) < 0.2).astype(np.float32)
    elif case == "truth_clear":
        truth = np.zeros(shape, dtype=bool)
    else:
        truth = np.ones(shape, dtype=bool)
    for inclusive in (False, True):
        want = metrics_ref.curve(v, truth, thr, inclusive)
        got = _curve(v, truth, thr, inclusive)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_curve_accepts_uint8_truth_noncontiguous_input_and_repeats():
    thr = _thresholds(8, None)
    v, truth = _stack((6, 64, 66), thr, seed=5)
    want = metrics_ref.curve(v[:, ::2, 1:], truth[:, ::2, 1:], thr)
    dv, dt = torch.from_numpy(v).to(DEV)[:, ::2, 1:], (torch.from_numpy(truth).to(DEV).to(torch.uint8) * 255)[:, ::2, 1:]
    assert not dv.is_contiguous() and not dt.is_contiguous()
    a = metrics.iou_curve(dv, dt, thr)
    b = metrics.iou_curve(dv, dt.reshape(-1), list(map(float, thr)))          # another shape with the same element count; a list
    torch.cuda.synchronize()
    for x, y, w in zip(a, b, want):
        np.testing.assert_array_equal(x.cpu().numpy(), w)
        assert torch.equal(x, y)


def _labels(K, shape, seed):
    rs = np.random.RandomState(seed)
    lab = (rs.rand(K, *shape) < 0.4).astype(np.uint8)
    lab[rs.rand(K, *shape) < 0.1] = 255                  # "non-zero" is on, not "one"
    lab[rs.rand(K, *shape) < 0.05] = 2
    truth = rs.rand(*shape) < 0.3
    return lab, truth


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_match_numpy(shape, K):
    lab, truth = _labels(K, shape, seed=K + shape[0])
    want = metrics_ref.counts(lab, truth)
    dl, dt = torch.from_numpy(lab).to(DEV), torch.from_numpy(truth).to(DEV)
    got = metrics.iou_counts(dl, dt)
    again = metrics.iou_counts(dl, dt)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.shape == (K, 2)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    if K == 1:                                           # a single stack of truth's shape: [2]
        one = metrics.iou_counts(dl[0], dt)
        assert one.shape == (2,) and one.tolist() == want[0].tolist()


def test_counts_bool_and_noncontiguous():
    lab, truth = _labels(3, (5, 64, 66), seed=9)
    want = metrics_ref.counts(lab[:, :, ::2, 1:] != 0, truth[:, ::2, 1:])
    dl, dt = (torch.from_numpy(lab).to(DEV) != 0)[:, :, ::2, 1:], torch.from_numpy(truth).to(DEV)[:, ::2, 1:]
    assert dl.dtype == torch.bool and not dl.is_contiguous() and not dt.is_contiguous()
    np.testing.assert_array_equal(metrics.iou_counts(dl, dt).cpu().numpy(), want)
    # uint8 truth holding 255, uint8 labels
    np.testing.assert_array_equal(metrics.iou_counts(torch.from_numpy(lab).to(DEV)[:, :, ::2, 1:], dt.to(torch.uint8) * 255).cpu().numpy(),
                                  metrics_ref.counts(lab[:, :, ::2, 1:], truth[:, ::2, 1:]))
    # a row offset that is no multiple of 16 bytes, for labels and truth separately
    flat_l, flat_t = torch.from_numpy(lab[0]).to(DEV).reshape(-1), torch.from_numpy(truth).to(DEV).reshape(-1)
    got = metrics.iou_counts(flat_l[3:1003], flat_t[3:1003])
    assert got.tolist() == metrics_ref.counts(lab[0].reshape(-1)[3:1003], truth.reshape(-1)[3:1003])[0].tolist()


# ---------------------------------------------------------------- Handler.crf as the grid search
def _structured(h, w, seed):
    """Frames of flat blocks and repeated rows with a noisy disc mask holding exact 0.0 / 1.0 pixels (as tests/test_gpu_crf.py's)."""
    rs = np.random.RandomState(seed)
    frame = np.zeros((h, w, 3), np.uint8)
    for _ in range(6):
        y0, x0 = rs.randint(0, h), rs.randint(0, w)
        frame[y0:y0 + rs.randint(4, h // 2 + 4), x0:x0 + rs.randint(4, w // 2 + 4)] = rs.randint(0, 256, 3)
    frame[h // 3] = rs.randint(0, 256, (w, 3))
    frame[h // 3 + 1:h // 3 + 4] = frame[h // 3]
    frame = np.clip(frame.astype(int) + rs.randint(-2, 3, frame.shape), 0, 255).astype(np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    sd = (min(h, w) / 3.0 - np.hypot(xs - w / 2.0, ys - h / 2.0)) / 3.0
    p = 1.0 / (1.0 + np.exp(-sd)) + rs.normal(0, 0.15, (h, w))
    p = np.clip(p, 0.0, 1.0).astype(np.float32)
    p[rs.rand(h, w) < 0.03] = 1.0
    p[rs.rand(h, w) < 0.03] = 0.0
    return frame, p


def _dense(frames, p1, params):
    out = crf.dense_crf(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), torch.from_numpy(np.ascontiguousarray(p1)).to(DEV), params)
    return out.cpu().numpy()


GRID = "w1=5,22;it=2,10"
GRID_POINTS = [(5, 12, 3.1, 8, 1.8, 2), (5, 12, 3.1, 8, 1.8, 10), (22, 12, 3.1, 8, 1.8, 2), (22, 12, 3.1, 8, 1.8, 10)]


def _check_report(rep, frames, p1, truth):
    """Four rows in the reference's order, each scored as Handler.get_iou scores dense_crf at that point; returns the best labels."""
    assert [tuple(r["params"][k] for k in crf.GRID_KEYS) for r in rep["rows"]] == GRID_POINTS
    labels = [_dense(frames, p1, p) for p in GRID_POINTS]
    for r, lab in zip(rep["rows"], labels):
        assert [r["inter"], r["union"]] == metrics_ref.counts(lab, truth)[0].tolist()
        assert r["iou"] == r["inter"] / r["union"]
        assert round(r["iou"], 3) == handler.Handler.get_iou(lab, truth)
    b = metrics.best_index([r["iou"] for r in rep["rows"]])
    assert rep["best"] == {"index": b, "params": rep["rows"][b]["params"], "iou": rep["rows"][b]["iou"]}
    return labels[b]


def test_handler_crf_grid(tmp_path, golden, monkeypatch):
    monkeypatch.chdir(tmp_path)
    g = golden("g2_eval.npz")
    S = [_structured(64, 64, 40 + s) for s in range(3)]
    frames = np.concatenate([g["X"][:3], np.stack([f for f, _ in S])])
    p1 = np.concatenate([g["Z"][:3, 0].astype(np.float32), np.stack([p for _, p in S])])
    ys, xs = np.mgrid[0:64, 0:64]
    truth = np.broadcast_to(np.hypot(xs - 30.0, ys - 34.0) < 20.0, (6, 64, 64)).copy()
    H = handler.Handler(cli.parse_args(["--model", "m", "-eval", "-crf", "--crf-grid", GRID]))
    out = H.crf(frames, p1[:, None], truth)
    assert out.dtype == bool and out.shape == (6, 1, 64, 64) and len(H.crf_reports) == 1
    best = _check_report(H.crf_reports[0], frames, p1, truth)
    np.testing.assert_array_equal(out[:, 0], best >= 1)
    with pytest.raises(ValueError):
        H.crf(frames, p1[:, None], None)                 # several points and nothing to score them with
    assert len(H.crf_reports) == 1
    # a one-point grid: what the code without a grid returns, scored or (without labels, as -process) not
    H0 = handler.Handler(cli.parse_args(["--model", "m"]))
    plain = H0.crf(frames, p1[:, None], truth)
    np.testing.assert_array_equal(plain[:, 0], _dense(frames, p1, crf.REFERENCE_PARAMS) >= 1)
    assert H0.crf_reports == []
    H1 = handler.Handler(cli.parse_args(["--model", "m", "-eval", "-crf", "--crf-grid", "w1=22"]))
    np.testing.assert_array_equal(H1.crf(frames, p1[:, None], truth), plain)
    np.testing.assert_array_equal(H1.crf(frames, p1[:, None], None), plain)
    assert len(H1.crf_reports) == 1 and len(H1.crf_reports[0]["rows"]) == 1
    assert H1.crf_reports[0]["rows"][0]["inter"] == metrics_ref.counts(plain, truth)[0, 0]
    for kind in ("mask", "img", "crf"):
        assert os.path.isfile(os.path.join("m", "crf", f"0_{kind}.png"))


# ---------------------------------------------------------------- CLI, end to end
def _main(root, args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py")] + args + ["--model", "m"], cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _results(out):
    return [float(v) for v in out.split("RESULTS [")[-1].split("]")[0].split(",")]


def test_cli_eval_sweeps(tmp_path, golden, g1, monkeypatch):
    """The synthetic red-trees/ of test_gpu_crf.py::test_cli_eval_crf: 420 frames (160 evaluated), the G1 weights."""
    root = str(tmp_path)
    pc, pm = g1
    names = [str(s) for s in golden("g6_process.npz")["checkpoint_names"]]
    for name, state in zip(names, (pc, pm)):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    rs = np.random.RandomState(11)
    Xe = np.stack([_structured(64, 64, 200 + k % 40)[0] for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    Ye[:, 20:30, 10:20, 1] = rs.rand(10, 10) < 0.5
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    sweep_file = os.path.join(root, "m", "eval_sweep.json")

    base = _main(root, ["-eval"])
    assert not os.path.exists(sweep_file) and "THRESH SWEEP" not in base and "CRF GRID" not in base
    out = _main(root, ["-eval", "--thresh-grid", "0.01-0.05-0.5"])
    assert out.count("THRESH SWEEP") == 1 and "CRF GRID" not in out
    assert _results(out) == _results(base)
    with open(sweep_file) as fp:
        sweep = json.load(fp)
    assert set(sweep) == {"thresholds"}

    monkeypatch.chdir(root)
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    pick = slice(100, 5000, 2)
    frames, truth = Xe[pick], Ye[pick].all(axis=-1)
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = np.array([0.01, 0.05, 0.5], dtype=np.float32)
    inter, union = metrics_ref.curve(M[:, 0], truth, thr)
    n_truth = int(np.count_nonzero(truth))
    rows = sweep["thresholds"]["rows"]
    assert sweep["thresholds"]["n_truth"] == n_truth and [r["thresh"] for r in rows] == [float(t) for t in thr]
    for r, tp, un in zip(rows, inter, union):
        assert (r["tp"], r["fp"], r["fn"]) == (tp, un - n_truth, n_truth - tp)
        assert r["iou"] == tp / un and r["precision"] == tp / (un - n_truth + tp) and r["recall"] == tp / n_truth
    assert round(rows[1]["iou"], 3) == _results(out)[0]                       # the 0.05 entry is --eval-thresh's
    b = metrics.best_index([r["iou"] for r in rows])
    assert sweep["thresholds"]["best"] == {"index": b, "thresh": rows[b]["thresh"], "iou": rows[b]["iou"]}

    out = _main(root, ["-eval", "-crf", "--crf-grid", GRID])
    assert out.count("CRF GRID") == 1 and "THRESH SWEEP" not in out
    with open(sweep_file) as fp:
        sweep = json.load(fp)
    assert set(sweep) == {"crf"} and set(sweep["crf"]) == {"mask"}
    best = _check_report(sweep["crf"]["mask"], frames, M[:, 0], truth)
    got = _results(out)
    assert len(got) == 2 and got[0] == _results(base)[0] and got[1] == handler.Handler.get_iou(best, truth)
    assert got[1] == round(sweep["crf"]["mask"]["best"]["iou"], 3)
