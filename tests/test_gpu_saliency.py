"""The saliency baseline's sweep on the GPU (cgs_saliency_sweep, cgs_amd.saliency, -eval -salience --salience-grid) against
tests/saliency_ref.py, whose masks are Handler._saliency_post's own.  Counts are integers, masks bytes, the normaliser a bit pattern:
exact equality everywhere, except the one check of `mean=None` (2 ulp, from the order of the mean's summation)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import saliency_ref  # noqa: E402
from cgs_amd import _lib, cli, handler, metrics, saliency  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PX = 4096
K01 = 1.0 / 4096                                         # int(4096 * t): 1 here, 0 just below
EDGES = [K01, float(np.nextafter(K01, 0.0)), 4095.0 / 4096, 0.99999, 1e-5, 0.5]       # k = 1, 0, 4095, 4095, 0, 2048


def thresholds(name, salglobal):
    """float64.  Per-frame mode stays below 1 (k <= 4095); global mode also gets 1.0 and values above, where every mask is empty."""
    if name == "one":
        return np.array([0.5])
    if name == "eight":                                  # unsorted, with duplicates
        return np.array([0.5, 0.05, 1.5, 0.05, 1.0, 0.3, 0.5, 0.9] if salglobal else [0.5, 0.05, 0.97, 0.05, 0.7, 0.3, 0.5, 0.9])
    if name == "edges":
        return np.array(EDGES + ([1.0, 1.5] if salglobal else []))
    assert name == "many"
    rs = np.random.RandomState(5)
    thr = rs.uniform(1e-4, 1.2 if salglobal else 0.9999, 1024)
    thr[:len(EDGES)] = EDGES
    if salglobal:
        thr[10:14] = [1.0, 1.5, 1.0, float(np.nextafter(1.0, 0.0))]
    return thr


def _gradients(rs, scale=1e-4):
    return (rs.exponential(scale, PX) * rs.lognormal(0.0, 0.5)).astype(np.float32)


def stack(n, salglobal, seed=0):
    """(sal float32 [n,64,64], preds float32 [n], truth bool [n,64,64]).  Exponential values around 1e-4, as |gradient| sums are.
    n = 1: one such frame.  n = 3: a frame quantised to 20 values (ties straddle every cutoff), a frame with NaN pixels, a plain frame
    with a small prediction.  n = 37: those and an all-zero frame, a frame of 3000 zeros (more than most k), a constant frame, a frame
    whose non-zero values are 5..50 behind 3500 zeros (per-frame mode: S = 0 and sal / tiny overflows), and the predictions 1e-3, 0,
    -0.5, NaN, +inf on plain frames.  +inf pixels only in per-frame mode: one in a stack makes the global mean inf (test_global_inf)."""
    rs = np.random.RandomState(100 * n + seed)
    sal = np.stack([_gradients(rs) for _ in range(n)])
    preds = rs.uniform(0.3, 1.0, n).astype(np.float32)
    truth = rs.rand(n, 64, 64) < 0.3
    if n == 1:
        preds[0] = 0.9
    if n >= 3:
        q = sal[0]
        sal[0] = (np.ceil(q / q.max() * 20) * (q.max() / 20)).astype(np.float32)
        sal[1, rs.choice(PX, 9, replace=False)] = np.nan
        if not salglobal:
            sal[1, rs.choice(PX, 5, replace=False)] = np.inf
        preds[:3] = [0.9, 0.7, 1e-3]
    if n >= 12:
        sal[3] = 0.0
        sal[4, rs.choice(PX, 3000, replace=False)] = 0.0
        sal[5] = np.float32(1.25e-4)
        sal[6] = rs.uniform(5, 50, PX).astype(np.float32) if not salglobal else sal[6] * 30
        sal[6, rs.choice(PX, 3500, replace=False)] = 0.0
        preds[3:12] = [0.9, 0.5, 0.9, 0.8, 1e-3, 0.0, -0.5, np.nan, np.inf]
    return sal.reshape(n, 64, 64), preds, truth


@functools.lru_cache(maxsize=None)
def case(n, salglobal, name):
    """A stack, its thresholds and the reference's answer, computed once and shared (read only)."""
    sal, preds, truth = stack(n, salglobal)
    thr = thresholds(name, salglobal)
    inter, union, scl, masks = saliency_ref.sweep(sal, preds, truth, thr, salglobal)
    on = masks.reshape(len(thr), -1).sum(axis=1)
    assert ((on > 0) & (on < masks[0].size)).any(), "a degenerate case checks nothing"
    for a in (sal, preds, truth, thr, inter, union, scl, masks):
        a.setflags(write=False)
    return sal, preds, truth, thr, inter, union, scl, masks


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # a copy: the shared cases are read-only


def host_mean(sal):
    return np.where(sal >= 0, sal, 0.0).mean()


def bits(a):
    """float32 as bit patterns, every NaN as one (the k-th value of a frame can be a NaN; which NaN is not defined)."""
    a = np.array(a, dtype=np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def raw(sal, preds, truth, thr, salglobal, which, counts=None):
    """cgs_saliency_sweep itself.  Returns (counts, scale, hard) as numpy; counts / hard None when not asked for."""
    n, T = sal.shape[0], len(thr)
    d_sal, d_preds, d_thr = dev(sal), dev(preds), dev(np.asarray(thr, dtype=np.float64))
    d_truth = dev(truth.view(np.uint8)) if truth is not None else None
    d_g = dev((host_mean(sal) * np.asarray(thr).astype(np.float32)).astype(np.float32)) if salglobal else None
    d_k = None if salglobal else dev(saliency.frame_k(thr).astype(np.int32))
    d_counts = counts if counts is not None else (torch.empty((T, 2), dtype=torch.int64, device=DEV) if truth is not None else None)
    d_scale = torch.full((n, T), -7.0, dtype=torch.float32, device=DEV)
    d_hard = torch.full((n, 64, 64), 9, dtype=torch.uint8, device=DEV) if which >= 0 else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.call("cgs_saliency_sweep", ptr(d_sal), ptr(d_preds), ptr(d_truth), ptr(d_thr), ptr(d_g), ptr(d_k), T, n, 64, 64, which,
              ptr(d_counts), ptr(d_scale), ptr(d_hard), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (d_counts.cpu().numpy() if d_counts is not None else None, d_scale.cpu().numpy(),
            d_hard.cpu().numpy() if d_hard is not None else None)


MODES = pytest.mark.parametrize("salglobal", [True, False], ids=["global", "frame"])
# 1024 thresholds on 1 and 3 frames, 37 frames with the short grids: the reference calls _saliency_post once per threshold, which over
# 37 frames 1024 times is about 3 s per mode of reference alone; the kernel's work on a frame does not depend on n
CASES = [(1, "one"), (1, "eight"), (1, "many"), (3, "one"), (3, "eight"), (3, "edges"), (3, "many"), (37, "one"), (37, "eight"), (37, "edges")]


@MODES
@pytest.mark.parametrize("n,name", CASES, ids=[f"n{n}-{name}" for n, name in CASES])
def test_sweep_counts_scale_and_mask(n, name, salglobal):
    sal, preds, truth, thr, inter, union, scl, masks = case(n, salglobal, name)
    got_i, got_u, got_s = saliency.sweep(dev(sal), dev(preds), dev(truth), thr, salglobal, mean=host_mean(sal) if salglobal else None)
    torch.cuda.synchronize()
    assert got_i.dtype == torch.int64 and got_u.dtype == torch.int64 and got_i.shape == (len(thr),) == got_u.shape
    assert got_s.dtype == torch.float32 and got_s.shape == (n, len(thr))
    np.testing.assert_array_equal(got_i.cpu().numpy(), inter)
    np.testing.assert_array_equal(got_u.cpu().numpy(), union)
    np.testing.assert_array_equal(bits(got_s.cpu().numpy()), bits(scl))
    which = len(thr) // 2
    counts, scale, hard = raw(sal, preds, truth, thr, salglobal, which)
    np.testing.assert_array_equal(counts, np.stack([inter, union], axis=1))
    np.testing.assert_array_equal(bits(scale), bits(scl))
    np.testing.assert_array_equal(hard, masks[which])


@MODES
def test_which_at_each_end_none_and_no_truth(salglobal):
    sal, preds, truth, thr, inter, union, scl, masks = case(37, salglobal, "eight")
    want = np.stack([inter, union], axis=1)
    for which in (0, len(thr) - 1):
        counts, scale, hard = raw(sal, preds, truth, thr, salglobal, which)
        np.testing.assert_array_equal(hard, masks[which])
        np.testing.assert_array_equal(counts, want)
    counts, scale, hard = raw(sal, preds, truth, thr, salglobal, -1)
    assert hard is None
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(bits(scale), bits(scl))
    # no truth: the mask and the normaliser come out, counts is left alone
    sentinel = torch.full((len(thr), 2), -3, dtype=torch.int64, device=DEV)
    counts, scale, hard = raw(sal, preds, None, thr, salglobal, 3, counts=sentinel)
    np.testing.assert_array_equal(counts, np.full((len(thr), 2), -3))
    np.testing.assert_array_equal(hard, masks[3])
    np.testing.assert_array_equal(bits(scale), bits(scl))


@MODES
def test_post_is_the_sweeps_mask_and_the_hosts(salglobal):
    sal, preds, truth, thr, inter, union, scl, masks = case(37, salglobal, "eight")
    for i in (0, 2, 7):                                   # global: 0.5, 1.5 (empty, as at the reference's default), 0.9
        hard, scale = saliency.post(dev(sal), dev(preds), float(thr[i]), salglobal, mean=host_mean(sal) if salglobal else None)
        torch.cuda.synchronize()
        assert hard.dtype == torch.uint8 and hard.shape == (37, 64, 64) and scale.dtype == torch.float32 and scale.shape == (37,)
        np.testing.assert_array_equal(hard.cpu().numpy(), masks[i])
        np.testing.assert_array_equal(hard.cpu().numpy(), raw(sal, preds, truth, thr, salglobal, i)[2])
        np.testing.assert_array_equal(bits(scale.cpu().numpy()), bits(scl[:, i]))
        if salglobal and thr[i] >= 1.0:
            assert not hard.any()
    # [n, 1, 64, 64] as the Handler holds the maps
    hard4, _ = saliency.post(dev(sal[:, None]), dev(preds), float(thr[0]), salglobal, mean=host_mean(sal) if salglobal else None)
    np.testing.assert_array_equal(hard4.cpu().numpy(), masks[0])


def test_global_inf_pixel_switches_everything_off():
    sal, preds, truth = (a.copy() for a in stack(3, True))
    sal[2, 5, 7] = np.inf
    thr = np.array([0.3, 0.9])
    inter, union, scl, masks = saliency_ref.sweep(sal, preds, truth, thr, True)
    assert not masks.any() and np.isinf(scl).all()
    counts, scale, hard = raw(sal, preds, truth, thr, True, 0)
    np.testing.assert_array_equal(counts, np.stack([inter, union], axis=1))
    np.testing.assert_array_equal(bits(scale), bits(scl))
    assert not hard.any()


def test_device_mean_is_within_two_ulp():
    """mean=None: torch's float32 mean on the device instead of numpy's pairwise one; the normaliser float32(mean * float32(t)) may
    differ by the mean's last bit and the product's rounding of it: 2 ulp."""
    sal, preds, truth, thr, inter, union, scl, masks = case(37, True, "eight")
    got_i, got_u, got_s = saliency.sweep(dev(sal), dev(preds), dev(truth), thr, True)
    hard, scale1 = saliency.post(dev(sal), dev(preds), 0.5, True)
    torch.cuda.synchronize()
    ulp = np.abs(got_s.cpu().numpy().view(np.int32).astype(np.int64) - scl.view(np.int32).astype(np.int64))
    print("ulp distance of the device mean's normaliser:", ulp.max())
    assert ulp.max() <= 2
    assert got_i.shape == (8,) and hard.shape == (37, 64, 64)
    assert np.abs(scale1.cpu().numpy().view(np.int32).astype(np.int64) - scl[:, 0].view(np.int32).astype(np.int64)).max() <= 2


def test_argument_errors_on_device_tensors():
    sal, preds, truth = (dev(a) for a in stack(3, True))
    neg = sal.clone()
    neg[1, 2, 3] = -1e-6
    with pytest.raises(ValueError):
        saliency.sweep(neg, preds, truth, [0.5], True)
    with pytest.raises(ValueError):
        saliency.post(neg, preds, 0.5, False)
    with pytest.raises(ValueError):
        saliency.sweep(sal, preds.cpu(), truth, [0.5], True)
    with pytest.raises(ValueError):
        saliency.sweep(sal, preds, truth, [0.5, 1.0], False)          # k = 4096
    assert _lib.load().cgs_saliency_sweep(sal.data_ptr(), preds.data_ptr(), None, None, None, None, 1, 3, 32, 64, -1, None, None, None,
                                          None) < 0


# ---------------------------------------------------------------- Handler / CLI, end to end
GRID = "0.25-0.5-0.75"


def _results(out):
    return [float(v) for v in out.split("RESULTS [")[-1].split("]")[0].split(",")]


@MODES
def test_handler_eval_salience_grid(salglobal, tmp_path, golden, g1, monkeypatch, capsys):
    """The synthetic red-trees/ and G1 checkpoints of test_gpu_metrics.py::test_cli_eval_sweeps, -eval -salience --salience-thresh 0.5
    with and without --salience-grid 0.25-0.5-0.75, in process (cli.main).  The grid is the issue's own: on these frames it is not
    degenerate in either mode (asserted below: a row with some but not all pixels on)."""
    from test_gpu_metrics import _structured
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
    monkeypatch.chdir(root)
    sweep_file = os.path.join(root, "m", "eval_sweep.json")
    args = ["--model", "m", "-eval", "-salience", "--salience-thresh", "0.5"] + ([] if salglobal else ["-salglobal", ""])

    H0 = cli.main(args)
    base = capsys.readouterr().out
    assert not os.path.exists(sweep_file) and "SALIENCY SWEEP" not in base and H0.sweep is None
    seen = []
    inner = handler.Handler._sweep_masks
    monkeypatch.setattr(handler.Handler, "_sweep_masks", lambda self, *a, **kw: seen.append(inner(self, *a, **kw)) or seen[-1])
    H = cli.main(args + ["--salience-grid", GRID])
    out = capsys.readouterr().out
    assert out.count("SALIENCY SWEEP 3 thresholds (%s)" % ("global" if salglobal else "frame")) == 1
    assert out.index("SALIENCY SWEEP") < out.index("RESULTS [")
    assert _results(out) == _results(base) and len(_results(out)) == 2
    with open(sweep_file) as fp:
        sweep = json.load(fp)
    assert set(sweep) == {"saliency"} and set(H.sweep) == {"saliency"}
    rep = sweep["saliency"]
    assert set(rep) == {"mode", "n_truth", "rows", "best"} and rep["mode"] == ("global" if salglobal else "frame")

    pick = slice(100, 5000, 2)
    truth = Ye[pick].all(axis=-1)
    (preds, _, sal), = seen                               # what this eval's own H._sweep_masks returned
    thr = [0.25, 0.5, 0.75]
    inter, union, _, masks = saliency_ref.sweep(sal[:, 0], preds, truth, thr, salglobal)
    n_truth = int(np.count_nonzero(truth))
    rows = rep["rows"]
    assert rep["n_truth"] == n_truth and [r["thresh"] for r in rows] == thr
    for r, t, tp, un in zip(rows, thr, inter, union):
        assert (r["tp"], r["fp"], r["fn"]) == (tp, un - n_truth, n_truth - tp)
        assert r["iou"] == tp / un and r["recall"] == tp / n_truth
        assert ("k" in r) == (not salglobal) and (salglobal or r["k"] == int(4096 * t))
    print("pixels on per row:", [r["tp"] + r["fp"] for r in rows], "of", truth.size)
    assert any(0 < r["tp"] + r["fp"] < truth.size for r in rows)
    assert round(rows[1]["iou"], 3) == _results(out)[1]                       # the 0.5 row is --salience-thresh's
    b = metrics.best_index([r["iou"] for r in rows])
    assert rep["best"] == {"index": b, "thresh": rows[b]["thresh"], "iou": rows[b]["iou"]}
