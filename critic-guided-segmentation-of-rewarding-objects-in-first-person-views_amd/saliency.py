"""The saliency baseline's post-processing on the GPU (csrc/saliency.hip): what ``Handler._saliency_post`` does with numpy -- normalise
the |gradient| maps, weight them by the critic's prediction, clip at 1, threshold (main.py:976-1003) -- for a whole grid of thresholds
in one launch, every threshold with its own normaliser, scored against the truth where the maps are.  The on/off decision is
``_saliency_post``'s bit for bit (float64, as numpy 2 evaluates it), so every count is exact.
``parse_salience_grid`` and ``sweep_report`` are pure host helpers for ``-eval -salience --salience-grid`` (evaluate.py)."""
import numpy as np
import torch

from . import _lib, metrics

MAX_THRESHOLDS = _lib.SALIENCY_MAX_T
SIDE = _lib.SALIENCY_SIDE
PIXELS = SIDE * SIDE


def frame_k(thresholds):
    """Per-frame mode's index into the sorted frame, ``int(4096 * t)`` in float64 as ``_saliency_post`` takes it.  int64 [T]."""
    return np.trunc(PIXELS * np.asarray(thresholds, dtype=np.float64).reshape(-1)).astype(np.int64)


def _thresholds(thresholds, salglobal):
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    thr = np.array(thresholds, dtype=np.float64).reshape(-1)             # a copy: contiguous, writable, the caller's left alone
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} thresholds, got {thr.size}")
    if not np.isfinite(thr).all() or (thr <= 0).any():
        raise ValueError("every threshold must be a finite number above 0 (the threshold is also the normaliser)")
    if not salglobal and (frame_k(thr) > PIXELS - 1).any():
        raise ValueError(f"per-frame mode indexes the sorted frame at int({PIXELS} * t): every threshold must be below 1")
    return thr


def _run(name, sal, preds, truth, thresholds, salglobal, mean, which):
    thr = _thresholds(thresholds, salglobal)
    if not isinstance(sal, torch.Tensor) or not isinstance(preds, torch.Tensor):
        raise ValueError("sal and preds must be torch tensors")
    if sal.dtype != torch.float32 or preds.dtype != torch.float32:
        raise ValueError(f"sal and preds must be float32, got {sal.dtype} and {preds.dtype}")
    if sal.dim() < 3 or tuple(sal.shape[-2:]) != (SIDE, SIDE) or sal.numel() < PIXELS:
        raise ValueError(f"sal must be [n, {SIDE}, {SIDE}] (or [n, 1, {SIDE}, {SIDE}]), got {tuple(sal.shape)}")
    n = sal.numel() // PIXELS
    if preds.numel() != n:
        raise ValueError(f"{n} frames, {preds.numel()} predictions")
    if n > 0x7FFFFFFF:
        raise ValueError(f"{n} frames: more than one launch holds")
    if truth is not None:
        if not isinstance(truth, torch.Tensor) or truth.numel() != sal.numel():
            raise ValueError(f"truth must be a tensor of sal's {sal.numel()} elements")
        metrics._same_device(sal, preds, truth)
        truth = metrics._flat_u8(truth, "truth")
    else:
        metrics._same_device(sal, preds)
    if bool((sal < 0).any()):
        raise ValueError("sal holds a negative value: a saliency map is a sum of absolute gradients")
    if mean is not None and not salglobal:
        raise ValueError("mean belongs to the global mode")
    metrics._need_gpu(name, "cgs_saliency_sweep", sal)
    sal, preds = sal.reshape(n, PIXELS).contiguous(), preds.reshape(n).contiguous()
    T, dev = int(thr.size), sal.device
    with torch.cuda.device(dev):
        gscale = kth = None
        if salglobal:
            m = np.float32(torch.where(sal >= 0, sal, torch.zeros((), dtype=torch.float32, device=dev)).mean().item() if mean is None else mean)
            gscale = torch.from_numpy((m * thr.astype(np.float32)).astype(np.float32)).to(dev)        # float32(mean32 * float32(t))
        else:
            kth = torch.from_numpy(frame_k(thr).astype(np.int32)).to(dev)
        thr_dev = torch.from_numpy(thr).to(dev)
        counts = torch.empty((T, 2), dtype=torch.int64, device=dev) if truth is not None else None
        scale = torch.empty((n, T), dtype=torch.float32, device=dev)
        hard = torch.empty((n, SIDE, SIDE), dtype=torch.uint8, device=dev) if which >= 0 else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.call("cgs_saliency_sweep", sal.data_ptr(), preds.data_ptr(), ptr(truth), thr_dev.data_ptr(), ptr(gscale), ptr(kth), T, n,
                  SIDE, SIDE, int(which), ptr(counts), scale.data_ptr(), ptr(hard), torch.cuda.current_stream().cuda_stream)
    return counts, scale, hard


def sweep(sal, preds, truth, thresholds, salglobal, mean=None):
    """sal: device float32 [n, 64, 64] or [n, 1, 64, 64], non-negative or NaN; preds: device float32 [n]; truth: torch.bool / uint8 of
    sal's number of elements (non-zero = set); thresholds: 1..1024 finite numbers > 0 in any order, kept in float64 (per-frame mode:
    below 1, as int(4096 * t) indexes the sorted frame).  salglobal as ``-salglobal``: true normalises by
    float32(mean * float32(t)), false by each frame's int(4096 * t)-th smallest value.  ``mean`` (global mode) is the float32 mean of
    the stack's non-negative part; None takes it on the device with torch, whose order of summation is not numpy's: that mean, and
    with it the normaliser, can differ from ``_saliency_post``'s in the last bits.  Pass numpy's ``np.where(sal >= 0, sal, 0.0).mean()``
    of a host copy for counts that are ``_saliency_post``'s exactly (Handler does).
    Returns (inter, union, scale): int64 device [T] as ``metrics.iou_curve`` returns them, in the caller's threshold order, and the
    normaliser used, float32 device [n, T].  Raises ValueError for bad arguments (a negative value in sal among them: one device
    reduction and a synchronisation), CgsError without a GPU: there is no CPU path."""
    if truth is None:
        raise ValueError("sweep scores against truth; post gives the mask without one")
    counts, scale, _unused = _run("saliency.sweep", sal, preds, truth, thresholds, bool(salglobal), mean, -1)
    return counts[:, 0].contiguous(), counts[:, 1].contiguous(), scale


def post(sal, preds, thresh, salglobal, mean=None):
    """The hard mask of ``Handler._saliency_post(sal, preds, thresh, salglobal)`` on the device, arguments as ``sweep``'s.
    Returns (hard uint8 [n, 64, 64] of 0 / 1, scale float32 [n]: the normaliser of each frame)."""
    if np.ndim(thresh) != 0:
        raise ValueError("post takes one threshold; sweep takes a grid")
    _unused, scale, hard = _run("saliency.post", sal, preds, None, [float(thresh)], bool(salglobal), mean, 0)
    return hard, scale[:, 0].contiguous()


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_salience_grid(s):
    """``--salience-grid``: the syntax of ``--thresh-grid`` (dash-separated floats or ``lo:hi:n``).  Returns float64 [T] in the order
    given -- the threshold enters a float64 comparison, so 0.1 stays 0.1 --, 1 <= T <= 1024, every value finite and above 0."""
    s = str(s).strip()
    thr = metrics.parse_grid_values(s, "--salience-grid")
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"--salience-grid {s!r}: 1 to {MAX_THRESHOLDS} thresholds, got {thr.size}")
    if not np.isfinite(thr).all() or (thr <= 0).any():
        raise ValueError(f"--salience-grid {s!r}: every threshold must be a finite number above 0")
    return thr


def sweep_report(thresholds, inter, union, n_truth, salglobal=True):
    """``metrics.curve_report``'s table for a saliency sweep: the same rows with ``thresh`` the float64 threshold unrounded, in
    per-frame mode each row also with ``k`` = int(4096 * thresh).  Returns {"n_truth", "rows", "best": {"index", "thresh", "iou"}}."""
    thr = [float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1)]
    rep = metrics.curve_report(thr, inter, union, n_truth)
    for row, t, k in zip(rep["rows"], thr, frame_k(thr)):
        row["thresh"] = t
        if not salglobal:
            row["k"] = int(k)
    rep["best"]["thresh"] = rep["rows"][rep["best"]["index"]]["thresh"]
    return rep
