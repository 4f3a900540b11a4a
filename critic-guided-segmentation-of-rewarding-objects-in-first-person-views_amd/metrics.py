"""Evaluation scoring on the GPU (csrc/metrics.hip): intersection / union counts of a mask stack against the truth for a whole grid of
thresholds (``iou_curve``, the grid main.py:974-975 left commented out) or of K label stacks (``iou_counts``, the score of the
reference's CRF parameter search, main.py:1253).  The stacks are scored where they are; only the counts (int64) come back.
``parse_thresh_grid`` and ``curve_report`` are pure host helpers for ``-eval --thresh-grid`` (evaluate.py)."""
import math

import numpy as np
import torch

from . import _lib

MAX_THRESHOLDS = 1024


def _flat_u8(t, what):
    if t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what} must be torch.bool or torch.uint8, got {t.dtype}")
    t = t.reshape(-1)
    if not t.is_contiguous():
        t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t        # a bool is one byte, 0 or 1


def _same_device(*tensors):
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all tensors must be on the same device, got " + ", ".join(str(t.device) for t in tensors))


def _need_gpu(name, entry, t):
    if not torch.cuda.is_available() or not t.is_cuda:
        raise _lib.CgsError(f"{name} runs on the GPU ({entry}); " + ("no GPU is visible" if not torch.cuda.is_available() else
                            f"the tensors are on {t.device}") + " and there is no CPU fallback")


def iou_curve(prob, truth, thresholds, inclusive=False):
    """prob: device float32 tensor of any shape; truth: torch.bool / uint8 of as many elements (non-zero = set); thresholds: 1..1024
    numbers in any order (cast to float32).  Returns (inter, union), int64 device tensors [T] in the caller's threshold order:
    inter[t] = #{truth & (prob > thresholds[t])}, union[t] = #{truth | (prob > thresholds[t])} (>= with inclusive), the comparison in
    float32 as numpy's; a NaN in prob is on for no threshold.  No CPU path: raises CgsError without a GPU."""
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1).astype(np.float32)
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} thresholds, got {thr.size}")
    if np.isnan(thr).any():
        raise ValueError("a threshold is NaN")
    if prob.dtype != torch.float32:
        raise ValueError(f"prob must be float32, got {prob.dtype}")
    if prob.numel() != truth.numel() or prob.numel() < 1:
        raise ValueError(f"prob has {prob.numel()} elements, truth {truth.numel()}: they must agree and not be empty")
    _same_device(prob, truth)
    truth = _flat_u8(truth, "truth")
    _need_gpu("iou_curve", "cgs_iou_curve", prob)
    prob = prob.reshape(-1)
    if not prob.is_contiguous():
        prob = prob.contiguous()
    order = np.argsort(thr, kind="stable")
    T = int(thr.size)
    with torch.cuda.device(prob.device):
        thr_dev = torch.from_numpy(thr[order]).to(prob.device)
        counts = torch.empty((T, 2), dtype=torch.int64, device=prob.device)
        _lib.call("cgs_iou_curve", prob.data_ptr(), truth.data_ptr(), thr_dev.data_ptr(), T, int(bool(inclusive)), prob.numel(),
                  counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        back = torch.empty(T, dtype=torch.int64)
        back[torch.from_numpy(order)] = torch.arange(T)                       # row of the sorted result that holds threshold t
        counts = counts[back.to(prob.device)]
    return counts[:, 0].contiguous(), counts[:, 1].contiguous()


def iou_counts(labels, truth):
    """labels: device torch.bool / uint8 (non-zero = on), one stack of truth.numel() elements or K of them ([K, ...]); truth: bool / uint8.
    Returns int64 device [K, 2] = (#{truth & labels_k}, #{truth | labels_k}), or [2] when labels holds a single stack with truth's
    number of dimensions or fewer.  No CPU path: raises CgsError without a GPU."""
    px = truth.numel()
    if px < 1 or labels.numel() < px or labels.numel() % px:
        raise ValueError(f"labels has {labels.numel()} elements, truth {px}: labels must hold one or more whole stacks")
    K = labels.numel() // px
    single = K == 1 and labels.dim() <= truth.dim()
    if K > 1 and (labels.dim() < 1 or labels.shape[0] != K):
        raise ValueError(f"labels {tuple(labels.shape)} must be [K, ...] with truth's {px} elements per stack")
    _same_device(labels, truth)
    labels, truth = _flat_u8(labels, "labels"), _flat_u8(truth, "truth")
    _need_gpu("iou_counts", "cgs_iou_counts", labels)
    with torch.cuda.device(labels.device):
        counts = torch.empty((K, 2), dtype=torch.int64, device=labels.device)
        _lib.call("cgs_iou_counts", labels.data_ptr(), truth.data_ptr(), K, px, counts.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return counts[0] if single else counts


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_grid_values(s, flag):
    """The syntax shared by ``--thresh-grid`` and ``--salience-grid``: dash-separated floats or ``lo:hi:n`` (np.linspace(lo, hi, n)).
    Returns the values as float64 in the order given; ``flag`` names the option in the error."""
    s = str(s).strip()
    try:
        if ":" in s:
            lo, hi, n = s.split(":")
            if int(n) < 1:
                raise ValueError
            return np.linspace(float(lo), float(hi), int(n), dtype=np.float64)
        # a dash separates; a dash after the start, after another dash or after an exponent's e is a sign ("-0.1-0.5", "1e-3-0.5")
        parts, cur = [], ""
        for ch in s:
            if ch == "-" and cur and cur[-1] not in "eE-":
                parts.append(cur)
                cur = ""
            else:
                cur += ch
        parts.append(cur)
        return np.array([float(p) for p in parts], dtype=np.float64)
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected dash-separated numbers (0.01-0.05-0.5) or lo:hi:n") from None


def parse_thresh_grid(s):
    """``"0.01-0.05-0.5"`` (the reference's dash-separated floats, main.py:974) or ``"lo:hi:n"`` (np.linspace(lo, hi, n) in float64).
    Returns float32 [T], 1 <= T <= 1024, in the order given."""
    s = str(s).strip()
    thr = parse_grid_values(s, "--thresh-grid").astype(np.float32)
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"--thresh-grid {s!r}: 1 to {MAX_THRESHOLDS} thresholds, got {thr.size}")
    if np.isnan(thr).any():
        raise ValueError(f"--thresh-grid {s!r}: a threshold is NaN")
    return thr


def ratio(a, b):
    """a / b unrounded, NaN when b is 0."""
    return a / b if b else float("nan")


def best_index(scores):
    """Index of the highest score; ties go to the lowest index, a NaN ranks below every number (0 when all are NaN)."""
    best = 0
    for i, s in enumerate(scores):
        if not math.isnan(s) and (math.isnan(scores[best]) or s > scores[best]):
            best = i
    return best


def curve_report(thresholds, inter, union, n_truth):
    """The per-threshold table of ``-eval --thresh-grid``: for threshold t with tp = inter[t]: fp = union[t] - n_truth (on and not truth),
    fn = n_truth - tp, iou = tp / union, precision = tp / (tp + fp), recall = tp / n_truth (unrounded; NaN for an empty denominator),
    and the best row by iou (best_index).  Returns {"n_truth", "rows": [...], "best": {"index", "thresh", "iou"}}."""
    thr = [float(np.float32(t)) for t in np.asarray(thresholds).reshape(-1)]
    inter, union = [int(x) for x in np.asarray(inter).reshape(-1)], [int(x) for x in np.asarray(union).reshape(-1)]
    n_truth = int(n_truth)
    if not len(thr) == len(inter) == len(union):
        raise ValueError(f"{len(thr)} thresholds, {len(inter)} intersections, {len(union)} unions")
    rows = []
    for t, tp, un in zip(thr, inter, union):
        fp, fn = un - n_truth, n_truth - tp
        if tp < 0 or fp < 0 or fn < 0:
            raise ValueError(f"counts (inter {tp}, union {un}) do not fit {n_truth} truth pixels")
        rows.append({"thresh": t, "tp": tp, "fp": fp, "fn": fn, "iou": ratio(tp, un), "precision": ratio(tp, tp + fp),
                     "recall": ratio(tp, n_truth)})
    b = best_index([r["iou"] for r in rows])
    return {"n_truth": n_truth, "rows": rows, "best": {"index": b, "thresh": rows[b]["thresh"], "iou": rows[b]["iou"]}}
