"""How well a mask's outline follows the truth's, on the GPU (csrc/boundary.hip): per frame the two inner 4-neighbour boundaries, the
exact squared Euclidean distance of every pixel to each, and from them the counts of the boundary F-measure (the video-segmentation
benchmarks' contour accuracy), of boundary IoU (Cheng et al., CVPR 2021) and of the Hausdorff distance.  Everything is integer and
stays on the device; ``tol_squared`` / ``parse_boundary_tol`` / ``boundary_report`` are the pure host helpers of ``-eval
--boundary-tol`` (evaluate.py, eval_boundary.json).

Two conventions differ from other tools: everything outside the frame counts as off, so a mask cut by the frame edge has its boundary
there; and the boundary is the inner boundary (on pixels with an off 4-neighbour), not a ``seg2bmap`` half-pixel map."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib, metrics

MAX_SIDE = _lib.OBJ_MAX_SIDE
MAX_TOL, MAX_TOL_PX = _lib.BOUNDARY_MAX_TOL, _lib.BOUNDARY_MAX_TOL_PX

Boundary = namedtuple("Boundary", ["pred_px", "truth_px", "hd2_pred", "hd2_truth", "hit_pred", "hit_truth", "band_inter", "band_union",
                                   "dist2"])


def _tol_milli(tol):
    """The tolerances as whole thousandths of a pixel; ValueError in the style of ``objects.iou_milli``."""
    try:
        vals = [float(t) for t in tol]
    except TypeError:
        raise ValueError(f"tol must be a sequence of numbers, got {tol!r}") from None
    if not 1 <= len(vals) <= MAX_TOL:
        raise ValueError(f"1 to {MAX_TOL} tolerances, got {len(vals)}")
    out = []
    for t in vals:
        if t != t or abs(t) == float("inf"):
            raise ValueError(f"tolerance {t!r} is not a number")
        m = round(t * 1000)
        if abs(t * 1000 - m) > 1e-3:
            raise ValueError(f"tolerance {t!r} is not a whole number of thousandths")
        if not 0 <= m <= 1000 * MAX_TOL_PX:
            raise ValueError(f"tolerance {t!r} is outside [0, {MAX_TOL_PX}]")
        if m in out:
            raise ValueError(f"tolerance {t!r} is given twice")
        out.append(m)
    return out


def tol_squared(tol):
    """1 to 16 distinct tolerances in pixels, each a whole number of thousandths in [0, 128] -> (round(1000 t))^2 // 1_000_000 in Python
    integers, in the order given.  A squared distance d2 is an integer, so d2 <= t^2 exactly when d2 <= that value (1.415 -> 2, 1.414 ->
    1).  ValueError for an empty list, more than 16, a NaN, an infinity, a value outside the range or off the thousandths, a duplicate."""
    return [m * m // 1_000_000 for m in _tol_milli(tol)]


def score(pred, truth, tol=(1,), thresh=None, inclusive=False, want_dist2=False):
    """pred: device tensor [n,h,w] or [h,w] (then n = 1), 1 <= h, w <= 64: torch.bool / uint8 (non-zero = on, no thresh), or float32 with
    thresh: on where pred > thresh, or pred >= thresh with inclusive (compared in float32; a NaN is off), as ``objects.label`` takes its
    stack.  truth: torch.bool / uint8 of the same shape on the same device.  tol: as ``tol_squared`` takes it.
    A boundary pixel is an on pixel with an off 4-neighbour, the outside of the frame being off.  With d2_pred / d2_truth the squared
    Euclidean distance of a pixel to the nearest predicted / truth boundary pixel and q = tol_squared(tol)[k], returns
    Boundary(pred_px, truth_px int32 [n]: boundary pixels; hd2_pred int32 [n]: the largest d2_truth over the predicted boundary,
    hd2_truth: the other way round, both -1 when either boundary is empty; hit_pred int32 [n,T]: predicted boundary pixels with d2_truth
    <= q, hit_truth; band_inter, band_union int32 [n,T]: #(P & G) and #(P | G) for P = on pixels of pred with d2_pred <= q, G the same
    for the truth (boundary IoU; an empty boundary gives an empty band); dist2 int32 [n,2,h,w] or None: d2_pred and d2_truth, -1
    throughout a plane whose boundary is empty), in the caller's tolerance order, all on the inputs' device.
    No CPU path: raises CgsError without a GPU."""
    for name, t in (("pred", pred), ("truth", truth)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if pred.dim() not in (2, 3) or pred.shape != truth.shape:
        raise ValueError(f"pred and truth must be [n,h,w] or [h,w] and of one shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.dim() == 2:
        pred, truth = pred[None], truth[None]
    n, h, w = (int(s) for s in pred.shape)
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"pred {tuple(pred.shape)}: at least one frame of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    if pred.dtype in (torch.bool, torch.uint8):
        if thresh is not None:
            raise ValueError(f"thresh is for float32 masks; a {pred.dtype} stack is on where it is non-zero")
        kind, thr = _lib.OBJ_U8, 0.0
    elif pred.dtype == torch.float32:
        if thresh is None:
            raise ValueError("a float32 stack needs thresh")
        thr = float(thresh)
        if thr != thr:
            raise ValueError("thresh is NaN")
        kind = _lib.OBJ_F32_GE if inclusive else _lib.OBJ_F32_GT
    else:
        raise ValueError(f"pred must be torch.bool, uint8 or float32, got {pred.dtype}")
    if truth.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"truth must be torch.bool or uint8, got {truth.dtype}")
    q = tol_squared(tol)
    if not torch.cuda.is_available() or not (pred.is_cuda and truth.is_cuda):
        raise _lib.CgsError("boundary.score runs on the GPU (cgs_boundary_score); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensors are on {pred.device} and {truth.device}") + " and there is no CPU fallback")
    if pred.device != truth.device:
        raise ValueError(f"pred and truth are on two devices, {pred.device} and {truth.device}")
    pred, truth = pred.contiguous(), truth.contiguous()
    if pred.dtype == torch.bool:
        pred = pred.view(torch.uint8)                                     # a bool is one byte, 0 or 1
    if truth.dtype == torch.bool:
        truth = truth.view(torch.uint8)
    dev, T = pred.device, len(q)
    with torch.cuda.device(dev):
        tol2 = torch.tensor(q, dtype=torch.int32).to(dev)
        counts = torch.empty((n, 4 + 4 * T), dtype=torch.int32, device=dev)
        dist2 = torch.empty((n, 2, h, w), dtype=torch.int32, device=dev) if want_dist2 else None
        _lib.call("cgs_boundary_score", pred.data_ptr(), kind, thr, truth.data_ptr(), n, h, w, tol2.data_ptr(), T, counts.data_ptr(),
                  dist2.data_ptr() if want_dist2 else None, torch.cuda.current_stream().cuda_stream)
    per = counts[:, 4:].reshape(n, T, 4)
    return Boundary(*(counts[:, i].contiguous() for i in range(4)), *(per[:, :, i].contiguous() for i in range(4)), dist2)


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_boundary_tol(s):
    """``--boundary-tol``: ``"0-1-2-3"`` (dash-separated) or ``"lo:hi:n"`` (np.linspace(lo, hi, n)), as --thresh-grid is written.  Returns
    the tolerances in pixels as floats, whole thousandths, in the order given; ValueError as ``tol_squared``."""
    s = str(s).strip()
    vals = metrics.parse_grid_values(s, "--boundary-tol").tolist()
    try:
        return [m / 1000 for m in _tol_milli(vals)]
    except ValueError as e:
        raise ValueError(f"--boundary-tol {s!r}: {e}") from None


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _f_measure(p, r):
    """2 p r / (p + r); NaN when either is NaN, 0 when both are 0."""
    if math.isnan(p) or math.isnan(r):
        return float("nan")
    return 2 * p * r / (p + r) if p + r else 0.0


def boundary_report(pred_px, truth_px, hd2_pred, hd2_truth, hit_pred, hit_truth, band_inter, band_union, tol):
    """One block of eval_boundary.json from the outputs of ``score`` over a stack (tensors or arrays: four [n], four [n,T]) and the
    tolerances ``score`` was given: {"frames", "pred_px", "truth_px": the sums, "per_tol": per tolerance {"tol", "tol2", "hit_pred",
    "hit_truth", "band_inter", "band_union": the sums, "precision": hit_pred / pred_px, "recall": hit_truth / truth_px, "f": 2 P R /
    (P + R), "boundary_iou": band_inter / band_union -- pooled over the stack as get_iou pools, unrounded, NaN for an empty denominator
    -- "frame_mean_f": the mean of the per-frame F over the frames with pred_px + truth_px > 0, a frame with exactly one empty side
    having F = 0 (NaN without such frames)}, "hausdorff": {"frames": frames where both boundaries exist, "max", "mean": of
    sqrt(max(hd2_pred, hd2_truth)) over them (NaN without any), "one_sided": frames where exactly one boundary is empty}, "best":
    {"index", "tol", "f": the tolerance of the highest pooled F (metrics.best_index), "boundary_iou": {"index", "tol", "value"}: the
    same for boundary IoU, "hausdorff_max", "hausdorff_mean"}}."""
    q = tol_squared(tol)
    tols = [m / 1000 for m in _tol_milli(tol)]
    flat = lambda a: _host(a).reshape(-1).astype(np.int64)
    pp, tp, hp, ht = flat(pred_px), flat(truth_px), flat(hd2_pred), flat(hd2_truth)
    n, T = pp.shape[0], len(q)
    per = [_host(a).astype(np.int64) for a in (hit_pred, hit_truth, band_inter, band_union)]
    if not tp.shape[0] == hp.shape[0] == ht.shape[0] == n or any(a.shape != (n, T) for a in per):
        raise ValueError(f"{n} frames and {T} tolerances need four [n] and four [n,{T}] counts, got " +
                         ", ".join(str(a.shape) for a in (tp, hp, ht, *per)))
    hit_p, hit_t, inter, union = per
    if (min(pp.min(), tp.min(), hit_p.min(), hit_t.min(), inter.min()) < 0 or (hit_p > pp[:, None]).any() or (hit_t > tp[:, None]).any()
            or (inter > union).any()):
        raise ValueError("the hits do not fit the boundary pixel counts, or an intersection is larger than its union")
    sum_p, sum_t = int(pp.sum()), int(tp.sum())
    scored, rows = np.flatnonzero(pp + tp > 0), []
    for k in range(T):
        sp, st, si, su = (int(a[:, k].sum()) for a in per)
        precision, recall = metrics.ratio(sp, sum_p), metrics.ratio(st, sum_t)
        frame_f = [_f_measure(int(hit_p[i, k]) / int(pp[i]), int(hit_t[i, k]) / int(tp[i])) if pp[i] and tp[i] else 0.0 for i in scored]
        rows.append({"tol": tols[k], "tol2": q[k], "hit_pred": sp, "hit_truth": st, "band_inter": si, "band_union": su,
                     "precision": precision, "recall": recall, "f": _f_measure(precision, recall),
                     "boundary_iou": metrics.ratio(si, su), "frame_mean_f": metrics.ratio(math.fsum(frame_f), len(frame_f))})
    both = (pp > 0) & (tp > 0)
    hd2 = np.maximum(hp[both], ht[both])
    if (hd2 < 0).any():
        raise ValueError("a frame with both boundaries has a negative Hausdorff distance")
    hd = np.sqrt(hd2.astype(np.float64))
    hausdorff = {"frames": int(both.sum()), "max": float(hd.max()) if hd.size else float("nan"),
                 "mean": float(hd.mean()) if hd.size else float("nan"), "one_sided": int(((pp > 0) != (tp > 0)).sum())}
    bf, bi = metrics.best_index([r["f"] for r in rows]), metrics.best_index([r["boundary_iou"] for r in rows])
    best = {"index": bf, "tol": rows[bf]["tol"], "f": rows[bf]["f"],
            "boundary_iou": {"index": bi, "tol": rows[bi]["tol"], "value": rows[bi]["boundary_iou"]},
            "hausdorff_max": hausdorff["max"], "hausdorff_mean": hausdorff["mean"]}
    return {"frames": n, "pred_px": sum_p, "truth_px": sum_t, "per_tol": rows, "hausdorff": hausdorff, "best": best}
