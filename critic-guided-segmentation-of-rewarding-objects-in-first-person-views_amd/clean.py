"""Mask clean-up on the GPU (csrc/clean.hip): the standard steps between a soft mask and its objects -- threshold, hysteresis,
morphological opening and closing, filling of small holes -- on a mask stack where it is, one launch, bit for bit reproducible
(cgs_mask_clean, whose header comment in include/cgs_hip.h is the rule).  ``clean`` is the device entry; ``parse_clean`` and
``clean_report`` are the pure host helpers of ``--clean`` and ``--overlay-clean``."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_SIDE = _lib.OBJ_MAX_SIDE
MAX_RADIUS, MAX_FILL = _lib.CLEAN_MAX_RADIUS, _lib.CLEAN_MAX_FILL
SHAPES = {"square": _lib.CLEAN_SQUARE, "cross": _lib.CLEAN_CROSS}
COUNTS = ("on", "after_hyst", "after_open", "after_close", "after_fill", "components_dropped", "holes_found", "holes_filled")
KEYS = ("hyst", "open", "close", "fill", "shape", "conn")

Cleaned = namedtuple("Cleaned", ["mask", "gated", "counts"])


def _whole(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be a whole number {lo}..{hi}, got {v!r}")
    return int(v)


def clean(src, thresh=None, inclusive=False, strong=None, open=0, close=0, fill=0, shape="square", connectivity=8, want_gated=False):
    """src: device tensor [n,h,w] or [h,w] (then n = 1), 1 <= h, w <= 64: torch.bool / uint8 (non-zero = on, no thresh), or float32 with
    thresh: on where src > thresh, or src >= thresh with inclusive (compared in float32; a NaN is off), as ``objects.label`` reads it.
    Then, in this order: strong (float32 sources; a finite number >= thresh) keeps a `connectivity`-connected component of the on pixels
    only when one of its pixels passes the same compare against strong; open and close (radii 0..4, 0: off) with the (2r+1)^2 square
    or, shape="cross", the diamond of radius r, dilation reading outside the frame as off and erosion reading it as on; fill (0..4096,
    0: off) turns on the holes of at most that many pixels, a hole being a component of off pixels at the complementary connectivity
    that does not touch the frame's edge.
    Returns Cleaned(mask bool [n,h,w], gated float32 [n,h,w] or None, counts int32 [n,8] (COUNTS)), all on src's device.  gated
    (want_gated; float32 sources with thresh > 0) is 0 off the mask and, on it, the source value where that passes the threshold and
    thresh elsewhere: ``gated >= thresh`` is the mask.  No CPU path: raises CgsError without a GPU."""
    if not isinstance(src, torch.Tensor):
        raise ValueError(f"src must be a torch tensor, got {type(src).__name__}")
    if src.dim() not in (2, 3):
        raise ValueError(f"src must be [n,h,w] or [h,w], got {tuple(src.shape)}")
    if src.dim() == 2:
        src = src[None]
    n, h, w = (int(s) for s in src.shape)
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"src {tuple(src.shape)}: at least one frame of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    if src.dtype in (torch.bool, torch.uint8):
        if thresh is not None or strong is not None or want_gated:
            raise ValueError(f"thresh, strong and want_gated are for float32 masks; a {src.dtype} stack is on where it is non-zero")
        kind, thr = _lib.OBJ_U8, 0.0
    elif src.dtype == torch.float32:
        if thresh is None:
            raise ValueError("a float32 stack needs thresh")
        thr = float(np.float32(thresh))
        if thr != thr:
            raise ValueError("thresh is NaN")
        kind = _lib.OBJ_F32_GE if inclusive else _lib.OBJ_F32_GT
    else:
        raise ValueError(f"src must be torch.bool, uint8 or float32, got {src.dtype}")
    hyst, strong_v = strong is not None, 0.0
    if hyst:
        strong_v = float(np.float32(strong))
        if not math.isfinite(strong_v) or strong_v < thr:
            raise ValueError(f"strong must be a finite number at or above thresh ({thr!r}), got {strong!r}")
    if want_gated and not thr > 0:
        raise ValueError(f"want_gated needs thresh > 0 (off cells are 0 there), got {thresh!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if shape not in SHAPES:
        raise ValueError(f"shape must be 'square' or 'cross', got {shape!r}")
    open_r, close_r = _whole(open, "open", 0, MAX_RADIUS), _whole(close, "close", 0, MAX_RADIUS)
    fill_area = _whole(fill, "fill", 0, MAX_FILL)
    if not torch.cuda.is_available() or not src.is_cuda:
        raise _lib.CgsError("clean.clean runs on the GPU (cgs_mask_clean); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensor is on {src.device}") + " and there is no CPU fallback")
    if not src.is_contiguous():
        src = src.contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)                                       # a bool is one byte, 0 or 1
    dev = src.device
    with torch.cuda.device(dev):
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        gated = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_gated else None
        counts = torch.empty((n, len(COUNTS)), dtype=torch.int32, device=dev)
        _lib.call("cgs_mask_clean", src.data_ptr(), kind, thr, int(hyst), strong_v, n, h, w, int(connectivity), SHAPES[shape], open_r,
                  close_r, fill_area, mask.data_ptr(), gated.data_ptr() if want_gated else None, counts.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return Cleaned(mask.view(torch.bool), gated, counts)


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_clean(s, flag="--clean"):
    """``"hyst=0.8;open=1;close=2;fill=16;shape=cross;conn=4"``: --crf-grid's KEY=value;... with one value per key, keys in any order.
    hyst: the strong threshold (a finite number), open / close: radii 0..4, fill: the largest hole filled, 0..4096, shape: square |
    cross, conn: 4 | 8.  Returns {"hyst": float or None, "open", "close", "fill": ints, "shape": str, "conn": int} with the defaults
    off, 0, 0, 0, square, 8.  ValueError naming the flag for an unknown or repeated key, an empty item, a non-number, a value out of
    range, or a spec in which no operation is active."""
    spec = {"hyst": None, "open": 0, "close": 0, "fill": 0, "shape": "square", "conn": 8}
    seen = set()
    for item in str(s).split(";"):
        key, eq, val = (t.strip() for t in item.partition("="))
        if not eq or key not in KEYS or not val:
            raise ValueError(f"{flag} {item!r}: expected KEY=value with KEY one of {', '.join(KEYS)}")
        if key in seen:
            raise ValueError(f"{flag}: {key} is given twice")
        seen.add(key)
        if key == "shape":
            if val not in SHAPES:
                raise ValueError(f"{flag} {item!r}: shape is square or cross")
            spec[key] = val
        elif key == "hyst":
            try:
                v = float(val)
            except ValueError:
                raise ValueError(f"{flag} {item!r}: {val!r} is not a number") from None
            if not math.isfinite(v):
                raise ValueError(f"{flag} {item!r}: {val!r} is not finite")
            spec[key] = v
        else:
            try:
                v = int(val)
            except ValueError:
                raise ValueError(f"{flag} {item!r}: {val!r} is not a whole number") from None
            lo, hi = {"open": (0, MAX_RADIUS), "close": (0, MAX_RADIUS), "fill": (0, MAX_FILL), "conn": (4, 8)}[key]
            if not lo <= v <= hi or (key == "conn" and v not in (4, 8)):
                raise ValueError(f"{flag} {item!r}: {key} is " + ("4 or 8" if key == "conn" else f"a whole number {lo}..{hi}"))
            spec[key] = v
    if spec["hyst"] is None and not (spec["open"] or spec["close"] or spec["fill"]):
        raise ValueError(f"{flag} {s!r}: no operation is active (give hyst, open, close or fill)")
    return spec


def spec_text(spec):
    """A parsed spec in its canonical written form (every key, KEYS order; hyst only when given)."""
    return ";".join(f"{k}={spec[k]}" for k in KEYS if spec[k] is not None)


def spec_kwargs(spec):
    """A parsed spec as the keyword arguments of ``clean``."""
    return dict(strong=spec["hyst"], open=spec["open"], close=spec["close"], fill=spec["fill"], shape=spec["shape"],
                connectivity=spec["conn"])


def clean_report(counts, spec):
    """counts: int [n,8] or [8] (tensor or array) of ``clean`` -> the JSON block {"spec": the parsed spec, "frames": n, and the eight
    sums under the names of COUNTS}."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.reshape(-1, len(COUNTS)).astype(np.int64)
    return {"spec": dict(spec), "frames": int(c.shape[0]), **{k: int(v) for k, v in zip(COUNTS, c.sum(axis=0))}}
