"""From masks to objects on the GPU (csrc/objects.hip): connected-component labelling of a mask stack where it is, an area filter, the
numbering of ``scipy.ndimage.label`` and a table of the objects (area, bounding box, coordinate sums, first pixel).  Everything is
integer and stays on the device; ``table_rows`` is the host helper that turns a table into the dicts of ``objects.json``
(handler.py: ``-process -objects`` / ``-eval -objects``)."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_SIDE = _lib.OBJ_MAX_SIDE
FIELDS = ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "first")

Objects = namedtuple("Objects", ["labels", "mask", "kept", "found", "table"])


def label(src, thresh=None, inclusive=False, connectivity=8, min_area=1, max_objects=64, want_labels=True, want_mask=False):
    """src: device tensor [n,h,w] or [h,w] (then n = 1), 1 <= h, w <= 64: torch.bool / uint8 (non-zero = on, no thresh), or float32 with
    thresh: on where src > thresh, or src >= thresh with inclusive (compared in float32; a NaN is off).  connectivity 4 or 8; components
    of fewer than min_area pixels are removed; the kept ones are numbered 1..K per frame in raster order of their first pixel.
    Returns Objects(labels int32 [n,h,w] or None, mask bool [n,h,w] or None, kept int32 [n], found int32 [n] (before the filter),
    table int32 [n,max_objects,8]: area, x0, y0, x1, y1, sum_x, sum_y, first; zero rows from min(kept, max_objects) on), all on src's
    device.  labels numbers every kept component, also those beyond max_objects.  No CPU path: raises CgsError without a GPU."""
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
        if thresh is not None:
            raise ValueError(f"thresh is for float32 masks; a {src.dtype} stack is on where it is non-zero")
        kind, thr = _lib.OBJ_U8, 0.0
    elif src.dtype == torch.float32:
        if thresh is None:
            raise ValueError("a float32 stack needs thresh")
        thr = float(thresh)
        if thr != thr:
            raise ValueError("thresh is NaN")
        kind = _lib.OBJ_F32_GE if inclusive else _lib.OBJ_F32_GT
    else:
        raise ValueError(f"src must be torch.bool, uint8 or float32, got {src.dtype}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    min_area, max_objects = _as_int(min_area, "min_area"), _as_int(max_objects, "max_objects")
    if min_area < 1 or max_objects < 1 or max(min_area, max_objects) > 0x7FFFFFFF:
        raise ValueError(f"min_area and max_objects must be at least 1 (and fit 32 bits), got {min_area} and {max_objects}")
    if not torch.cuda.is_available() or not src.is_cuda:
        raise _lib.CgsError("objects.label runs on the GPU (cgs_objects_label); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensor is on {src.device}") + " and there is no CPU fallback")
    if not src.is_contiguous():
        src = src.contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)                                       # a bool is one byte, 0 or 1
    dev = src.device
    with torch.cuda.device(dev):
        labels = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_labels else None
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_mask else None
        count = torch.empty((n, 2), dtype=torch.int32, device=dev)
        table = torch.empty((n, max_objects, len(FIELDS)), dtype=torch.int32, device=dev)
        _lib.call("cgs_objects_label", src.data_ptr(), kind, thr, n, h, w, int(connectivity), min_area, max_objects,
                  labels.data_ptr() if want_labels else None, mask.data_ptr() if want_mask else None, count.data_ptr(),
                  table.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return Objects(labels, mask.view(torch.bool) if want_mask else None, count[:, 0].contiguous(), count[:, 1].contiguous(), table)


def _as_int(v, what):
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{what} must be a whole number, got {v!r}")
    return int(v)


# ---------------------------------------------------------------------------------------------------------------- host helper
def table_rows(table, kept, width=MAX_SIDE):
    """table [n,max_objects,8] and kept [n] (tensors or arrays) -> per frame the list of its first min(kept, max_objects) objects as
    {"label", "area", "bbox": [x0, y0, x1, y1] (inclusive), "centroid": [sum_x / area, sum_y / area], "first": [x, y]}.
    The table stores `first` as the raster index y * width + x: width is the frames' width (the project's masks are 64 wide)."""
    table = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    kept = kept.detach().cpu().numpy() if isinstance(kept, torch.Tensor) else np.asarray(kept)
    kept = kept.reshape(-1)
    if table.ndim != 3 or table.shape[2] != len(FIELDS) or table.shape[0] != kept.shape[0]:
        raise ValueError(f"table {table.shape} must be [n, max_objects, {len(FIELDS)}] with one kept count per frame, got {kept.shape[0]} counts")
    width = int(width)
    if width < 1:
        raise ValueError(f"width must be at least 1, got {width}")
    out = []
    for rows, k in zip(table, kept):
        frame = []
        for i in range(min(int(k), table.shape[1])):
            area, x0, y0, x1, y1, sx, sy, first = (int(v) for v in rows[i])
            frame.append({"label": i + 1, "area": area, "bbox": [x0, y0, x1, y1], "centroid": [sx / area, sy / area],
                          "first": [first % width, first // width]})
        out.append(frame)
    return out
