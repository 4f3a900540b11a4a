"""From masks to objects on the GPU (csrc/objects.hip): connected-component labelling of a mask stack where it is, an area filter, the
numbering of ``scipy.ndimage.label`` and a table of the objects (area, bounding box, coordinate sums, first pixel).  Everything is
integer and stays on the device; ``table_rows`` is the host helper that turns a table into the dicts of ``objects.json``
(process.py: ``-process -objects``, evaluate.py: ``-eval -objects``).

``match`` (csrc/objects_match.hip) matches the objects of two label stacks frame by frame at a list of IoU thresholds; ``sum_iou`` adds
up the matched pairs' IoU on the device, and ``parse_match_iou`` / ``match_report`` are the pure host helpers of
``-eval -objects --match-iou`` (eval_match.json).

``track`` (csrc/objects_track.hip) follows the objects of one label stack from frame to frame (mutual best partners above an IoU
threshold, chains resolved on the device), ``switches`` counts identity switches of a prediction's tracks against the truth's, and
``parse_track_iou`` / ``natural_order`` / ``track_report`` / ``track_rows`` are the pure host helpers of ``-objects --track-iou``
(eval_tracks.json, tracks.json).  ``TrackStream`` gives ``track``'s numbers to a label stack that arrives in chunks
(``-process --source-video --overlay-tracks``); ``stream_remap`` is its arithmetic.  With ``max_gap`` G > 0 (``--track-gap``,
``--overlay-gap``) both bridge gaps of up to G missing frames (cgs_objects_track_gap), and ``fragments`` counts how often a truth
track is split over several predicted tracks.  With ``motion`` (``--track-motion``, ``--overlay-motion``) the earlier frame's labels
are carried along ``temporal.flow``'s backward block vectors before they are intersected (cgs_objects_track_mc); ``motion_report``
is the block the reports gain.  ``fill`` (csrc/objects_fill.hip, ``--track-fill``) gives the frames that a bridged link jumps over
the mask of the link's tail object, carried there along the same vectors; ``fill_report`` is the block the reports gain.
``FillStream`` gives ``fill``'s result to a label stack that arrives in chunks, G frames behind it (``--overlay-fill``), through
``fill(frames=)``, the frame range of a window (cgs_objects_track_fill_window).  ``appearance`` and ``reid`` (csrc/objects_reid.hip,
``--track-reid``) put an identity layer on top of the tracks: a 64-bin colour histogram per track, and tracks that do not overlap in
time, lie at most ``window`` frames apart and have the same histogram are chained into one identity; ``identities`` gives every object
its identity, and ``parse_track_reid`` / ``parse_track_reid_window`` / ``reid_report`` are the host helpers.  ``ablate``, ``value`` and
``select`` (csrc/objects_value.hip, ``--object-value``) ask the critic about every object: the frame is rebuilt on the device once per
object with that object replaced, the critic's value of each rebuilt frame is taken from the frame's own, and the objects whose drop
fails ``--min-value-drop`` are removed and the rest renumbered; ``value_chunks`` / ``value_keep`` / ``value_report`` and the three
``parse_*`` of its flags are the host helpers."""
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_SIDE = _lib.OBJ_MAX_SIDE
FIELDS = ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "first")
MATCH_MAX_OBJECTS, MATCH_MAX_IOU = _lib.OBJ_MATCH_MAX_OBJECTS, _lib.OBJ_MATCH_MAX_IOU

Objects = namedtuple("Objects", ["labels", "mask", "kept", "found", "table"])
Matches = namedtuple("Matches", ["pred_max", "truth_max", "matched_pred", "matched_truth", "best"])
TRACK_FIELDS = ("first_frame", "first_label", "length", "area_sum", "area_min", "area_max", "inter_sum", "union_sum")
TRACK_MAX_FRAMES = _lib.OBJ_TRACK_MAX_FRAMES
LENGTH_BINS = ("1", "2", "3-4", "5-8", "9-16", "17-32", "33+")             # upper ends 1, 2, 4, 8, 16, 32, then the rest
TRACK_MAX_GAP = _lib.OBJ_TRACK_MAX_GAP
MOTION_SIDE, MOTION_BLOCKS, MOTION_MAX_SEARCH = 64, 64 // _lib.TEMPORAL_BLOCK, _lib.TEMPORAL_MAX_SEARCH      # cgs_objects_track_mc
Tracks = namedtuple("Tracks", ["prev", "track", "n_tracks", "n_links", "n_objects", "longest", "table", "track_labels", "rgb",
                               "gap", "gap_links", "extra"], defaults=(None, None, None))
REID_BINS, REID_MAX_WINDOW, REID_MAX_FRAMES = _lib.OBJ_REID_BINS, _lib.OBJ_REID_MAX_WINDOW, _lib.OBJ_REID_MAX_FRAMES
REID_SIM, REID_WINDOW, REID_MIN_AREA = 0.8, 64, 64          # --track-reid's defaults: judgements, not tuned values
Appearance = namedtuple("Appearance", ["track_hist", "object_hist"])
Reid = namedtuple("Reid", ["prev", "next", "sim", "identity", "signature", "n_identities", "n_links", "n_eligible", "longest"])
VALUE_SIDE, VALUE_MAX_OBJECTS, VALUE_MAX_GROW = _lib.OBJ_VALUE_SIDE, _lib.OBJ_VALUE_MAX_OBJECTS, _lib.OBJ_VALUE_MAX_GROW
VALUE_FILL, VALUE_GROW = "low", 0                         # --object-value's defaults: judgements, not tuned values
Ablated = namedtuple("Ablated", ["images", "row_frame", "row_label", "offsets"])
Values = namedtuple("Values", ["base", "drop", "fill_frame", "rows", "chunks"])
Filled = namedtuple("Filled", ["labels", "track", "age", "table", "n_objects", "n_cells", "n_dropped", "n_vanished", "rgb"])


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


# ---------------------------------------------------------------------------------------------------------------- matching
def iou_milli(iou):
    """A sequence of IoU thresholds as whole thousandths: round(t * 1000) for each.  ValueError for an empty list, more than 16, a value
    that is not within 1e-6 of a thousandth or lies outside [0.5, 1] (below 0.5 a match would not be unique), or a duplicate."""
    try:
        vals = [float(t) for t in iou]
    except TypeError:
        raise ValueError(f"iou must be a sequence of numbers, got {iou!r}") from None
    if not 1 <= len(vals) <= MATCH_MAX_IOU:
        raise ValueError(f"1 to {MATCH_MAX_IOU} IoU thresholds, got {len(vals)}")
    out = []
    for t in vals:
        if t != t or abs(t) == float("inf"):
            raise ValueError(f"IoU threshold {t!r} is not a number")
        m = round(t * 1000)
        if abs(t * 1000 - m) > 1e-3:
            raise ValueError(f"IoU threshold {t!r} is not a whole number of thousandths")
        if not 500 <= m <= 1000:
            raise ValueError(f"IoU threshold {t!r} is outside [0.5, 1]")
        if m in out:
            raise ValueError(f"IoU threshold {t!r} is given twice")
        out.append(m)
    return out


def match(pred_labels, truth_labels, iou=(0.5,), max_objects=64, want_best=True):
    """pred_labels, truth_labels: int32 device tensors [n,h,w] or [h,w] of one shape, 1 <= h, w <= 64, label maps as ``label`` gives
    them (a value <= 0 is background; hand-made maps need not be connected components).  Objects numbered above max_objects (1..64)
    take no part in the matching but show in pred_max / truth_max.  iou: 1..16 distinct thresholds in [0.5, 1], whole thousandths; a
    predicted and a truth object match at t when inter > 0 and inter / union >= t, compared exactly in integers.
    Returns Matches(pred_max int32 [n], truth_max int32 [n] (the largest label of each frame), matched_pred int32 [n,T] (objects
    <= max_objects with at least one match), matched_truth int32 [n,T], best int32 [n,2,max_objects,4] or None: side 0, row p-1 is
    (t, inter, area_p, area_t) of the truth object of largest IoU with p (ties: the smallest t; (0, 0, area_p, 0) without overlap), side
    1, row t-1 is (p, inter, area_t, area_p); zero rows from min(largest label, max_objects) on), all on the inputs' device.
    No CPU path: raises CgsError without a GPU."""
    for name, t in (("pred_labels", pred_labels), ("truth_labels", truth_labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be torch.int32, got {t.dtype}")
    if pred_labels.dim() not in (2, 3) or pred_labels.shape != truth_labels.shape:
        raise ValueError(f"the label maps must be [n,h,w] or [h,w] and of one shape, got {tuple(pred_labels.shape)} and "
                         f"{tuple(truth_labels.shape)}")
    if pred_labels.dim() == 2:
        pred_labels, truth_labels = pred_labels[None], truth_labels[None]
    n, h, w = (int(s) for s in pred_labels.shape)
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"label maps {tuple(pred_labels.shape)}: at least one frame of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    milli = iou_milli(iou)
    max_objects = _as_int(max_objects, "max_objects")
    if not 1 <= max_objects <= MATCH_MAX_OBJECTS:
        raise ValueError(f"max_objects must be 1..{MATCH_MAX_OBJECTS}, got {max_objects}")
    if not torch.cuda.is_available() or not (pred_labels.is_cuda and truth_labels.is_cuda):
        raise _lib.CgsError("objects.match runs on the GPU (cgs_objects_match); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensors are on {pred_labels.device} and {truth_labels.device}") + " and there is no CPU fallback")
    if pred_labels.device != truth_labels.device:
        raise ValueError(f"the label maps are on two devices, {pred_labels.device} and {truth_labels.device}")
    pred_labels, truth_labels = pred_labels.contiguous(), truth_labels.contiguous()
    dev, T = pred_labels.device, len(milli)
    with torch.cuda.device(dev):
        thr = torch.tensor(milli, dtype=torch.int32).to(dev)
        counts = torch.empty((n, 2 + 2 * T), dtype=torch.int32, device=dev)
        best = torch.empty((n, 2, max_objects, 4), dtype=torch.int32, device=dev) if want_best else None
        _lib.call("cgs_objects_match", pred_labels.data_ptr(), truth_labels.data_ptr(), n, h, w, max_objects, thr.data_ptr(), T,
                  counts.data_ptr(), best.data_ptr() if want_best else None, torch.cuda.current_stream().cuda_stream)
    pairs = counts[:, 2:].reshape(n, T, 2)
    return Matches(counts[:, 0].contiguous(), counts[:, 1].contiguous(), pairs[:, :, 0].contiguous(), pairs[:, :, 1].contiguous(), best)


def sum_iou(best, iou):
    """best: Matches.best [n,2,K,4] (a tensor, on any device).  float64 [T] on its device: for each threshold the sum, over the predicted
    objects whose best IoU reaches it, of that IoU (the numerator of panoptic quality).  The compare is the kernel's, in integers."""
    milli = torch.tensor(iou_milli(iou), dtype=torch.int64, device=best.device)
    rows = best[:, 0].reshape(-1, 4).to(torch.int64)
    inter, union = rows[:, 1], rows[:, 2] + rows[:, 3] - rows[:, 1]
    value = inter.double() / union.clamp(min=1).double()                 # a row without overlap has inter = 0: it adds nothing
    reach = (inter[None] > 0) & (1000 * inter[None] >= milli[:, None] * union[None])
    return (value[None] * reach).sum(dim=1)


# ---------------------------------------------------------------------------------------------------------------- tracking
def _track_milli(iou):
    """One link threshold in (0, 1] as whole thousandths; ValueError in the style of ``iou_milli``."""
    if isinstance(iou, bool) or not isinstance(iou, (int, float, np.integer, np.floating)):
        raise ValueError(f"the track IoU must be one number, got {iou!r}")
    t = float(iou)
    if t != t or abs(t) == float("inf"):
        raise ValueError(f"track IoU {t!r} is not a number")
    m = round(t * 1000)
    if abs(t * 1000 - m) > 1e-3:
        raise ValueError(f"track IoU {t!r} is not a whole number of thousandths")
    if not 1 <= m <= 1000:
        raise ValueError(f"track IoU {t!r} is outside (0, 1]")
    return m


def _max_gap(max_gap):
    max_gap = _as_int(max_gap, "max_gap")
    if not 0 <= max_gap <= TRACK_MAX_GAP:
        raise ValueError(f"max_gap must be 0..{TRACK_MAX_GAP}, got {max_gap}")
    return max_gap


def _motion_field(motion, n, device):
    """``track``'s motion argument as the int8 [n - 1,8,8,2] backward field on the labels' device; ValueError otherwise."""
    if isinstance(motion, (tuple, list)):
        if len(motion) != 2:
            raise ValueError(f"motion must be the bwd tensor or the (fwd, bwd) pair of temporal.flow, got {len(motion)} items")
        motion = motion[1]
    if not isinstance(motion, torch.Tensor) or motion.dtype != torch.int8:
        raise ValueError("motion must be an int8 tensor [n - 1,8,8,2] (temporal.flow's bwd), got "
                         + (f"{motion.dtype}" if isinstance(motion, torch.Tensor) else type(motion).__name__))
    if tuple(motion.shape) != (n - 1, MOTION_BLOCKS, MOTION_BLOCKS, 2):
        raise ValueError(f"motion {tuple(motion.shape)}: {n} frames need [{n - 1},{MOTION_BLOCKS},{MOTION_BLOCKS},2]")
    if motion.device != device:
        raise ValueError(f"motion is on {motion.device}, the labels on {device}")
    return motion.contiguous()


def track(labels, iou=0.5, max_objects=64, max_tracks=None, want_labels=False, want_rgb=False, max_gap=0, motion=None):
    """labels: int32 device tensor [n,h,w] or [h,w] (then n = 1), 1 <= h, w <= 64, n <= 2^17, a label stack as ``label`` gives it
    (hand-made maps allowed; views are made contiguous).  An object of frame f is a label in 1..max_objects (at most 64) with a pixel
    in f.  Objects p of f and q of f + 1 are linked when each is the other's best partner (``match``'s `best`: largest IoU, ties to the
    smallest number) and inter / union >= iou, compared in integers; iou is one number in (0, 1], whole thousandths -- mutual best keeps
    links one-to-one below 0.5 too.  A track is a maximal chain of links; tracks are numbered from 1 by their first frame, then label.
    Returns Tracks(prev int32 [n,K]: the label in f - 1 that object l of f continues (0: none), track int32 [n,K]: the track number (0:
    no object), n_tracks, n_links, n_objects, longest: int32 scalars ON THE DEVICE (no synchronisation here; int() them), table int32
    [max_tracks,8]: first_frame, first_label, length, area_sum, area_min, area_max, inter_sum, union_sum per track (the last two over
    its links), zero rows from min(n_tracks, max_tracks) on; max_tracks defaults to n * max_objects, which holds every track;
    track_labels int32 [n,h,w] or None: per pixel its object's track, rgb uint8 [n,h,w,3] or None: a colour per track, black where
    there is none).  No CPU path: raises CgsError without a GPU.
    max_gap G in 0..8: 0 is the above (cgs_objects_track).  G > 0 bridges up to G missing frames (cgs_objects_track_gap, whose header
    comment defines the level order): prev then names the label in frame f - gap, longest is the longest span in frames, and the tuple
    also holds gap int32 [n,K] (0 no link, 1 adjacent, g bridged over g - 1 frames), gap_links int32 [G + 1] (links of gap g at g - 1)
    and extra int32 [max_tracks,2] (bridges, missed per track; span = length + missed); the three are None at G = 0.
    motion: ``temporal.flow``'s bwd (int8 [n - 1,8,8,2] on the labels' device) or its (fwd, bwd) pair; the stack must be 64 x 64.  Frame
    a's labels are then gathered along the chain of block vectors from f back to a before they are intersected with frame f's, at
    every level, and the union counts the carried area (cgs_objects_track_mc, whose header comment in include/cgs_hip.h is the rule).
    The result always carries gap, gap_links and extra; an all-zero field gives the result without motion bit for bit."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"labels must be a torch tensor, got {type(labels).__name__}")
    if labels.dtype != torch.int32:
        raise ValueError(f"labels must be torch.int32, got {labels.dtype}")
    if labels.dim() not in (2, 3):
        raise ValueError(f"labels must be [n,h,w] or [h,w], got {tuple(labels.shape)}")
    max_gap = _max_gap(max_gap)
    if labels.dim() == 2:
        labels = labels[None]
    n, h, w = (int(s) for s in labels.shape)
    if not 1 <= n <= TRACK_MAX_FRAMES or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"labels {tuple(labels.shape)}: 1..{TRACK_MAX_FRAMES} frames of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    milli = _track_milli(iou)
    if motion is not None:
        if (h, w) != (MOTION_SIDE, MOTION_SIDE):
            raise ValueError(f"labels {tuple(labels.shape)}: motion needs frames of {MOTION_SIDE} x {MOTION_SIDE} (8 x 8 blocks of 8 cells)")
        motion = _motion_field(motion, n, labels.device)
    max_objects = _as_int(max_objects, "max_objects")
    if not 1 <= max_objects <= MATCH_MAX_OBJECTS:
        raise ValueError(f"max_objects must be 1..{MATCH_MAX_OBJECTS}, got {max_objects}")
    max_tracks = n * max_objects if max_tracks is None else _as_int(max_tracks, "max_tracks")
    if not 1 <= max_tracks <= 0x7FFFFFFF // len(TRACK_FIELDS):
        raise ValueError(f"max_tracks must be at least 1 (and its table fit 32-bit indices), got {max_tracks}")
    if not torch.cuda.is_available() or not labels.is_cuda:
        raise _lib.CgsError("objects.track runs on the GPU (cgs_objects_track); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensor is on {labels.device}") + " and there is no CPU fallback")
    labels = labels.contiguous()
    dev, K = labels.device, max_objects
    with torch.cuda.device(dev):
        need = int(_lib.load().cgs_objects_track_gap_scratch_bytes(n, K, max_gap) if max_gap or motion is not None else
                   _lib.load().cgs_objects_track_scratch_bytes(n, K))       # (the motion entry's scratch is the gap entry's)
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        prev = torch.empty((n, K), dtype=torch.int32, device=dev)
        trk = torch.empty((n, K), dtype=torch.int32, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        table = torch.empty((max_tracks, len(TRACK_FIELDS)), dtype=torch.int32, device=dev)
        painted = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_labels else None
        rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if want_rgb else None
        if max_gap or motion is not None:
            gap = torch.empty((n, K), dtype=torch.int32, device=dev)
            gap_links = torch.empty(max_gap + 1, dtype=torch.int32, device=dev)
            extra = torch.empty((max_tracks, 2), dtype=torch.int32, device=dev)
            outs = (max_tracks, prev.data_ptr(), gap.data_ptr(), trk.data_ptr(), totals.data_ptr(), gap_links.data_ptr(), table.data_ptr(),
                    extra.data_ptr(), painted.data_ptr() if want_labels else None, rgb.data_ptr() if want_rgb else None, scratch.data_ptr(),
                    scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
            if motion is not None:
                _lib.call("cgs_objects_track_mc", labels.data_ptr(), motion.data_ptr() if n > 1 else None, n, h, w, K, milli, max_gap, *outs)
            else:
                _lib.call("cgs_objects_track_gap", labels.data_ptr(), n, h, w, K, milli, max_gap, *outs)
            return Tracks(prev, trk, totals[0], totals[1], totals[2], totals[3], table, painted, rgb, gap, gap_links, extra)
        _lib.call("cgs_objects_track", labels.data_ptr(), n, h, w, K, milli, max_tracks, prev.data_ptr(), trk.data_ptr(),
                  totals.data_ptr(), table.data_ptr(), painted.data_ptr() if want_labels else None, rgb.data_ptr() if want_rgb else None,
                  scratch.data_ptr(), scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
    return Tracks(prev, trk, totals[0], totals[1], totals[2], totals[3], table, painted, rgb)


def track_colours(track_numbers):
    """``track``'s colour of every track number (any integer tensor): uint8 [..., 3], black for 0, else with hsh = (uint32) t *
    2654435761 channel c is 64 + ((hsh >> 8 c) & 255) * 191 / 255 -- the formula of cgs_objects_track's rgb, in torch."""
    t = track_numbers.to(torch.int64) & 0xFFFFFFFF
    hsh = (t * 2654435761) & 0xFFFFFFFF
    rgb = torch.stack([64 + ((hsh >> (8 * c)) & 255) * 191 // 255 for c in range(3)], dim=-1)
    return torch.where((t != 0)[..., None], rgb, torch.zeros_like(rgb)).to(torch.uint8)


def _frame_range(frames, n):
    """``fill``'s frames argument as (f0, f1) with 0 <= f0 <= f1 <= n; ValueError otherwise."""
    if not isinstance(frames, (tuple, list)) or len(frames) != 2:
        raise ValueError(f"frames must be None or a pair (f0, f1), got {frames!r}")
    f0, f1 = _as_int(frames[0], "frames[0]"), _as_int(frames[1], "frames[1]")
    if not 0 <= f0 <= f1 <= n:
        raise ValueError(f"frames ({f0}, {f1}): 0 <= f0 <= f1 <= {n} (the stack's frames)")
    return f0, f1


def fill(labels, tracks, motion=None, max_objects=64, want_table=True, want_rgb=False, frames=None):
    """The masks that the bridged links of ``track`` jump over (cgs_objects_track_fill, whose header comment in include/cgs_hip.h is
    the rule).  labels: the int32 device stack [n,h,w] that was tracked; tracks: ``track``'s result for it with max_gap G >= 1 and the
    same max_objects (G is len(tracks.gap_links) - 1; a result without gap raises ValueError); motion: as in ``track``, and the field
    the tracks were made with (None: none).  For every frame between the two ends of a link of gap >= 2 the link's tail object is
    carried there along the backward vectors, and the cells it lands on that hold no object become a new object of that frame, numbered
    behind the frame's largest label; a new object that would be numbered above max_objects is dropped.
    Returns Filled(labels int32 [n,h,w]: the input where nothing was written, track int32 [n,K]: the track of every object, new ones
    included, age int32 [n,K]: for a new object the number of frames its mask was carried over, else 0, table int32 [n,K,8] or None:
    ``label``'s row of every new object, zero elsewhere, n_objects, n_cells, n_dropped, n_vanished: int32 scalars ON THE DEVICE (new
    objects, their cells, candidates dropped for want of a label, candidates that reached no free cell), rgb uint8 [n,h,w,3] or None:
    ``track``'s colour per track over the filled labels).  Nothing here synchronises.  No CPU path: raises CgsError without a GPU.
    frames: None, or (f0, f1) with 0 <= f0 <= f1 <= n: only the frames f0 <= m < f1 are filled (cgs_objects_track_fill_window) -- the
    results then hold f1 - f0 frames, frame m at m - f0, and the four counts are sums over those frames; every frame still sees the whole
    stack around it, so (0, n) is the result of None bit for bit.  ``FillStream`` calls it so.
    Limits: the mask comes from the tail alone, moved by whole cells, block by block; cells that hold an object are never written."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"labels must be a torch tensor, got {type(labels).__name__}")
    if labels.dtype != torch.int32:
        raise ValueError(f"labels must be torch.int32, got {labels.dtype}")
    if labels.dim() not in (2, 3):
        raise ValueError(f"labels must be [n,h,w] or [h,w], got {tuple(labels.shape)}")
    if labels.dim() == 2:
        labels = labels[None]
    n, h, w = (int(s) for s in labels.shape)
    if not 1 <= n <= TRACK_MAX_FRAMES or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"labels {tuple(labels.shape)}: 1..{TRACK_MAX_FRAMES} frames of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    max_objects = _as_int(max_objects, "max_objects")
    if not 1 <= max_objects <= MATCH_MAX_OBJECTS:
        raise ValueError(f"max_objects must be 1..{MATCH_MAX_OBJECTS}, got {max_objects}")
    if not isinstance(tracks, Tracks):
        raise ValueError(f"tracks must be the result of objects.track, got {type(tracks).__name__}")
    if tracks.gap is None or tracks.gap_links is None:
        raise ValueError("tracks without gap: fill needs the result of objects.track with max_gap >= 1")
    G = int(tracks.gap_links.shape[0]) - 1
    if not 1 <= G <= TRACK_MAX_GAP:
        raise ValueError(f"tracks made with max_gap {G}: fill needs 1..{TRACK_MAX_GAP} (without a bridged link there is nothing to fill)")
    for name, t in (("prev", tracks.prev), ("gap", tracks.gap), ("track", tracks.track)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n, max_objects):
            raise ValueError(f"tracks.{name} must be int32 [{n},{max_objects}] (the labels' frames, max_objects), got "
                             + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != labels.device:
            raise ValueError(f"tracks.{name} is on {t.device}, the labels on {labels.device}")
    if motion is not None:
        if (h, w) != (MOTION_SIDE, MOTION_SIDE):
            raise ValueError(f"labels {tuple(labels.shape)}: motion needs frames of {MOTION_SIDE} x {MOTION_SIDE} (8 x 8 blocks of 8 cells)")
        motion = _motion_field(motion, n, labels.device)
    if frames is not None:
        f0, f1 = _frame_range(frames, n)
    if not torch.cuda.is_available() or not labels.is_cuda:
        raise _lib.CgsError("objects.fill runs on the GPU (cgs_objects_track_fill); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensor is on {labels.device}") + " and there is no CPU fallback")
    labels = labels.contiguous()
    prev, gap, trk = tracks.prev.contiguous(), tracks.gap.contiguous(), tracks.track.contiguous()
    dev, K = labels.device, max_objects
    with torch.cuda.device(dev):
        m, rows = (n, n) if frames is None else (f1 - f0, max(f1 - f0, 1))       # (an empty range still hands the entry real buffers)
        out = torch.empty((rows, h, w), dtype=torch.int32, device=dev)
        out_track = torch.empty((rows, K), dtype=torch.int32, device=dev)
        age = torch.empty((rows, K), dtype=torch.int32, device=dev)
        table = torch.empty((rows, K, len(FIELDS)), dtype=torch.int32, device=dev) if want_table else None
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        field = motion.data_ptr() if motion is not None and n > 1 else None
        if frames is None:
            _lib.call("cgs_objects_track_fill", labels.data_ptr(), field, n, h, w, K, G,
                      prev.data_ptr(), gap.data_ptr(), trk.data_ptr(), out.data_ptr(), out_track.data_ptr(), age.data_ptr(),
                      table.data_ptr() if want_table else None, totals.data_ptr(), torch.cuda.current_stream().cuda_stream)
        else:
            _lib.call("cgs_objects_track_fill_window", labels.data_ptr(), field, n, h, w, K, G, prev.data_ptr(), gap.data_ptr(),
                      trk.data_ptr(), f0, f1, out.data_ptr(), out_track.data_ptr(), age.data_ptr(),
                      table.data_ptr() if want_table else None, totals.data_ptr(), torch.cuda.current_stream().cuda_stream)
            out, out_track, age, table, n = out[:m], out_track[:m], age[:m], table[:m] if want_table else None, m
        rgb = None
        if want_rgb:
            inside = (out >= 1) & (out <= K)
            number = torch.gather(out_track, 1, (out.reshape(n, -1).to(torch.int64) - 1).clamp(0, K - 1)).reshape(n, h, w)
            rgb = track_colours(torch.where(inside, number, torch.zeros_like(number)))
    return Filled(out, out_track, age, table, totals[0], totals[1], totals[2], totals[3], rgb)


def appearance(frames, labels, tracks=None, max_objects=64, want_objects=False):
    """The colour histograms of cgs_objects_appearance (its header comment in include/cgs_hip.h is the rule).  frames: uint8 device
    tensor [n,h,w,3], the frames the labels were made from; labels: int32 [n,h,w] on the same device, 1 <= h, w <= 64, n <= 2^14;
    tracks: ``track``'s result for these labels with the same max_objects, or None.  A pixel's bin is ((R >> 6) << 4) | ((G >> 6) << 2)
    | (B >> 6), 64 bins.  Returns Appearance(track_hist int32 [max_tracks,64] (max_tracks: the rows of tracks.table): per track the
    pixels of its objects by bin, None without tracks; object_hist int32 [n,K,64]: the same per object, None unless want_objects or
    tracks is None).  Nothing here synchronises.  No CPU path: raises CgsError without a GPU."""
    for name, t, dtype in (("frames", frames, torch.uint8), ("labels", labels, torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if labels.dim() != 3 or frames.dim() != 4 or tuple(frames.shape) != tuple(labels.shape) + (3,):
        raise ValueError(f"labels must be [n,h,w] and frames [n,h,w,3], got {tuple(labels.shape)} and {tuple(frames.shape)}")
    n, h, w = (int(s) for s in labels.shape)
    if not 1 <= n <= REID_MAX_FRAMES or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"labels {tuple(labels.shape)}: 1..{REID_MAX_FRAMES} frames of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels")
    max_objects = _as_int(max_objects, "max_objects")
    if not 1 <= max_objects <= MATCH_MAX_OBJECTS:
        raise ValueError(f"max_objects must be 1..{MATCH_MAX_OBJECTS}, got {max_objects}")
    if frames.device != labels.device:
        raise ValueError(f"frames are on {frames.device}, the labels on {labels.device}")
    if tracks is not None:
        if not isinstance(tracks, Tracks):
            raise ValueError(f"tracks must be the result of objects.track or None, got {type(tracks).__name__}")
        t = tracks.track
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n, max_objects):
            raise ValueError(f"tracks.track must be int32 [{n},{max_objects}] (the labels' frames, max_objects), got "
                             + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != labels.device:
            raise ValueError(f"tracks.track is on {t.device}, the labels on {labels.device}")
    if not torch.cuda.is_available() or not labels.is_cuda:
        raise _lib.CgsError("objects.appearance runs on the GPU (cgs_objects_appearance); " + ("no GPU is visible" if not
                            torch.cuda.is_available() else f"the tensors are on {labels.device}") + " and there is no CPU fallback")
    frames, labels = frames.contiguous(), labels.contiguous()
    dev, K = labels.device, max_objects
    want_objects = bool(want_objects) or tracks is None
    with torch.cuda.device(dev):
        rows = int(tracks.table.shape[0]) if tracks is not None else 0
        trk = tracks.track.contiguous() if tracks is not None else None
        S = torch.empty((rows, REID_BINS), dtype=torch.int32, device=dev) if tracks is not None else None
        H = torch.empty((n, K, REID_BINS), dtype=torch.int32, device=dev) if want_objects else None
        _lib.call("cgs_objects_appearance", frames.data_ptr(), labels.data_ptr(), trk.data_ptr() if trk is not None else None, n, h, w, K,
                  rows, S.data_ptr() if S is not None else None, H.data_ptr() if H is not None else None,
                  torch.cuda.current_stream().cuda_stream)
    return Appearance(S, H)


def _reid_milli(sim):
    """``reid``'s similarity threshold in (0, 1] as whole thousandths; ValueError in the style of ``_track_milli``."""
    try:
        return _track_milli(sim)
    except ValueError as e:
        raise ValueError(str(e).replace("track IoU", "re-identification similarity")) from None


def _reid_window(window):
    window = _as_int(window, "window")
    if not 1 <= window <= REID_MAX_WINDOW:
        raise ValueError(f"window must be 1..{REID_MAX_WINDOW}, got {window}")
    return window


def reid(tracks, appearance, n_frames, sim=REID_SIM, window=REID_WINDOW, min_area=REID_MIN_AREA):
    """Tracks chained into identities by colour (cgs_objects_reid, whose header comment in include/cgs_hip.h is the rule).  tracks:
    ``track``'s result for a stack of n_frames frames, with the full table (max_tracks >= n_frames * max_objects: a truncated table
    cannot be re-identified); appearance: ``appearance``'s result for the same tracks.  A track is eligible with at least min_area
    pixels over its life; its signature is its histogram scaled to 4096.  Eligible tracks t, u with last(t) < first(u) <= last(t) +
    window are linked when each is the other's best partner by histogram intersection and the intersection reaches sim (whole
    thousandths in (0, 1]) of the smaller signature sum, in integers.  An identity is a maximal chain of links.
    Returns Reid(prev, next int32 [max_tracks]: the track linked before / behind track t at t - 1, 0 for none; sim int32 [max_tracks]:
    the intersection of the link to prev; identity int32 [max_tracks]: numbered from 1 by their first track, zero from n_tracks on;
    signature int16 [max_tracks,64]; n_identities, n_links, n_eligible, longest: int32 scalars ON THE DEVICE (no synchronisation here;
    longest is the most tracks in one identity)).  The defaults 0.8 / 64 / 64 are judgements, not tuned values.  No CPU path."""
    if not isinstance(tracks, Tracks):
        raise ValueError(f"tracks must be the result of objects.track, got {type(tracks).__name__}")
    if not isinstance(appearance, Appearance) or not isinstance(appearance.track_hist, torch.Tensor):
        raise ValueError("appearance must be the result of objects.appearance with tracks (its track_hist is needed)")
    n = _as_int(n_frames, "n_frames")
    if not 1 <= n <= REID_MAX_FRAMES:
        raise ValueError(f"n_frames must be 1..{REID_MAX_FRAMES}, got {n}")
    table, trk, S = tracks.table, tracks.track, appearance.track_hist
    if not isinstance(trk, torch.Tensor) or trk.dim() != 2 or int(trk.shape[0]) != n:
        raise ValueError(f"tracks.track must be [{n},K] (n_frames rows), got "
                         + (f"{tuple(trk.shape)}" if isinstance(trk, torch.Tensor) else type(trk).__name__))
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != len(TRACK_FIELDS):
        raise ValueError(f"tracks.table must be int32 [max_tracks,{len(TRACK_FIELDS)}]")
    rows, K = int(table.shape[0]), int(trk.shape[1])
    if rows < n * K:
        raise ValueError(f"tracks.table has {rows} rows, {n} frames of {K} objects need {n * K}: a truncated table cannot be re-identified "
                         "(track with max_tracks=None)")
    if S.dtype != torch.int32 or tuple(S.shape) != (rows, REID_BINS):
        raise ValueError(f"appearance.track_hist must be int32 [{rows},{REID_BINS}] (the table's rows), got {S.dtype} {tuple(S.shape)}")
    extra = tracks.extra
    if extra is not None and (not isinstance(extra, torch.Tensor) or extra.dtype != torch.int32 or tuple(extra.shape) != (rows, 2)):
        raise ValueError(f"tracks.extra must be int32 [{rows},2] or None")
    milli, window = _reid_milli(sim), _reid_window(window)
    min_area = _as_int(min_area, "min_area")
    if not 1 <= min_area <= 0x7FFFFFFF:
        raise ValueError(f"min_area must be at least 1 (and fit 32 bits), got {min_area}")
    if not torch.cuda.is_available() or not table.is_cuda:
        raise _lib.CgsError("objects.reid runs on the GPU (cgs_objects_reid); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the table is on {table.device}") + " and there is no CPU fallback")
    dev = table.device
    for name, t in (("appearance.track_hist", S), ("tracks.n_tracks", tracks.n_tracks), ("tracks.extra", extra)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the table on {dev}")
    table, S = table.contiguous(), S.contiguous()
    extra = extra.contiguous() if extra is not None else None
    with torch.cuda.device(dev):
        n_tracks = tracks.n_tracks.reshape(1).to(torch.int32).contiguous()
        need = int(_lib.load().cgs_objects_reid_scratch_bytes(n, rows))
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        out = torch.empty((4, rows), dtype=torch.int32, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        Q = torch.empty((rows, REID_BINS), dtype=torch.int16, device=dev)
        _lib.call("cgs_objects_reid", S.data_ptr(), table.data_ptr(), extra.data_ptr() if extra is not None else None, n_tracks.data_ptr(),
                  n, rows, milli, window, min_area, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                  totals.data_ptr(), Q.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
    return Reid(out[0], out[1], out[2], out[3], Q, totals[0], totals[1], totals[2], totals[3])


def identities(track, identity):
    """The identity of every object: track int [n,K] (``Tracks.track`` or ``Filled.track``, so a carried object gets its track's
    identity), identity int [max_tracks] (``Reid.identity``), on one device.  int32 [n,K], 0 where there is no object or the track
    number lies beyond the table.  A gather in torch, no synchronisation."""
    if not isinstance(track, torch.Tensor) or track.dim() != 2 or not isinstance(identity, torch.Tensor) or identity.dim() != 1:
        raise ValueError("track must be a tensor [n,K] and identity a tensor [max_tracks]")
    if track.device != identity.device:
        raise ValueError(f"track is on {track.device}, identity on {identity.device}")
    t = track.to(torch.int64)
    rows = int(identity.shape[0])
    inside = (t >= 1) & (t <= rows)
    if rows == 0:
        return torch.zeros_like(track, dtype=torch.int32)
    got = identity.to(torch.int32)[(t - 1).clamp(0, rows - 1)]
    return torch.where(inside, got, torch.zeros_like(got))


def stream_remap(local, carried_local, carried_global, c0, n_tracks):
    """The track numbers of a chunk tracked behind one carried frame, as numbers of the whole stream.  local: int [m,K], rows 1.. of
    ``track(cat(carry, chunk)).track``; carried_local: int [K], its row 0 (every object of the carried frame heads a track there, so
    these are 1..c0 in label order); carried_global: int [K], the carried frame's numbers in the stream; c0: the carried frame's object
    count; n_tracks: the stream's tracks before this chunk (both scalars, tensors or ints).  A local number t of a carried object maps
    to that object's number, every other t to n_tracks + (t - c0) -- heads are numbered by frame, then label, in both -- and 0 to 0.
    Returns int64 [m,K].  torch gather / scatter on the tensors' device, no synchronisation.
    Behind c carried frames (``TrackStream`` with max_gap = c - 1): carried_local and carried_global are [c,K], rows c.. are local and
    c0 is the number of local tracks whose first frame is carried (they are 1..c0, and each holds a carried object).  Links inside
    the carried frames are the stream's own, so carried objects that share a local number share their stream number."""
    local, carried_local = local.to(torch.int64), carried_local.to(torch.int64).reshape(-1)
    size = local.shape[0] * local.shape[1] + carried_local.shape[0] + 1           # more than the largest local number
    lut = torch.arange(size, dtype=torch.int64, device=local.device) - c0 + n_tracks
    lut.scatter_(0, carried_local, carried_global.to(torch.int64).reshape(-1))    # (an absent object writes 0 at 0)
    lut[0] = 0
    return lut[local]


class TrackStream:
    """``track`` for a label stack that comes in chunks: for every split of a stack, the concatenated results of ``push`` are
    ``track(stack, iou, max_objects).track`` bit for bit.  A link depends on its two frames only and tracks are numbered by their first
    frame, then label, so the last frame of a chunk (its labels and its numbers) is all that the next chunk needs.  ``n_tracks`` is the
    number of tracks so far, an int32 scalar on the device (0 before the first push); nothing here synchronises with the host.
    With max_gap = G > 0 a link (f - g -> f), g <= G + 1, depends on the frames f - g .. f only, so the last G + 1 frames pushed are
    carried (fewer while the stream is shorter than that): G frames are not enough, a chunk's first frame may reach G + 1 back.
    With motion=True every push also takes the frames' backward block vectors and the results are those of ``track(stack,
    motion=bwd)``: a link (a -> f) depends on the frames a and f and the vectors bwd[a .. f - 1] only, so the stream carries each
    carried frame's vector (the one to the frame before it) beside its labels."""

    def __init__(self, iou, max_objects=64, max_gap=0, motion=False):
        self.milli = _track_milli(iou)
        self.iou = self.milli / 1000
        self.max_objects = _as_int(max_objects, "max_objects")
        if not 1 <= self.max_objects <= MATCH_MAX_OBJECTS:
            raise ValueError(f"max_objects must be 1..{MATCH_MAX_OBJECTS}, got {max_objects}")
        self.max_gap = _max_gap(max_gap)
        self.motion = bool(motion)
        self.n_tracks = 0
        self._carry = None                     # (labels [c,h,w], numbers int32 [c,K]) of the last c <= max_gap + 1 frames pushed
        self._vectors = None                   # motion: int8 [c,8,8,2], row j from carried frame j to the frame before it

    def push(self, labels, bwd=None):
        """labels: int32 device tensor [m,h,w], m >= 1, of the shape and on the device of the first push, m + 1 <= 2^17.  Returns int32
        [m,K]: the track number in the whole stream of every object, 0 where there is none.
        bwd (with motion=True, and only then): int8 [m,8,8,2] on the labels' device, row i the vectors from pushed frame i to the
        frame before it in the stream (``temporal.flow``'s bwd of the stream, one row late); row 0 of the first push is ignored."""
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.dim() != 3 or labels.shape[0] < 1:
            raise ValueError("labels must be an int32 tensor [m,h,w] with at least one frame, got "
                             + (f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__))
        m = int(labels.shape[0])
        keep = self.max_gap + 1
        if (bwd is not None) != self.motion:
            raise ValueError("bwd goes with TrackStream(motion=True), and every push of such a stream needs it")
        if self.motion:
            if not isinstance(bwd, torch.Tensor) or bwd.dtype != torch.int8 or tuple(bwd.shape) != (m, MOTION_BLOCKS, MOTION_BLOCKS, 2) \
                    or bwd.device != labels.device:
                raise ValueError(f"bwd must be an int8 tensor [{m},{MOTION_BLOCKS},{MOTION_BLOCKS},2] on {labels.device}, got "
                                 + (f"{bwd.dtype} {tuple(bwd.shape)} on {bwd.device}" if isinstance(bwd, torch.Tensor) else type(bwd).__name__))
        if m + keep > TRACK_MAX_FRAMES:
            raise ValueError(f"a chunk of {m} frames: with the carried frame{'s' if keep > 1 else ''} at most {TRACK_MAX_FRAMES} are "
                             "tracked at once")
        if self._carry is None:
            tr = track(labels, iou=self.iou, max_objects=self.max_objects, max_tracks=1, max_gap=self.max_gap,
                       motion=bwd[1:] if self.motion else None)
            ids, self.n_tracks = tr.track, tr.n_tracks
            self._carry = (labels[-keep:].contiguous().clone(), ids[-keep:].clone())
            self._vectors = bwd[-keep:].clone() if self.motion else None
        else:
            last, last_ids = self._carry
            if labels.shape[1:] != last.shape[1:] or labels.device != last.device:
                raise ValueError(f"labels {tuple(labels.shape)} on {labels.device}: the stream holds frames of {tuple(last.shape[1:])} on "
                                 f"{last.device}")
            c = int(last.shape[0])
            field = torch.cat((self._vectors[1:], bwd)) if self.motion else None      # row i: frames i + 1 -> i of cat(last, labels)
            tr = track(torch.cat((last, labels)), iou=self.iou, max_objects=self.max_objects, max_tracks=1, max_gap=self.max_gap,
                       motion=field)
            c0 = tr.track[:c].max()            # tracks are numbered by first frame: those headed in the carry are 1..c0
            ids = stream_remap(tr.track[c:], tr.track[:c], last_ids, c0, self.n_tracks).to(torch.int32)
            self.n_tracks = (self.n_tracks + tr.n_tracks - c0).to(torch.int32)
            self._carry = (torch.cat((last, labels))[-keep:].contiguous().clone(), torch.cat((last_ids, ids))[-keep:].clone())
            self._vectors = torch.cat((self._vectors, bwd))[-keep:].clone() if self.motion else None
        return ids


class FillStream:
    """``fill`` for a label stack that comes in chunks: for every split of a stack, the concatenation of what ``push`` and ``flush``
    return (labels, track, age, table) is ``fill(stack, track(stack, iou, max_objects, max_gap=G, motion=...), motion=...)`` bit for bit,
    and the four counts, summed over the calls, are the whole stack's (``totals`` holds the sums so far, int32 [4] on the device:
    objects, cells, dropped, vanished).  The track numbers are the whole stream's, ``TrackStream``'s, for segmented and carried objects.
    A frame m is spanned only by links (a -> f) with f in (m, m + G] and a >= m - G, and a link depends on the frames a .. f only
    (``TrackStream``), so a frame is final once G frames behind it are pushed, and a window that starts G frames before the first frame
    not yet returned holds every link that spans it: ``push`` returns all frames pushed so far except the last G, less those already
    returned -- possibly none -- and ``flush`` the rest, behind which no frame exists.  The stream holds at most 2 G frames beside the
    chunk.  Per push: ``TrackStream.push`` for the numbers, ``track`` over the window for prev / gap, and cgs_objects_track_fill_window
    over the frames that became final.  ``n_tracks`` is ``TrackStream``'s; nothing here synchronises with the host."""

    def __init__(self, iou, max_objects=64, max_gap=1, motion=False):
        max_gap = _max_gap(max_gap)
        if max_gap < 1:
            raise ValueError(f"max_gap must be 1..{TRACK_MAX_GAP} for FillStream (without a bridged link there is nothing to fill), got 0")
        self._stream = TrackStream(iou, max_objects=max_objects, max_gap=max_gap, motion=motion)
        self.iou, self.max_objects, self.max_gap, self.motion = self._stream.iou, self._stream.max_objects, max_gap, self._stream.motion
        self.totals = None                     # int32 [4] on the device after the first push
        self._labels = self._ids = self._bwd = None      # the window: frames _start .. _pushed - 1 of the stream
        self._start = self._done = self._pushed = 0      # _done: frames returned so far; _start = max(0, _done - max_gap)
        self._flushed = False

    @property
    def n_tracks(self):
        return self._stream.n_tracks

    def _empty(self, like):
        K, dev = self.max_objects, like.device
        zero = torch.zeros(4, dtype=torch.int32, device=dev)
        return Filled(like.new_empty((0,) + tuple(like.shape[1:])), torch.empty((0, K), dtype=torch.int32, device=dev),
                      torch.empty((0, K), dtype=torch.int32, device=dev), torch.empty((0, K, len(FIELDS)), dtype=torch.int32, device=dev),
                      zero[0], zero[1], zero[2], zero[3], None)

    def _final(self, upto):
        """The frames _done .. upto - 1 of the stream, filled; the window then starts max_gap frames before `upto`."""
        if upto <= self._done:
            return self._empty(self._labels)
        G, lo = self.max_gap, self._start
        field = self._bwd[1:] if self.motion else None                   # row i: frames i + 1 -> i of the window
        tr = track(self._labels, iou=self.iou, max_objects=self.max_objects, max_tracks=1, max_gap=G, motion=field)
        out = fill(self._labels, tr._replace(track=self._ids), motion=field, max_objects=self.max_objects,
                   frames=(self._done - lo, upto - lo))
        self.totals = self.totals + torch.stack((out.n_objects, out.n_cells, out.n_dropped, out.n_vanished))
        self._done = upto
        keep = max(lo, upto - G) - lo
        self._labels, self._ids = self._labels[keep:].contiguous(), self._ids[keep:].contiguous()
        if self.motion:
            self._bwd = self._bwd[keep:].contiguous()
        self._start = lo + keep
        return out

    def push(self, labels, bwd=None):
        """labels (and bwd with motion=True) as ``TrackStream.push`` takes them.  Returns ``fill``'s Filled for the frames that became
        final, in stream order: zero or more frames (rgb is None)."""
        if self._flushed:
            raise ValueError("the stream was flushed: a new stack needs a new FillStream")
        if isinstance(labels, torch.Tensor) and labels.dim() == 3 and int(labels.shape[0]) + 2 * self.max_gap > TRACK_MAX_FRAMES:
            raise ValueError(f"a chunk of {int(labels.shape[0])} frames: with the {2 * self.max_gap} frames of the window at most "
                             f"{TRACK_MAX_FRAMES} are tracked at once")
        ids = self._stream.push(labels, bwd)                             # (every check of the arguments is there)
        labels = labels.contiguous()
        if self._labels is None:
            self._labels, self._ids, self._bwd = labels, ids, bwd
            self.totals = torch.zeros(4, dtype=torch.int32, device=labels.device)
        else:
            self._labels, self._ids = torch.cat((self._labels, labels)), torch.cat((self._ids, ids))
            if self.motion:
                self._bwd = torch.cat((self._bwd, bwd))
        self._pushed += int(labels.shape[0])
        return self._final(self._pushed - self.max_gap)

    def flush(self):
        """The frames not yet returned, at most max_gap (none when everything was returned); the stream ends here."""
        if self._labels is None:
            raise ValueError("nothing was pushed")
        if self._flushed:
            raise ValueError("the stream was flushed already")
        self._flushed = True
        return self._final(self._pushed)


def switches(truth_prev, pred_track, best, iou):
    """truth_prev: ``track(truth).prev``, pred_track: ``track(pred).track``, both int32 [n,K]; best: ``match(pred, truth).best`` int32
    [n,2,K,4], all on one device; iou as ``match`` takes it.  int32 [T,3] on the device, per threshold (covered: truth objects whose best
    predicted partner reaches it, continued: truth links with both ends covered, switches: continued links whose two predicted partners
    lie in different predicted tracks).  Gaps are not bridged: an uncovered frame ends the comparison there.  The kernel reads
    truth_prev as "the label in frame f - 1", so with tracks of ``max_gap`` > 0 pass ``torch.where(tr.gap == 1, tr.prev, 0)``; what
    bridging buys shows in ``fragments``."""
    for name, t in (("truth_prev", truth_prev), ("pred_track", pred_track), ("best", best)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be torch.int32, got {t.dtype}")
    if truth_prev.dim() != 2 or truth_prev.shape != pred_track.shape:
        raise ValueError(f"truth_prev and pred_track must be [n,K] of one shape, got {tuple(truth_prev.shape)} and {tuple(pred_track.shape)}")
    n, K = (int(s) for s in truth_prev.shape)
    if n < 1 or not 1 <= K <= MATCH_MAX_OBJECTS or n > TRACK_MAX_FRAMES or tuple(best.shape) != (n, 2, K, 4):
        raise ValueError(f"[n,K] = [{n},{K}] (1..{TRACK_MAX_FRAMES} frames, K in 1..{MATCH_MAX_OBJECTS}) needs best [{n},2,{K},4], got "
                         f"{tuple(best.shape)}")
    milli = iou_milli(iou)
    if not torch.cuda.is_available() or not (truth_prev.is_cuda and pred_track.is_cuda and best.is_cuda):
        raise _lib.CgsError("objects.switches runs on the GPU (cgs_objects_track_switches); there is no CPU fallback")
    if not truth_prev.device == pred_track.device == best.device:
        raise ValueError("truth_prev, pred_track and best are on different devices")
    truth_prev, pred_track, best = truth_prev.contiguous(), pred_track.contiguous(), best.contiguous()
    dev = best.device
    with torch.cuda.device(dev):
        thr = torch.tensor(milli, dtype=torch.int32).to(dev)
        counts = torch.empty((len(milli), 3), dtype=torch.int32, device=dev)
        _lib.call("cgs_objects_track_switches", truth_prev.data_ptr(), pred_track.data_ptr(), best.data_ptr(), thr.data_ptr(), len(milli),
                  n, K, counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return counts


def fragments(truth_track, pred_track, best, iou):
    """truth_track: ``track(truth).track``, pred_track: ``track(pred).track``, int32 [n,K]; best: ``match(pred, truth).best`` int32
    [n,2,K,4], all on one device; iou as ``match`` takes it.  int64 [T] on that device: per matching threshold, over the covered truth
    objects (those whose best predicted partner reaches it), the number of distinct (truth track, predicted track) pairs less the
    number of distinct truth tracks -- 0 when every truth track is followed by one predicted track.  torch.unique on the device."""
    for name, t in (("truth_track", truth_track), ("pred_track", pred_track), ("best", best)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be torch.int32, got {t.dtype}")
    if truth_track.dim() != 2 or truth_track.shape != pred_track.shape:
        raise ValueError(f"truth_track and pred_track must be [n,K] of one shape, got {tuple(truth_track.shape)} and "
                         f"{tuple(pred_track.shape)}")
    n, K = (int(s) for s in truth_track.shape)
    if n < 1 or K < 1 or tuple(best.shape) != (n, 2, K, 4):
        raise ValueError(f"[n,K] = [{n},{K}] needs best [{n},2,{K},4], got {tuple(best.shape)}")
    if not truth_track.device == pred_track.device == best.device:
        raise ValueError("truth_track, pred_track and best are on different devices")
    milli = iou_milli(iou)
    row = best[:, 1].to(torch.int64)                                              # (pred partner, inter, area_t, area_p) per truth object
    partner, inter, union = row[..., 0], row[..., 1], row[..., 2] + row[..., 3] - row[..., 1]
    tt = truth_track.to(torch.int64)
    pt = torch.gather(pred_track.to(torch.int64), 1, (partner - 1).clamp(0, K - 1))
    base = int(n) * K + 1                                                         # more than any track number
    out = []
    for m in milli:
        cov = (partner >= 1) & (partner <= K) & (tt > 0) & (inter > 0) & (1000 * inter >= m * union)
        out.append(torch.unique(tt[cov] * base + pt[cov]).numel() - torch.unique(tt[cov]).numel())
    return torch.tensor(out, dtype=torch.int64, device=best.device)


# ---------------------------------------------------------------------------------------------------------------- the value of an object
def _value_stack(frames, labels, kept, max_objects, who, frames_range=None):
    """The checks ``ablate`` and ``value`` share; returns (frames, labels, kept, n, K, (f0, f1)) ready for the kernel."""
    for name, t, dtype in (("frames", frames, torch.uint8), ("labels", labels, torch.int32), ("kept", kept, torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if labels.dim() != 3 or tuple(labels.shape[1:]) != (VALUE_SIDE, VALUE_SIDE) or tuple(frames.shape) != tuple(labels.shape) + (3,):
        raise ValueError(f"labels must be [n,{VALUE_SIDE},{VALUE_SIDE}] and frames [n,{VALUE_SIDE},{VALUE_SIDE},3] (the critic takes only "
                         f"that size), got {tuple(labels.shape)} and {tuple(frames.shape)}")
    n = int(labels.shape[0])
    if n < 1 or tuple(kept.shape) != (n,):
        raise ValueError(f"at least one frame and kept [n], got {n} frames and kept {tuple(kept.shape)}")
    max_objects = _as_int(max_objects, "max_objects")
    if not 1 <= max_objects <= VALUE_MAX_OBJECTS:
        raise ValueError(f"max_objects must be 1..{VALUE_MAX_OBJECTS}, got {max_objects}")
    if not (frames.device == labels.device == kept.device):
        raise ValueError(f"frames, labels and kept are on {frames.device}, {labels.device} and {kept.device}")
    span = (0, n) if frames_range is None else _frame_range(frames_range, n)
    if not torch.cuda.is_available() or not labels.is_cuda:
        raise _lib.CgsError(f"objects.{who} runs on the GPU (cgs_objects_ablate); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensors are on {labels.device}") + " and there is no CPU fallback")
    return _aligned16(frames.contiguous()), labels.contiguous(), kept.contiguous(), n, max_objects, span


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()          # (a view at an odd byte offset: the kernel moves 16 bytes at a time)


def _value_fill(fill, allow_low=False):
    """``ablate``'s fill as (mode, R | G << 8 | B << 16, tensor or None, the JSON form); ValueError otherwise."""
    if isinstance(fill, str):
        if fill == "mean":
            return 2, 0, None, "mean"
        if fill == "low" and allow_low:
            return None, 0, None, "low"
        raise ValueError(f"fill {fill!r}: expected " + ('"low", ' if allow_low else "") + '"mean", (r, g, b) or a uint8 tensor [64,64,3]')
    if isinstance(fill, torch.Tensor):
        if fill.dtype != torch.uint8 or tuple(fill.shape) != (VALUE_SIDE, VALUE_SIDE, 3):
            raise ValueError(f"a fill frame must be a uint8 tensor [{VALUE_SIDE},{VALUE_SIDE},3], got {fill.dtype} {tuple(fill.shape)}")
        return 1, 0, fill, "frame"
    try:
        rgb = [_as_int(v, "fill colour") for v in fill]
    except TypeError:
        raise ValueError(f"fill {fill!r}: expected \"mean\", (r, g, b) or a uint8 tensor [64,64,3]") from None
    if len(rgb) != 3 or not all(0 <= v <= 255 for v in rgb):
        raise ValueError(f"fill colour {fill!r}: three whole numbers 0..255")
    return 0, rgb[0] | rgb[1] << 8 | rgb[2] << 16, None, rgb


def _value_grow(grow):
    grow = _as_int(grow, "grow")
    if not 0 <= grow <= VALUE_MAX_GROW:
        raise ValueError(f"grow must be 0..{VALUE_MAX_GROW}, got {grow}")
    return grow


def ablate(frames, labels, kept, fill="mean", grow=0, max_objects=64, frames_range=None):
    """The "this frame without object k" images of cgs_objects_ablate (its header comment in include/cgs_hip.h is the rule).  frames:
    uint8 device tensor [n,64,64,3]; labels: int32 [n,64,64] as ``label`` gives them; kept: int32 [n] (``Objects.kept``), on one device.
    The rows of frame f are its objects k = 1 .. min(kept[f], max_objects) in that order, frame by frame; row (f, k) is frame f with
    the fill written over every cell within `grow` cells (0..4, a clipped square) of a cell labelled k, other objects' cells included,
    and the frame's own bytes elsewhere.  fill: "mean" (per frame the rounded mean colour of its label-0 cells, of all cells when it has
    none, computed by the kernel), a colour (r, g, b), or one uint8 tensor [64,64,3] on the same device for all rows.  A label above
    max_objects gets no row and matches no k.  frames_range: None or (f0, f1), 0 <= f0 <= f1 <= n: only the rows of those frames;
    the concatenation over any split of 0..n is the whole-stack result bit for bit.
    Returns Ablated(images uint8 [rows,64,64,3], row_frame int32 [rows], row_label int32 [rows], offsets int32 [n + 1]: the exclusive
    prefix sum of the row counts over the WHOLE stack, so a range's rows are offsets[f0] .. offsets[f1] - 1).  The row count comes to
    the host (one synchronisation); without rows nothing is launched.  No CPU path: raises CgsError without a GPU."""
    mode, rgb, frame, _ = _value_fill(fill)
    grow = _value_grow(grow)
    frames, labels, kept, n, K, (f0, f1) = _value_stack(frames, labels, kept, max_objects, "ablate", frames_range)
    dev = labels.device
    if frame is not None:
        if frame.device != dev:
            raise ValueError(f"the fill frame is on {frame.device}, the frames on {dev}")
        frame = _aligned16(frame.contiguous())
    with torch.cuda.device(dev):
        offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(kept.clamp(0, K), 0)
        lo, hi = (int(v) for v in offsets[[f0, f1]].tolist())
        rows = hi - lo
        images = torch.empty((rows, VALUE_SIDE, VALUE_SIDE, 3), dtype=torch.uint8, device=dev)
        row_frame = torch.empty(rows, dtype=torch.int32, device=dev)
        row_label = torch.empty(rows, dtype=torch.int32, device=dev)
        if rows:
            _lib.call("cgs_objects_ablate", frames.data_ptr(), labels.data_ptr(), offsets.data_ptr(), n, f0, f1, K, grow, mode, rgb,
                      frame.data_ptr() if frame is not None else None, 0, rows, images.data_ptr(), row_frame.data_ptr(),
                      row_label.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return Ablated(images, row_frame, row_label, offsets)


def value_chunks(rows, chunk_rows):
    """``value``'s ranges: the frames cut greedily into consecutive ranges whose row total is at most chunk_rows (a frame joins the
    range while the total still fits, so a frame without rows always does); a range without rows is left out.  rows: the row count of
    every frame, each at most chunk_rows.  Returns [(f0, f1, rows)]."""
    out, f0, total = [], 0, 0
    for f, r in enumerate(int(v) for v in rows):
        if r > chunk_rows:
            raise ValueError(f"frame {f} has {r} rows, chunk_rows is {chunk_rows}")
        if total + r > chunk_rows:
            out.append((f0, f, total))
            f0, total = f, 0
        total += r
    out.append((f0, len(rows), total))
    return [c for c in out if c[2]]


def value(infer, frames, labels, kept, fill="low", grow=0, max_objects=64, chunk_rows=2048):
    """How far the critic's value of a frame falls when one object alone is taken out of it: the training rule replaced = A (1 - Z) +
    Z B asked once per object with a hard Z.  infer: a callable X_u8 [b,64,64,3] -> pred [b] float32 on the frames' device (the
    handler passes ``lambda X: eng.infer(X, want_mask=False)[0]``: fp32, eval mode); frames, labels, kept, grow, max_objects as
    ``ablate`` takes them; fill as there, or "low": the frame of smallest base value, the rule's B, one for the whole stack.
    1. base = infer over the frames in consecutive chunks of at most chunk_rows frames.
    2. "low" is the frame at int(np.argmin(base.cpu().numpy())): the first index on ties, taken on the host.
    3. The frames are cut into ranges of at most chunk_rows rows (``value_chunks``; chunk_rows >= 64, so a frame always fits); every
       range is one ``ablate`` and one infer over its rows.
    4. drop[f, k - 1] = base[f] - pred(row (f, k)), one float32 subtraction; entries without a row are 0.
    Returns Values(base float32 [n], drop float32 [n,max_objects], fill_frame: the index "low" chose, else None, rows: the row total,
    chunks: [(f0, f1, rows)] -- the chunk composition is part of the contract, a caller can repeat it).  A frame that is its own fill
    frame is rebuilt unchanged, so its objects have drop 0 exactly, by construction and not by measurement.
    Limits: one replacement at a time (no Shapley value: two objects that are each redundant with the other both score low); "mean"
    and a colour lie outside what the critic was trained on; one critic forward per object.  No CPU path."""
    if not callable(infer):
        raise ValueError(f"infer must be callable, got {type(infer).__name__}")
    mode, _, frame, _ = _value_fill(fill, allow_low=True)
    grow = _value_grow(grow)
    chunk_rows = _as_int(chunk_rows, "chunk_rows")
    if chunk_rows < VALUE_MAX_OBJECTS:
        raise ValueError(f"chunk_rows must be at least {VALUE_MAX_OBJECTS} (one frame's rows always fit), got {chunk_rows}")
    frames, labels, kept, n, K, _ = _value_stack(frames, labels, kept, max_objects, "value")
    if frame is not None and frame.device != labels.device:
        raise ValueError(f"the fill frame is on {frame.device}, the frames on {labels.device}")
    dev = labels.device
    with torch.cuda.device(dev):
        base = torch.cat([infer(frames[lo:lo + chunk_rows]).reshape(-1).to(torch.float32) for lo in range(0, n, chunk_rows)])
        fill_frame = None
        if mode is None:
            fill_frame = int(np.argmin(base.cpu().numpy()))
            fill = frames[fill_frame]
        counts = kept.clamp(0, K).cpu().numpy()
        chunks = value_chunks(counts, chunk_rows)
        drop = torch.zeros((n, K), dtype=torch.float32, device=dev)
        for f0, f1, rows in chunks:
            ab = ablate(frames, labels, kept, fill=fill, grow=grow, max_objects=K, frames_range=(f0, f1))
            pred = infer(ab.images).reshape(-1).to(torch.float32)
            if int(pred.shape[0]) != rows:
                raise ValueError(f"infer returned {int(pred.shape[0])} values for {rows} images")
            f, k = ab.row_frame.to(torch.int64), ab.row_label.to(torch.int64) - 1
            drop[f, k] = base[f] - pred
    return Values(base, drop, fill_frame, int(counts.sum()), chunks)


def select(res, keep):
    """The objects that pass: res: ``label``'s Objects with labels and a table of at least K rows; keep: bool or uint8 device tensor
    [n,K], K <= 64.  Old label k of frame f becomes 1 + the number of kept labels below it when k <= min(kept[f], K) and keep[f, k - 1],
    else 0 -- every label above K too: an object that was never scored is dropped (cgs_objects_select).  The order is kept, so the new
    numbers are still the raster order of the first pixel.  Returns (Objects(labels, mask bool, kept, found: passed through, table
    [n,K,8]: the kept rows in order, zero rows behind them), unscored int32 [n]: the objects above K that were dropped).  The reports
    and ``track`` take the result as they take ``label``'s.  No CPU path: raises CgsError without a GPU."""
    if not isinstance(res, Objects) or not isinstance(res.labels, torch.Tensor) or not isinstance(res.table, torch.Tensor):
        raise ValueError("res must be the result of objects.label with labels (want_labels=True) and its table")
    if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 2:
        raise ValueError("keep must be a bool or uint8 tensor [n,K], got "
                         + (f"{keep.dtype} {tuple(keep.shape)}" if isinstance(keep, torch.Tensor) else type(keep).__name__))
    labels, table, kept = res.labels, res.table, res.kept
    if labels.dtype != torch.int32 or labels.dim() != 3 or table.dtype != torch.int32 or kept.dtype != torch.int32:
        raise ValueError("res.labels must be int32 [n,h,w], res.table and res.kept int32")
    n, h, w = (int(s) for s in labels.shape)
    K = int(keep.shape[1])
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE) or not 1 <= K <= VALUE_MAX_OBJECTS or int(keep.shape[0]) != n:
        raise ValueError(f"labels {tuple(labels.shape)} and keep {tuple(keep.shape)}: n frames of 1..{MAX_SIDE} x 1..{MAX_SIDE} pixels and "
                         f"keep [n,K] with K in 1..{VALUE_MAX_OBJECTS}")
    if table.dim() != 3 or int(table.shape[0]) != n or int(table.shape[1]) < K or int(table.shape[2]) != len(FIELDS) or tuple(kept.shape) != (n,):
        raise ValueError(f"res.table {tuple(table.shape)} must be [{n},>={K},{len(FIELDS)}] and res.kept [{n}]")
    if not torch.cuda.is_available() or not labels.is_cuda:
        raise _lib.CgsError("objects.select runs on the GPU (cgs_objects_select); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensors are on {labels.device}") + " and there is no CPU fallback")
    dev = labels.device
    if not (table.device == kept.device == keep.device == dev):
        raise ValueError("res.labels, res.table, res.kept and keep are on different devices")
    labels, table, kept = labels.contiguous(), table[:, :K].contiguous(), kept.contiguous()
    keep = keep.contiguous()
    keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
    with torch.cuda.device(dev):
        out = torch.empty_like(labels)
        out_table = torch.empty_like(table)
        out_kept = torch.empty_like(kept)
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        unscored = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("cgs_objects_select", labels.data_ptr(), table.data_ptr(), kept.data_ptr(), keep.data_ptr(), n, h, w, K, out.data_ptr(),
                  out_table.data_ptr(), out_kept.data_ptr(), mask.data_ptr(), unscored.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return Objects(out, mask.view(torch.bool), out_kept, res.found, out_table), unscored


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_object_value_fill(s, flag="--object-value-fill"):
    """``--object-value-fill``: "low", "mean" or a colour "R,G,B" of whole numbers 0..255.  Returns "low", "mean" or (r, g, b)."""
    s = str(s).strip()
    if s in ("low", "mean"):
        return s
    try:
        rgb = tuple(int(p.strip()) for p in s.split(","))
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected low, mean or R,G,B") from None
    if len(rgb) != 3 or not all(0 <= v <= 255 for v in rgb):
        raise ValueError(f"{flag} {s!r}: expected low, mean or R,G,B with three whole numbers 0..255")
    return rgb


def parse_object_value_grow(s, flag="--object-value-grow"):
    """``--object-value-grow``: a whole number 0..4, the cells around an object that are replaced with it.  Returns the int."""
    try:
        v = int(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected a whole number 0..{VALUE_MAX_GROW}") from None
    if not 0 <= v <= VALUE_MAX_GROW:
        raise ValueError(f"{flag} {v}: expected a whole number 0..{VALUE_MAX_GROW}")
    return v


def parse_min_value_drop(s, flag="--min-value-drop"):
    """``--min-value-drop``: one finite number (it may be negative: a drop is a difference).  Returns the float."""
    try:
        v = float(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected one finite number") from None
    if v != v or abs(v) == float("inf"):
        raise ValueError(f"{flag} {s!r}: expected one finite number")
    return v


def value_keep(drop, kept, min_drop):
    """The keep table of ``select`` for a threshold: drop >= min_drop compared in float32 (a NaN is not kept), for the objects that
    have a row (k <= min(kept, K)).  drop float32 [n,K] and kept int32 [n] on one device; bool [n,K] there."""
    K = int(drop.shape[1])
    has_row = torch.arange(K, device=drop.device)[None] < kept.clamp(0, K)[:, None]
    return (drop >= torch.tensor(min_drop, dtype=torch.float32, device=drop.device)) & has_row


def value_report(values, kept, fill, grow, min_drop=None, keep=None, unscored=None, stems=None):
    """The "object_value" header of objects.json / the "value" block of eval_objects.json from ``value``'s result.  kept: the frames'
    object counts (tensor or array); fill: the flag's value ("low", "mean" or (r, g, b)); keep: ``value_keep``'s table with a
    threshold; unscored: the objects numbered above K, ``select``'s per-frame count or, without a selection, max(kept - K, 0); stems:
    the frames' names, then "fill_frame" is a name.  {"fill", "fill_frame", "grow", "min_value_drop", "rows", "unscored", "base_mean",
    "drop": {"mean", "min", "max", "negative"} over the scored objects in float64 (None without any), and with keep "selected_objects"}."""
    base, drop, kept = _host(values.base).astype(np.float64), _host(values.drop).astype(np.float64), _host(kept).reshape(-1).astype(np.int64)
    K = drop.shape[1]
    scored = np.arange(K)[None] < np.clip(kept, 0, K)[:, None]
    d = drop[scored]
    ff = values.fill_frame
    rep = {"fill": list(fill) if isinstance(fill, (tuple, list)) else fill,
           "fill_frame": None if ff is None else (stems[ff] if stems is not None else int(ff)), "grow": int(grow),
           "min_value_drop": None if min_drop is None else float(min_drop), "rows": int(values.rows),
           "unscored": int(np.maximum(kept - K, 0).sum()) if unscored is None else int(_host(unscored).sum()),
           "base_mean": float(base.mean()) if base.size else None,
           "drop": {"mean": float(d.mean()) if d.size else None, "min": float(d.min()) if d.size else None,
                    "max": float(d.max()) if d.size else None, "negative": int(np.count_nonzero(d < 0))}}
    if keep is not None:
        rep["selected_objects"] = int(np.count_nonzero(_host(keep) & scored))
    return rep


def parse_track_gap(s, flag="--track-gap"):
    """``--track-gap`` / ``--overlay-gap``: a whole number 0..8 (objects.TRACK_MAX_GAP).  Returns the int; ValueError otherwise."""
    try:
        g = int(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected a whole number 0..{TRACK_MAX_GAP}") from None
    if not 0 <= g <= TRACK_MAX_GAP:
        raise ValueError(f"{flag} {g}: expected a whole number 0..{TRACK_MAX_GAP}")
    return g


def parse_track_motion(s, flag="--track-motion"):
    """``--track-motion`` / ``--overlay-motion``: a whole number 0..4 (the search range of temporal.flow in cells a frame; 0: off).
    Returns the int; ValueError otherwise."""
    try:
        v = int(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected a whole number 0..{MOTION_MAX_SEARCH}") from None
    if not 0 <= v <= MOTION_MAX_SEARCH:
        raise ValueError(f"{flag} {v}: expected a whole number 0..{MOTION_MAX_SEARCH}")
    return v


def motion_report(bwd, search):
    """The "track_motion" block of tracks.json / eval_tracks.json / {stem}-tracks.json from the backward field the tracker used (int8
    [n - 1,8,8,2], tensor or array; may be empty): {"search", "block": 8, "mean_cells_per_frame": the mean Euclidean length of the
    vectors, "saturated": the share of vectors with a component at +-search} -- the figures the video report gives for
    --smooth-motion.  Both are None for an empty field."""
    v = _host(bwd).reshape(-1, 2).astype(np.float64)
    search = int(search)
    return {"search": search, "block": _lib.TEMPORAL_BLOCK,
            "mean_cells_per_frame": float(np.sqrt((v ** 2).sum(axis=1)).mean()) if len(v) else None,
            "saturated": float((np.abs(v).max(axis=1) >= search).mean()) if len(v) else None}


def fill_report(filled):
    """The "track_fill" block of tracks.json and the counts of eval_tracks.json's "fill" from ``fill``'s result: {"objects", "cells",
    "dropped", "vanished"}.  One transfer of the four scalars."""
    counts = torch.stack([filled.n_objects, filled.n_cells, filled.n_dropped, filled.n_vanished]).tolist()
    return dict(zip(("objects", "cells", "dropped", "vanished"), (int(v) for v in counts)))


def parse_track_reid(s, flag="--track-reid"):
    """``--track-reid``: the similarity threshold, one number in (0, 1], a whole number of thousandths.  Returns it as a float;
    ValueError otherwise."""
    s = str(s).strip()
    try:
        v = float(s)
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected one number in (0, 1]") from None
    try:
        return _reid_milli(v) / 1000
    except ValueError as e:
        raise ValueError(f"{flag} {s!r}: {e}") from None


def parse_track_reid_window(s, flag="--track-reid-window"):
    """``--track-reid-window``: a whole number 1..1024 (objects.REID_MAX_WINDOW), the most frames between the last frame of a track and
    the first of the track that continues it.  Returns the int; ValueError otherwise."""
    try:
        v = int(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected a whole number 1..{REID_MAX_WINDOW}") from None
    if not 1 <= v <= REID_MAX_WINDOW:
        raise ValueError(f"{flag} {v}: expected a whole number 1..{REID_MAX_WINDOW}")
    return v


def parse_track_reid_area(s, flag="--track-reid-area"):
    """``--track-reid-area``: a whole number >= 1, the pixels a track needs over its life to be re-identified.  Returns the int."""
    try:
        v = int(str(s).strip())
    except ValueError:
        raise ValueError(f"{flag} {s!r}: expected a whole number of at least 1") from None
    if not 1 <= v <= 0x7FFFFFFF:
        raise ValueError(f"{flag} {v}: expected a whole number of at least 1 (that fits 32 bits)")
    return v


def reid_report(reid, table, extra=None, sim=REID_SIM, window=REID_WINDOW, min_area=REID_MIN_AREA):
    """The "track_reid" block of tracks.json from ``reid``'s result and the tracks' table (and extra): {"sim", "window", "min_area",
    "bins": 64, "eligible", "links", "identities", "longest", "link_gaps": the links by first(u) - last(t) in LENGTH_BINS}.
    eval_tracks.json's "reid" is its four counts.  Tensors or arrays; the gaps are binned where they are."""
    counts = [int(v) for v in _host(torch.stack([reid.n_identities, reid.n_links, reid.n_eligible, reid.longest])
                                    if isinstance(reid.n_identities, torch.Tensor) else
                                    [reid.n_identities, reid.n_links, reid.n_eligible, reid.longest]).reshape(-1)]
    prev, table = _host(reid.prev).reshape(-1).astype(np.int64), _host(table).astype(np.int64)
    last = table[:, 0] + table[:, 2] - 1 + (_host(extra).astype(np.int64)[:, 1] if extra is not None else 0)
    u = np.flatnonzero(prev[:table.shape[0]] > 0)
    gaps = table[u, 0] - last[prev[u] - 1]
    if len(u) != counts[1] or (len(u) and gaps.min() < 1):
        raise ValueError(f"{len(u)} links in prev, the totals say {counts[1]} (or a link that does not run forward in time)")
    return {"sim": float(sim), "window": int(window), "min_area": int(min_area), "bins": REID_BINS, "eligible": counts[2],
            "links": counts[1], "identities": counts[0], "longest": counts[3],
            "link_gaps": dict(zip(LENGTH_BINS, (int(v) for v in length_hist(gaps))))}


def identity_rows(identity, reid_prev, n_tracks, first, last, lengths):
    """The "identities" list of tracks.json: identity, reid_prev [max_tracks] (tensors or arrays), and per track (index t - 1) the names
    of its first and last frame and its length in objects.  [{"identity", "tracks": [...], "first", "last", "objects"}] in order."""
    identity = _host(identity).reshape(-1)
    rows = {}
    for t in range(int(n_tracks)):
        row = rows.setdefault(int(identity[t]), {"identity": int(identity[t]), "tracks": [], "first": first[t], "last": last[t], "objects": 0})
        row["tracks"].append(t + 1)
        row["last"] = last[t]
        row["objects"] += int(lengths[t])
    return [rows[k] for k in sorted(rows)]


def parse_track_iou(s):
    """``--track-iou``: one number in (0, 1], a whole number of thousandths.  Returns it as a float; ValueError otherwise."""
    s = str(s).strip()
    try:
        v = float(s)
    except ValueError:
        raise ValueError(f"--track-iou {s!r}: expected one number in (0, 1]") from None
    try:
        return _track_milli(v) / 1000
    except ValueError as e:
        raise ValueError(f"--track-iou {s!r}: {e}") from None


def natural_order(stems):
    """Indices that sort the names with every run of digits compared as a number (frame2 before frame10); names that compare equal
    that way (frame01, frame1) are ordered as plain strings."""
    stems = [str(s) for s in stems]

    def key(i):
        pieces = re.split(r"(\d+)", stems[i])
        return [(0, int(p), "") if k % 2 else (1, 0, p) for k, p in enumerate(pieces) if p != ""], stems[i]

    return sorted(range(len(stems)), key=key)


def length_hist(lengths):
    """The table's length column (tensor on any device, or array; zero rows are no tracks) -> the 7 counts of LENGTH_BINS, int64 on
    the column's device (torch) or the host (numpy)."""
    if isinstance(lengths, torch.Tensor):
        v = lengths.reshape(-1).to(torch.int64)
        v = v[v > 0]
        bins = torch.bucketize(v, torch.tensor([1, 2, 4, 8, 16, 32], dtype=torch.int64, device=v.device))
        return torch.bincount(bins, minlength=len(LENGTH_BINS))
    v = np.asarray(lengths).reshape(-1).astype(np.int64)
    v = v[v > 0]
    return np.bincount(np.searchsorted(np.array([1, 2, 4, 8, 16, 32]), v, side="left"), minlength=len(LENGTH_BINS))


def track_report(totals, lengths, inter_sum=0, union_sum=0, untracked=0, max_gap=0, gap_links=None, missed=0):
    """One side of eval_tracks.json / tracks.json.  totals: (tracks, links, objects, longest) of ``track``; lengths: the table's length
    column (a tensor is binned where it is and only the 7 counts come to the host); inter_sum, union_sum: the sums of those columns;
    untracked: objects numbered above max_objects.  {"objects", "untracked_objects", "tracks", "links", "singletons", "mean_length":
    objects / tracks, "max_length", "length_hist": {"1", "2", "3-4", "5-8", "9-16", "17-32", "33+"}, "link_iou": inter_sum / union_sum};
    a ratio with a zero denominator is None.  With max_gap G > 0 (gap_links: ``track``'s, missed: the sum of its extra's second
    column) the fourth total is the longest span: "max_length" is then the largest length, and the dict gains "track_gap": G,
    "bridged_links", "missed_frames", "links_by_gap": {"1", ..., "G+1"} and "max_span"."""
    n_tracks, n_links, n_objects, longest = (int(v) for v in _host(totals).reshape(-1))
    hist = [int(v) for v in _host(length_hist(lengths))]
    inter_sum, union_sum, untracked = int(inter_sum), int(union_sum), int(untracked)
    if min(n_tracks, n_links, n_objects, longest, inter_sum, union_sum, untracked) < 0 or n_tracks + n_links != n_objects:
        raise ValueError(f"{n_tracks} tracks and {n_links} links do not make {n_objects} objects")
    if sum(hist) != n_tracks:
        raise ValueError(f"the length column holds {sum(hist)} tracks, the totals say {n_tracks}")
    ratio = lambda a, b: a / b if b else None
    side = {"objects": n_objects, "untracked_objects": untracked, "tracks": n_tracks, "links": n_links, "singletons": hist[0],
            "mean_length": ratio(n_objects, n_tracks), "max_length": longest, "length_hist": dict(zip(LENGTH_BINS, hist)),
            "link_iou": ratio(inter_sum, union_sum)}
    max_gap = _max_gap(max_gap)
    if max_gap:
        by_gap = [int(v) for v in _host(gap_links).reshape(-1)]
        if len(by_gap) != max_gap + 1 or min(by_gap) < 0 or sum(by_gap) != n_links or int(missed) < 0:
            raise ValueError(f"gap_links {by_gap} must be {max_gap + 1} counts that add up to the {n_links} links")
        lengths = _host(lengths).reshape(-1)
        side.update({"max_length": int(lengths.max()) if lengths.size else 0, "track_gap": max_gap, "bridged_links": sum(by_gap[1:]),
                     "missed_frames": int(missed), "links_by_gap": {str(g + 1): v for g, v in enumerate(by_gap)}, "max_span": longest})
    return side


def track_rows(table, n_tracks, extra=None):
    """table [max_tracks,8] (tensor or array) -> the first min(n_tracks, max_tracks) tracks as {"track", "first_frame", "first_label",
    "length", "area_sum", "area_min", "area_max", "inter_sum", "union_sum", "link_iou": inter_sum / union_sum (None for a singleton)}.
    extra [max_tracks,2] (``track``'s with max_gap > 0): the rows gain "bridges", "missed" and "last_frame" = first_frame + length +
    missed - 1."""
    table = _host(table)
    if extra is not None:
        extra = _host(extra)
        if extra.shape != (table.shape[0], 2):
            raise ValueError(f"extra {extra.shape} must be [{table.shape[0]}, 2]")
    if table.ndim != 2 or table.shape[1] != len(TRACK_FIELDS):
        raise ValueError(f"table {table.shape} must be [max_tracks, {len(TRACK_FIELDS)}]")
    n_tracks = int(n_tracks)
    if n_tracks < 0:
        raise ValueError(f"n_tracks must not be negative, got {n_tracks}")
    rows = []
    for t in range(min(n_tracks, table.shape[0])):
        row = {"track": t + 1, **{k: int(v) for k, v in zip(TRACK_FIELDS, table[t])}}
        row["link_iou"] = row["inter_sum"] / row["union_sum"] if row["union_sum"] else None
        if extra is not None:
            row.update(bridges=int(extra[t, 0]), missed=int(extra[t, 1]), last_frame=row["first_frame"] + row["length"] + int(extra[t, 1]) - 1)
        rows.append(row)
    return rows


def parse_match_iou(s):
    """``"0.5-0.75-0.95"`` (dash-separated) or ``"lo:hi:n"`` (np.linspace(lo, hi, n) in float64), as --thresh-grid is written.  Returns
    the thresholds as floats, whole thousandths (0.5:0.95:10 gives exactly 0.5, 0.55, ..., 0.95); ValueError as ``iou_milli``."""
    s = str(s).strip()
    try:
        if ":" in s:
            lo, hi, n = s.split(":")
            if int(n) < 1:
                raise ValueError
            vals = np.linspace(float(lo), float(hi), int(n), dtype=np.float64).tolist()
        else:
            vals = [float(p) for p in s.split("-")]                      # an empty item ("0.5-", "0.5--0.6") is no number
    except ValueError:
        raise ValueError(f"--match-iou {s!r}: expected dash-separated numbers (0.5-0.75-0.95) or lo:hi:n") from None
    try:
        return [m / 1000 for m in iou_milli(vals)]
    except ValueError as e:
        raise ValueError(f"--match-iou {s!r}: {e}") from None


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def match_report(pred_max, truth_max, matched_pred, matched_truth, sum_iou, iou, max_objects=MATCH_MAX_OBJECTS):
    """One block of eval_match.json from the outputs of ``match`` over a stack (tensors or arrays: pred_max, truth_max [n],
    matched_pred, matched_truth [n,T]) and sum_iou [T]: {"pred_objects": sum of pred_max, "truth_objects", "overflow_frames": frames
    where either map holds more than max_objects objects (those beyond it can never match), "per_iou": per threshold {"iou",
    "matched_pred", "matched_truth", "fp": pred_objects - matched_pred, "fn": truth_objects - matched_truth, "precision": matched_pred /
    pred_objects, "recall": matched_truth / truth_objects, "f1": their harmonic mean, "sum_iou", "pq": sum_iou / (matched_pred + fp / 2
    + fn / 2)}}.  A ratio with a zero denominator is None."""
    milli = iou_milli(iou)
    pred_max, truth_max = _host(pred_max).reshape(-1).astype(np.int64), _host(truth_max).reshape(-1).astype(np.int64)
    mp, mt = _host(matched_pred).astype(np.int64), _host(matched_truth).astype(np.int64)
    sums = _host(sum_iou).reshape(-1).astype(np.float64)
    n, T = pred_max.shape[0], len(milli)
    if truth_max.shape[0] != n or mp.shape != (n, T) or mt.shape != (n, T) or sums.shape[0] != T:
        raise ValueError(f"{n} and {truth_max.shape[0]} frames, matched counts {mp.shape} and {mt.shape}, {sums.shape[0]} sums: "
                         f"expected [n], [n], [n,{T}], [n,{T}] and [{T}]")
    ratio = lambda a, b: a / b if b else None
    n_pred, n_truth = int(pred_max.sum()), int(truth_max.sum())
    rows = []
    for k, m in enumerate(milli):
        tp_p, tp_t, s = int(mp[:, k].sum()), int(mt[:, k].sum()), float(sums[k])
        fp, fn = n_pred - tp_p, n_truth - tp_t
        if tp_p < 0 or tp_t < 0 or fp < 0 or fn < 0:
            raise ValueError(f"matched counts ({tp_p}, {tp_t}) do not fit {n_pred} predicted and {n_truth} truth objects")
        precision, recall = ratio(tp_p, n_pred), ratio(tp_t, n_truth)
        f1 = None if precision is None or recall is None else ratio(2 * precision * recall, precision + recall)
        rows.append({"iou": m / 1000, "matched_pred": tp_p, "matched_truth": tp_t, "fp": fp, "fn": fn, "precision": precision,
                     "recall": recall, "f1": f1, "sum_iou": s, "pq": ratio(s, tp_p + fp / 2 + fn / 2)})
    return {"pred_objects": n_pred, "truth_objects": n_truth,
            "overflow_frames": int(np.count_nonzero((pred_max > max_objects) | (truth_max > max_objects))), "per_iou": rows}


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
