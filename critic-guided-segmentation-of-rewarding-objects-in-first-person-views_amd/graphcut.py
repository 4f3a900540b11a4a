"""GrabCut-style mask refinement on the GPU (csrc/graph_cut.hip): an exact binary min cut per frame, seeded by the soft mask, with
colour histograms of the frame's own foreground and background as the models and contrast-weighted links between neighbouring cells
(cgs_graph_cut, whose header comment in include/cgs_hip.h is the rule).  Everything on the device is an integer or a float compare,
and the largest source side of a minimum cut is unique, so the result is pinned bit for bit (tests/graph_cut_ref.py: scipy's max
flow).  ``cut`` is the device entry; ``tables``, ``parse_spec``, ``spec_text`` and ``cut_report`` are the pure host helpers of
``--graph-cut``."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_SIDE, MAX_ITERS, MAX_LAMBDA, SCALE = _lib.CUT_MAX_SIDE, _lib.CUT_MAX_ITERS, _lib.CUT_MAX_LAMBDA, _lib.CUT_SCALE
EMPTY, EARLY, NOT_CONVERGED = _lib.CUT_EMPTY, _lib.CUT_EARLY, _lib.CUT_NOT_CONVERGED
STATS = ("status", "iterations", "rounds", "energy", "seed_on", "on", "unknown", "changed")
KEYS = ("lo", "hi", "lambda", "it", "bins", "conn")
# judgements, not tuned values: the weight of the contrast term, the cuts a frame gets, the bins a channel
LAMBDA, ITERS, BINS, CONN = 50, 3, 8, 8
# the most rounds (searches from the sink) a cut may take before it gives up (CUT_NOT_CONVERGED).  At the kernel's 16 sweeps a round the
# most any frame took on an MI355X was 7 (tools/time_graph_cut.py's 2450-frame stack, profiles/graph_cut_time.jsonl) and 6 on the test
# stacks; the bound is empirical, so the default keeps 18 times the larger figure (the issue asks for at least 8)
MAX_ROUNDS = 128

Cut = namedtuple("Cut", ["mask", "stats"])
_tables = {}


def _whole(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be a whole number {lo}..{hi}, got {v!r}")
    return int(v)


def tables(lam):
    """(WA, WD, L), the int32 tables of the rule, made in float64: WA[i] = rint(16 lam exp(-i / 128)) and WD[i] = WA's value over
    sqrt(2) before the rounding, i = 0..1023 (the capacity of an axial / a diagonal pair); L[k] = rint(16 ln k), k = 1..4608, L[0] = 0
    (not read)."""
    lam = _whole(lam, "lambda", 0, MAX_LAMBDA)
    e = SCALE * lam * np.exp(-np.arange(_lib.CUT_TABLE, dtype=np.float64) / 128.0)
    L = np.zeros(_lib.CUT_LOG_TABLE, dtype=np.float64)
    L[1:] = SCALE * np.log(np.arange(1, _lib.CUT_LOG_TABLE, dtype=np.float64))
    return np.rint(e).astype(np.int32), np.rint(e / math.sqrt(2.0)).astype(np.int32), np.rint(L).astype(np.int32)


def default_band(thresh):
    """(lo, hi) when they are not given: half way from the threshold to 0 and to 1 (a judgement, not a tuned value)."""
    return thresh / 2.0, (1.0 + thresh) / 2.0


def check_band(thresh, lo, hi, what="graphcut.cut"):
    """lo <= thresh <= hi as the kernel compares them (float32), none a NaN; returns the three as float32-exact floats."""
    t, a, b = (float(np.float32(v)) for v in (thresh, lo, hi))
    if t != t or a != a or b != b:
        raise ValueError(f"{what}: thresh, lo and hi must be numbers, got {thresh!r}, {lo!r}, {hi!r}")
    if not a <= t <= b:
        raise ValueError(f"{what}: lo <= thresh <= hi is required (a hard cell agrees with its seed), got lo={lo!r}, thresh={thresh!r}, hi={hi!r}")
    return t, a, b


def cut(frames_u8, mask, thresh, inclusive=False, lo=None, hi=None, lam=LAMBDA, iters=ITERS, bins=BINS, connectivity=CONN, max_rounds=None,
        sweeps=None):
    """frames_u8: device tensor uint8 [n,h,w,3] or [h,w,3] (RGB), mask: float32 [n,h,w] or [h,w] on the same device, 1 <= h, w <= 64.
    The seed labelling is mask > thresh, or mask >= thresh with inclusive (float32 compares, a NaN is off); cells with mask < lo (and
    NaNs) are hard background, cells with mask > hi hard foreground, the others are decided by up to `iters` (1..8) exact min cuts:
    colour histograms of `bins` (4 | 8) bins a channel of the current labelling as t-links, lam (0..100) times a contrast weight as
    n-links over the `connectivity` (4 | 8) neighbourhood (the rule: cgs_graph_cut in include/cgs_hip.h).  lo, hi default to
    default_band(thresh); lo <= thresh <= hi.  max_rounds (default MAX_ROUNDS) bounds the rounds of a cut: a cut that needs more keeps
    the labelling it started from and sets NOT_CONVERGED.  sweeps (16 | 32 | 64): the sweeps of a round, for timing; not part of the result.
    Returns Cut(mask bool [n,h,w], stats int32 [n,8] (STATS)), both on the device.  No CPU path: raises CgsError without a GPU."""
    for name, t in (("frames_u8", frames_u8), ("mask", mask)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be [n,h,w] or [h,w], got {tuple(mask.shape)}")
    if mask.dim() == 2:
        mask = mask[None]
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]
    n, h, w = (int(s) for s in mask.shape)
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"mask {tuple(mask.shape)}: at least one frame of 1..{MAX_SIDE} x 1..{MAX_SIDE} cells")
    if mask.dtype != torch.float32:
        raise ValueError(f"mask must be float32, got {mask.dtype}")
    if frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != (n, h, w, 3):
        raise ValueError(f"frames_u8 must be uint8 {(n, h, w, 3)}, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    if thresh is None:
        raise ValueError("graphcut.cut needs thresh")
    d_lo, d_hi = default_band(float(thresh))
    thr, lo_v, hi_v = check_band(thresh, d_lo if lo is None else lo, d_hi if hi is None else hi)
    lam = _whole(lam, "lam", 0, MAX_LAMBDA)
    iters = _whole(iters, "iters", 1, MAX_ITERS)
    if bins not in (4, 8):
        raise ValueError(f"bins must be 4 or 8, got {bins!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    max_rounds = _whole(MAX_ROUNDS if max_rounds is None else max_rounds, "max_rounds", 1, _lib.CUT_MAX_ROUNDS)
    if sweeps is not None and sweeps not in (16, 32, 64):
        raise ValueError(f"sweeps must be 16, 32 or 64, got {sweeps!r}")
    if not torch.cuda.is_available() or not mask.is_cuda or frames_u8.device != mask.device:
        raise _lib.CgsError("graphcut.cut runs on the GPU (cgs_graph_cut); " + ("no GPU is visible" if not torch.cuda.is_available()
                            else f"the tensors are on {frames_u8.device} and {mask.device}") + " and there is no CPU fallback")
    frames_u8, mask = frames_u8.contiguous(), mask.contiguous()
    dev = mask.device
    key = (lam, str(dev))
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(t).to(dev) for t in tables(lam))
    wa, wd, L = _tables[key]
    kind = _lib.OBJ_F32_GE if inclusive else _lib.OBJ_F32_GT
    with torch.cuda.device(dev):
        out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        stats = torch.empty((n, len(STATS)), dtype=torch.int32, device=dev)
        head = (frames_u8.data_ptr(), mask.data_ptr(), kind, thr, lo_v, hi_v, n, h, w, int(connectivity), int(bins), iters, max_rounds)
        tail = (wa.data_ptr(), wd.data_ptr(), L.data_ptr(), out.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if sweeps is None:
            _lib.call("cgs_graph_cut", *head, *tail)
        else:
            _lib.call("cgs_graph_cut_sweeps", *head, int(sweeps), *tail)
    return Cut(out.view(torch.bool), stats)


# ---------------------------------------------------------------------------------------------------------------- host helpers
def parse_spec(s, flag="--graph-cut"):
    """``"lo=0.1;hi=0.9;lambda=50;it=3;bins=8;conn=8"``: --clean's KEY=value;... with one value per key, keys in any order, every key
    optional (an empty string is the defaults).  lo, hi: finite numbers (default None: default_band of the threshold the path compares
    with), lambda: 0..100, it: 1..8, bins: 4 | 8, conn: 4 | 8.  Returns {"lo", "hi": float or None, "lambda", "it", "bins", "conn":
    ints}.  ValueError naming the flag for an unknown or repeated key, an empty item, a non-number, a value out of range or lo > hi."""
    spec = {"lo": None, "hi": None, "lambda": LAMBDA, "it": ITERS, "bins": BINS, "conn": CONN}
    seen = set()
    for item in (str(s).split(";") if str(s).strip() else []):
        key, eq, val = (t.strip() for t in item.partition("="))
        if not eq or key not in KEYS or not val:
            raise ValueError(f"{flag} {item!r}: expected KEY=value with KEY one of {', '.join(KEYS)}")
        if key in seen:
            raise ValueError(f"{flag}: {key} is given twice")
        seen.add(key)
        if key in ("lo", "hi"):
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
            lo, hi = {"lambda": (0, MAX_LAMBDA), "it": (1, MAX_ITERS), "bins": (4, 8), "conn": (4, 8)}[key]
            if not lo <= v <= hi or (key in ("bins", "conn") and v not in (4, 8)):
                raise ValueError(f"{flag} {item!r}: {key} is " + ("4 or 8" if key in ("bins", "conn") else f"a whole number {lo}..{hi}"))
            spec[key] = v
    if spec["lo"] is not None and spec["hi"] is not None and spec["lo"] > spec["hi"]:
        raise ValueError(f"{flag} {s!r}: lo lies above hi")
    return spec


def spec_band(spec, thresh, flag="--graph-cut"):
    """(lo, hi) of a parsed spec at the threshold its path compares with, the defaults filled in; ValueError unless lo <= thresh <= hi."""
    d_lo, d_hi = default_band(float(thresh))
    lo, hi = d_lo if spec["lo"] is None else spec["lo"], d_hi if spec["hi"] is None else spec["hi"]
    check_band(thresh, lo, hi, flag)
    return lo, hi


def spec_text(spec):
    """A parsed spec in its canonical written form (KEYS order; lo and hi only when given)."""
    return ";".join(f"{k}={spec[k]}" for k in KEYS if spec[k] is not None)


def spec_kwargs(spec):
    """A parsed spec as the keyword arguments of ``cut``."""
    return dict(lo=spec["lo"], hi=spec["hi"], lam=spec["lambda"], iters=spec["it"], bins=spec["bins"], connectivity=spec["conn"])


def cut_report(stats, spec):
    """stats: int [n,8] or [8] (tensor or array) of ``cut`` -> the JSON block {"spec": the parsed spec, "frames": n, "empty", "early",
    "not_converged": the frames with that status bit, "iterations", "energy", "seed_on", "on", "unknown", "changed": sums, "rounds":
    the most any frame's cut took}."""
    c = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    c = c.reshape(-1, len(STATS)).astype(np.int64)
    bits = {"empty": EMPTY, "early": EARLY, "not_converged": NOT_CONVERGED}
    return {"spec": dict(spec), "frames": int(c.shape[0]), **{k: int(np.count_nonzero(c[:, 0] & b)) for k, b in bits.items()},
            **{k: int(c[:, STATS.index(k)].sum()) for k in ("iterations", "energy", "seed_on", "on", "unknown", "changed")},
            "rounds": int(c[:, 2].max()) if len(c) else 0}
