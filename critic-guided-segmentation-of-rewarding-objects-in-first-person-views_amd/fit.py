"""Frames of any size for ``-process -fit`` (csrc/fit.hip): the network stays at 64 x 64 -- the critic's head is a Linear over the
flattened map -- and this module is the way in and the way out.  ``down`` shrinks uint8 frames of 64..4096 pixels a side to the
network's grid with the exact integer box average (a stretch, not a letterbox); ``up`` brings a 64 x 64 map back to the frame's size
by joint bilateral upsampling (Kopf et al., "Joint Bilateral Upsampling", SIGGRAPH 2007) guided by the frame, so that the mask's
outline follows the frame's edges and not the 64 x 64 staircase.  Both run on the GPU only; ``home_cells`` / ``box_weights`` /
``check_size`` are the pure host helpers.

The defaults sigma_s = 1 cell and sigma_r = 16 colour units are a judgement taken from the joint-bilateral literature (a spatial
Gaussian of about the low-resolution pixel pitch, a range Gaussian of a few percent of the colour scale); they are not a tuned result."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

SIDE, MAX_SIDE, RADIUS = _lib.FIT_SIDE, _lib.FIT_MAX_SIDE, _lib.FIT_RADIUS
SIGMA_SPATIAL, SIGMA_RANGE = 1.0, 16.0
MIN_SIGMA_SPATIAL = 0.5            # below it the smallest weight exp(-6.25 / sigma_s^2) of the nearest-colour tap leaves fp32's normal range

Up = namedtuple("Up", ["soft", "grey", "hard"])


# ---------------------------------------------------------------------------------------------------------------- host helpers
def check_size(h, w):
    """(h, w) as ints; ValueError unless both are whole numbers in 64..4096."""
    for name, v in (("h", h), ("w", w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
        if not SIDE <= v <= MAX_SIDE:
            raise ValueError(f"{name} = {v}: a frame is {SIDE} to {MAX_SIDE} pixels a side")
    return int(h), int(w)


def home_cells(L):
    """int64 [L]: the cell of the 64-cell grid that holds the centre of pixel p of an axis of length L, ((2 p + 1) 32) // L."""
    L, _ = check_size(L, SIDE)
    return ((2 * np.arange(L, dtype=np.int64) + 1) * 32) // L


def box_weights(L):
    """int64 [64, L]: w_L(o, s), the length of the overlap of output cell o = [L o, L o + L) and source pixel s = [64 s, 64 s + 64) on
    an axis of length L.  Rows sum to L, columns to 64; at L = 64 it is 64 times the identity."""
    L, _ = check_size(L, SIDE)
    o, s = np.arange(SIDE, dtype=np.int64)[:, None], np.arange(L, dtype=np.int64)[None, :]
    return np.maximum(np.minimum(L * o + L, SIDE * s + SIDE) - np.maximum(L * o, SIDE * s), 0)


def check_sigmas(sigma_s, sigma_r, names=("sigma_s", "sigma_r")):
    """(sigma_s, sigma_r) as floats; ValueError for a value that is not a finite number, sigma_s < 0.5 or sigma_r <= 0."""
    out = []
    for name, v, least, strict in ((names[0], sigma_s, MIN_SIGMA_SPATIAL, False), (names[1], sigma_r, 0.0, True)):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {v!r}") from None
        if not math.isfinite(v) or v > 3.0e38:
            raise ValueError(f"{name} = {v!r} is not a finite number")
        if v < least or (strict and v == least):
            raise ValueError(f"{name} = {v!r}: " + (f"at least {least} cells" if not strict else "must be positive"))
        out.append(v)
    return tuple(out)


def _frames(name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{name} must be uint8, got {t.dtype}")
    if t.dim() != 4 or t.shape[-1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{name} must be [n,H,W,3] with at least one frame, got {tuple(t.shape)}")
    try:
        check_size(int(t.shape[1]), int(t.shape[2]))
    except ValueError as e:
        raise ValueError(f"{name} {tuple(t.shape)}: {e}") from None
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def _need_gpu(what, *tensors):
    if not torch.cuda.is_available() or not all(t.is_cuda for t in tensors):
        raise _lib.CgsError(f"{what} runs on the GPU; " + ("no GPU is visible" if not torch.cuda.is_available() else
                            "the tensors are on " + ", ".join(str(t.device) for t in tensors)) + " and there is no CPU fallback")
    if len({t.device for t in tensors}) != 1:
        raise ValueError("the tensors are on several devices: " + ", ".join(str(t.device) for t in tensors))


# ---------------------------------------------------------------------------------------------------------------- the GPU calls
def down(frames_u8):
    """frames_u8: device tensor uint8 [n,H,W,3], 64 <= H, W <= 4096.  Returns uint8 [n,64,64,3] on the same device: per channel the
    exact box average (2 S + H W) // (2 H W) with S the pixel values weighted by box_weights(H) x box_weights(W): the block mean when H
    and W are multiples of 64, a copy at 64 x 64.  Integer throughout, bit for bit reproducible.  No CPU path: raises CgsError without a GPU."""
    n, h, w = _frames("frames_u8", frames_u8)
    _need_gpu("fit.down (cgs_fit_down_u8)", frames_u8)
    frames_u8 = frames_u8.contiguous()
    with torch.cuda.device(frames_u8.device):
        out = torch.empty((n, SIDE, SIDE, 3), dtype=torch.uint8, device=frames_u8.device)
        _lib.call("cgs_fit_down_u8", frames_u8.data_ptr(), n, h, w, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def up(values, guide, low=None, sigma_s=SIGMA_SPATIAL, sigma_r=SIGMA_RANGE, thresh=None, inclusive=True, want=("soft",)):
    """values: device tensor [n,64,64], float32 in [0,1], or uint8 / bool labels (non-zero = 1.0).  guide: uint8 [n,H,W,3], the frames.
    low: uint8 [n,64,64,3] = down(guide), computed here when None.  sigma_s >= 0.5 in cells, sigma_r > 0 in colour units of 0..255.
    want: some of "soft", "grey", "hard"; "hard" needs thresh.
    Joint bilateral upsampling over the 5 x 5 cells around a pixel's home cell (home_cells), taps outside the grid skipped:
    w = exp(-(ds / (2 sigma_s^2) + (d2 - d2_min) / (2 sigma_r^2))), ds the squared distance in cells from the pixel's centre to the
    cell's, d2 the squared colour distance of guide[y,x] and low[cell], d2_min its smallest value over the taps (integers), and
    soft = sum w m / sum w in float32.  Returns Up(soft float32 [n,H,W], grey uint8 [n,H,W] = soft * 255 truncated in float32, hard
    uint8 [n,H,W] = soft >= thresh, or > thresh without inclusive), an entry not asked for being None, on the inputs' device.
    No CPU path: raises CgsError without a GPU."""
    if not isinstance(values, torch.Tensor):
        raise ValueError(f"values must be a torch tensor, got {type(values).__name__}")
    n, h, w = _frames("guide", guide)
    if values.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise ValueError(f"values must be float32, uint8 or bool, got {values.dtype}")
    if tuple(values.shape) != (n, SIDE, SIDE):
        raise ValueError(f"values must be [{n},{SIDE},{SIDE}] for {n} guide frames, got {tuple(values.shape)}")
    if low is not None:
        if not isinstance(low, torch.Tensor) or low.dtype != torch.uint8 or tuple(low.shape) != (n, SIDE, SIDE, 3):
            raise ValueError(f"low must be a uint8 tensor [{n},{SIDE},{SIDE},3], got "
                             + (f"{low.dtype} {tuple(low.shape)}" if isinstance(low, torch.Tensor) else type(low).__name__))
    if n > 65535:
        raise ValueError(f"guide: at most 65535 frames a call, got {n}")
    sigma_s, sigma_r = check_sigmas(sigma_s, sigma_r)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in Up._fields for k in want):
        raise ValueError(f"want must name some of {Up._fields}, got {want!r}")
    thr = 0.0
    if "hard" in want:
        if thresh is None:
            raise ValueError("want 'hard' needs thresh")
        thr = float(thresh)
        if thr != thr:
            raise ValueError("thresh is NaN")
    tensors = (values, guide) + ((low,) if low is not None else ())
    _need_gpu("fit.up (cgs_fit_up_joint)", *tensors)
    values, guide = values.contiguous(), guide.contiguous()
    if values.dtype == torch.bool:
        values = values.view(torch.uint8)
    low = down(guide) if low is None else low.contiguous()
    dev = guide.device
    with torch.cuda.device(dev):
        outs = {k: torch.empty((n, h, w), dtype=torch.float32 if k == "soft" else torch.uint8, device=dev) for k in want}
        ptr = lambda k: outs[k].data_ptr() if k in outs else None
        _lib.call("cgs_fit_up_joint", values.data_ptr(), _lib.FIT_MAP_F32 if values.dtype == torch.float32 else _lib.FIT_MAP_U8,
                  guide.data_ptr(), low.data_ptr(), n, h, w, sigma_s, sigma_r, thr, int(bool(inclusive)), ptr("soft"), ptr("grey"),
                  ptr("hard"), torch.cuda.current_stream().cuda_stream)
    return Up(*(outs.get(k) for k in Up._fields))
