"""Masks smoothed along time for ``-process --source-video --smooth R`` (csrc/temporal.hip).  The network sees one frame at a time, so
its masks flicker when they are played as a video; ``smooth`` is a spatio-temporal joint bilateral filter over the stack of 64 x 64 masks,
guided by the shrunk frames (``fit.down``): a cell is averaged with the 3 x 3 cells around it in the R frames before and after, each
weighted by a Gaussian in time (sigma_t = R / 2), in space (sigma 1 cell) and in the colour distance to the cell's own colour (sigma_r).
Motion is not compensated -- the 3 x 3 search and the range term stand in for a motion model: a cell whose colour changed gets no weight
from the other frame.  Runs on the GPU only; ``check_radius`` / ``sigma_t`` are the pure host helpers.

The default sigma_r = 16 colour units is the same judgement as ``fit.SIGMA_RANGE``, not a tuned result."""
import numpy as np
import torch

from . import _lib
from .fit import _need_gpu, check_sigmas

SIDE, MAX_RADIUS = _lib.TEMPORAL_SIDE, _lib.TEMPORAL_MAX_RADIUS
SIGMA_RANGE = 16.0


def check_radius(radius, least=1, name="radius"):
    """radius as an int; ValueError unless it is a whole number in least..8."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {radius!r}")
    if not least <= radius <= MAX_RADIUS:
        raise ValueError(f"{name} = {radius}: {least} to {MAX_RADIUS} frames each way")
    return int(radius)


def sigma_t(radius):
    """The temporal sigma in frames: the window of +-radius frames is +-2 sigma."""
    return check_radius(radius) / 2.0


def smooth(z, low, radius, sigma_r=SIGMA_RANGE, f0=0, f1=None):
    """z: device tensor float32 [n,64,64] in [0,1].  low: uint8 [n,64,64,3] = fit.down of the frames.  radius 1..8, sigma_r > 0.
    Returns float32 [f1 - f0,64,64], frames f0 <= f < f1 of the smoothed stack (all of it by default), on the inputs' device.
    For frame f and cell p: the centre tap (f, p) with weight exactly 1, then k = -radius .. -1, 1 .. radius, frame g = f + k when
    0 <= g < n, the 3 x 3 cells p + (dy, dx) inside the grid (dy outer, dx inner), w = exp(-(k^2 / (2 sigma_t^2) + (dy^2 + dx^2) / 2 +
    d2 / (2 sigma_r^2))) with d2 the integer squared colour distance of low[g][p + (dy, dx)] and low[f][p]; out = sum w z / sum w in
    float32 in that order.  Frames outside the stack and cells outside the grid are skipped, not clamped.  A caller that works in chunks
    passes a window (the last `radius` frames before the chunk, the chunk, the first `radius` after it) and the chunk's range: the
    result equals the one-call result bit for bit.  No CPU path: raises CgsError without a GPU."""
    if not isinstance(z, torch.Tensor) or not isinstance(low, torch.Tensor):
        raise ValueError(f"z and low must be torch tensors, got {type(z).__name__} and {type(low).__name__}")
    if z.dtype != torch.float32 or z.dim() != 3 or tuple(z.shape[1:]) != (SIDE, SIDE) or z.shape[0] < 1:
        raise ValueError(f"z must be float32 [n,{SIDE},{SIDE}] with at least one frame, got {z.dtype} {tuple(z.shape)}")
    n = int(z.shape[0])
    if low.dtype != torch.uint8 or tuple(low.shape) != (n, SIDE, SIDE, 3):
        raise ValueError(f"low must be uint8 [{n},{SIDE},{SIDE},3], got {low.dtype} {tuple(low.shape)}")
    radius = check_radius(radius)
    _, sigma_r = check_sigmas(1.0, sigma_r)
    f1 = n if f1 is None else f1
    if not (isinstance(f0, (int, np.integer)) and isinstance(f1, (int, np.integer)) and 0 <= f0 < f1 <= n):
        raise ValueError(f"frames {f0}..{f1} are no range inside the {n} frames of the stack")
    _need_gpu("temporal.smooth (cgs_temporal_smooth)", z, low)
    z, low = z.contiguous(), low.contiguous()
    with torch.cuda.device(z.device):
        out = torch.empty((int(f1 - f0), SIDE, SIDE), dtype=torch.float32, device=z.device)
        _lib.call("cgs_temporal_smooth", z.data_ptr(), low.data_ptr(), n, int(f0), int(f1), radius, sigma_r, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out
