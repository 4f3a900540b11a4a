"""Masks smoothed along time for ``-process --source-video --smooth R`` (csrc/temporal.hip).  The network sees one frame at a time, so
its masks flicker when they are played as a video; ``smooth`` is a spatio-temporal joint bilateral filter over the stack of 64 x 64 masks,
guided by the shrunk frames (``fit.down``): a cell is averaged with the 3 x 3 cells around it in the R frames before and after, each
weighted by a Gaussian in time (sigma_t = R / 2), in space (sigma 1 cell) and in the colour distance to the cell's own colour (sigma_r).
By default the taps of every frame sit around the cell's own position -- the 3 x 3 search and the range term stand in for a motion
model: a cell whose colour changed gets no weight from the other frame.  With ``motion=flow(low, S)`` (``--smooth-motion S``,
csrc/temporal_motion.hip) the taps follow block-matched motion: one integer vector per 8 x 8-cell block and pair of neighbouring frames,
up to S <= 4 cells a frame, chained over the |k| frames between a tap and its cell.  That compensates translation by whole cells (a
camera pan); it does not compensate motion inside a block, motion of a fraction of a cell, or occlusion -- there the range term is what is
left.  Runs on the GPU only; ``check_radius`` / ``check_search`` / ``sigma_t`` are the pure host helpers.

The default sigma_r = 16 colour units is the same judgement as ``fit.SIGMA_RANGE``, not a tuned result; so are the block of 8 cells and
the search limit of 4 cells of the motion."""
import numpy as np
import torch

from . import _lib
from .fit import _need_gpu, check_sigmas

SIDE, MAX_RADIUS = _lib.TEMPORAL_SIDE, _lib.TEMPORAL_MAX_RADIUS
BLOCK, MAX_SEARCH = _lib.TEMPORAL_BLOCK, _lib.TEMPORAL_MAX_SEARCH
BLOCKS = SIDE // BLOCK
SIGMA_RANGE = 16.0


def check_radius(radius, least=1, name="radius"):
    """radius as an int; ValueError unless it is a whole number in least..8."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {radius!r}")
    if not least <= radius <= MAX_RADIUS:
        raise ValueError(f"{name} = {radius}: {least} to {MAX_RADIUS} frames each way")
    return int(radius)


def check_search(search, least=1, name="search"):
    """search as an int; ValueError unless it is a whole number in least..4."""
    if isinstance(search, bool) or not isinstance(search, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {search!r}")
    if not least <= search <= MAX_SEARCH:
        raise ValueError(f"{name} = {search}: {least} to {MAX_SEARCH} cells each way")
    return int(search)


def sigma_t(radius):
    """The temporal sigma in frames: the window of +-radius frames is +-2 sigma."""
    return check_radius(radius) / 2.0


def flow(low, search=MAX_SEARCH):
    """low: device tensor uint8 [n,64,64,3] = fit.down of the frames.  search S = 1..4 cells.  Returns (fwd, bwd), int8 [n - 1,8,8,2] on
    low's device, components (dy, dx): fwd[g][by][bx] is the d with |dy|, |dx| <= S whose displaced block lies inside the grid that
    minimises the integer sum of |low[g][q] - low[g + 1][q + d]| over the 64 cells q of block (by, bx) and the three colours; bwd[g] is
    the same from frame g + 1 to frame g (not the negation of fwd).  Equal sums go to the candidate first by (dy^2 + dx^2, dy, dx): the
    smallest motion, and all zeros on constant frames.  A vector depends on its two frames only.  One frame gives [0,8,8,2] without a
    launch.  No CPU path: raises CgsError without a GPU."""
    if not isinstance(low, torch.Tensor):
        raise ValueError(f"low must be a torch tensor, got {type(low).__name__}")
    if low.dtype != torch.uint8 or low.dim() != 4 or tuple(low.shape[1:]) != (SIDE, SIDE, 3) or low.shape[0] < 1:
        raise ValueError(f"low must be uint8 [n,{SIDE},{SIDE},3] with at least one frame, got {low.dtype} {tuple(low.shape)}")
    search = check_search(search)
    _need_gpu("temporal.flow (cgs_temporal_flow)", low)
    n = int(low.shape[0])
    low = low.contiguous()
    with torch.cuda.device(low.device):
        fwd = torch.empty((n - 1, BLOCKS, BLOCKS, 2), dtype=torch.int8, device=low.device)
        bwd = torch.empty_like(fwd)
        if n > 1:
            _lib.call("cgs_temporal_flow", low.data_ptr(), n, search, fwd.data_ptr(), bwd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return fwd, bwd


def _check_motion(motion, n, device):
    """(fwd, bwd) of flow(), contiguous; ValueError unless both are int8 [n - 1,8,8,2] on `device`."""
    if not isinstance(motion, (tuple, list)) or len(motion) != 2 or not all(isinstance(m, torch.Tensor) for m in motion):
        raise ValueError("motion must be the pair (fwd, bwd) of torch tensors that temporal.flow returns")
    want = (n - 1, BLOCKS, BLOCKS, 2)
    for name, m in zip(("fwd", "bwd"), motion):
        if m.dtype != torch.int8 or tuple(m.shape) != want:
            raise ValueError(f"motion {name} must be int8 {list(want)}, got {m.dtype} {tuple(m.shape)}")
        if m.device != device:
            raise ValueError(f"motion {name} is on {m.device}, z on {device}")
    return motion[0].contiguous(), motion[1].contiguous()


def smooth(z, low, radius, sigma_r=SIGMA_RANGE, f0=0, f1=None, motion=None):
    """z: device tensor float32 [n,64,64] in [0,1].  low: uint8 [n,64,64,3] = fit.down of the frames.  radius 1..8, sigma_r > 0.
    Returns float32 [f1 - f0,64,64], frames f0 <= f < f1 of the smoothed stack (all of it by default), on the inputs' device.
    For frame f and cell p: the centre tap (f, p) with weight exactly 1, then k = -radius .. -1, 1 .. radius, frame g = f + k when
    0 <= g < n, the 3 x 3 cells p + (dy, dx) inside the grid (dy outer, dx inner), w = exp(-(k^2 / (2 sigma_t^2) + (dy^2 + dx^2) / 2 +
    d2 / (2 sigma_r^2))) with d2 the integer squared colour distance of low[g][p + (dy, dx)] and low[f][p]; out = sum w z / sum w in
    float32 in that order.  Frames outside the stack and cells outside the grid are skipped, not clamped.  A caller that works in chunks
    passes a window (the last `radius` frames before the chunk, the chunk, the first `radius` after it) and the chunk's range: the
    result equals the one-call result bit for bit.  motion = (fwd, bwd) of flow(low, S) (of the same window): the taps of frame f + k sit
    around p + m_k instead of p, m_0 = 0 and m_{j+1} = m_j + fwd[f + j][block of p + m_j clamped into the grid] (bwd[f - j - 1] for k < 0);
    d2 stays the distance to low[f][p] and the spatial term counts (dy, dx) only (cgs_temporal_smooth_mc).  All-zero fields give the
    result without motion bit for bit.  No CPU path: raises CgsError without a GPU."""
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
    if motion is not None:
        fwd, bwd = _check_motion(motion, n, z.device)
    _need_gpu("temporal.smooth (cgs_temporal_smooth)", z, low)
    z, low = z.contiguous(), low.contiguous()
    with torch.cuda.device(z.device):
        out = torch.empty((int(f1 - f0), SIDE, SIDE), dtype=torch.float32, device=z.device)
        if motion is None:
            _lib.call("cgs_temporal_smooth", z.data_ptr(), low.data_ptr(), n, int(f0), int(f1), radius, sigma_r, out.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        else:
            _lib.call("cgs_temporal_smooth_mc", z.data_ptr(), low.data_ptr(), fwd.data_ptr(), bwd.data_ptr(), n, int(f0), int(f1), radius,
                      sigma_r, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out
