"""Dense-CRF mask refinement (the reference's ``-crf``, main.py:1226-1263): two labels, Potts compatibility, the exact
fully-connected mean field on the GPU (``cgs_dense_crf2``, csrc/crf.hip).  The model is stated in include/cgs_hip.h and
INTEGRATION.md; it is the one SimpleCRF's ``densecrf(I, P, param)`` sets up, computed without the permutohedral lattice."""
import ctypes

import torch

from . import _lib

# (w_bilateral, alpha, beta, w_gaussian, gamma, iterations): the one-point grid of Handler.crf (main.py:1230-1235)
REFERENCE_PARAMS = (22, 12, 3.1, 8, 1.8, 10)
# the names of the reference's six lists (main.py:1230-1235), in the nesting order of its product (main.py:1238): w1 outermost
GRID_KEYS = ("w1", "alpha", "beta", "w2", "gamma", "it")


def parse_crf_grid(s):
    """``--crf-grid "w1=5,22;alpha=12;it=2,10"`` -> {key: [values]} over all six GRID_KEYS; a key not given keeps its one
    REFERENCE_PARAMS value.  `it` takes integers >= 0, the stds (alpha, beta, gamma) positive numbers.  An empty string is the
    reference's one-point grid."""
    grid = {k: [v] for k, v in zip(GRID_KEYS, REFERENCE_PARAMS)}
    seen = set()
    for item in filter(None, (part.strip() for part in str(s).split(";"))):
        key, eq, vals = item.partition("=")
        key = key.strip()
        if not eq or key not in GRID_KEYS:
            raise ValueError(f"--crf-grid {item!r}: expected KEY=v1,v2,... with KEY one of {', '.join(GRID_KEYS)}")
        if key in seen:
            raise ValueError(f"--crf-grid: {key} is given twice")
        seen.add(key)
        out = []
        for tok in vals.split(","):
            tok = tok.strip()
            try:
                v = int(tok)
            except ValueError:
                try:
                    v = float(tok)
                except ValueError:
                    raise ValueError(f"--crf-grid {item!r}: {tok!r} is not a number") from None
                if key == "it":
                    raise ValueError(f"--crf-grid {item!r}: it takes whole numbers") from None
            if v != v or v in (float("inf"), float("-inf")):
                raise ValueError(f"--crf-grid {item!r}: {tok!r} is not finite")
            if (key == "it" and v < 0) or (key in ("alpha", "beta", "gamma") and v <= 0):
                raise ValueError(f"--crf-grid {item!r}: {key} must be {'>= 0' if key == 'it' else 'positive'}")
            out.append(v)
        grid[key] = out
    return grid


def grid_points(grid):
    """The points of a parse_crf_grid() dict in the reference's product order (main.py:1238): w1 outermost, `it` innermost."""
    w1, alpha, beta, w2, gamma, it = (grid[k] for k in GRID_KEYS)
    return [(a, b, c, d, e, i) for a in w1 for b in alpha for c in beta for d in w2 for e in gamma for i in it]


def dense_crf(frames_u8, prob1, params=REFERENCE_PARAMS, return_q=False):
    """frames_u8: device uint8 [n,h,w,3]; prob1: device fp32 [n,h,w] = P(label 1).  Returns the uint8 labels [n,h,w] (and, with
    return_q, Q(label 1) fp32 [n,h,w] after the last mean-field step).  h * w <= 16384.  No CPU path: raises CgsError without a GPU."""
    if not torch.cuda.is_available():
        raise _lib.CgsError("dense_crf runs on the GPU (cgs_dense_crf2); no GPU is visible and there is no CPU fallback")
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError(f"frames_u8 must be uint8 [n,h,w,3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    n, h, w, _ = frames_u8.shape
    if tuple(prob1.shape) != (n, h, w) or prob1.dtype != torch.float32:
        raise ValueError(f"prob1 must be float32 [{n},{h},{w}], got {prob1.dtype} {tuple(prob1.shape)}")
    if not (frames_u8.is_cuda and prob1.is_cuda and frames_u8.device == prob1.device):
        raise ValueError("frames_u8 and prob1 must be on the same GPU")
    w1, alpha, beta, w2, gamma, it = params
    prm = _lib.CrfParams(float(w1), float(alpha), float(beta), float(w2), float(gamma), int(it))
    frames_u8, prob1 = frames_u8.contiguous(), prob1.contiguous()
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=frames_u8.device)
    q = torch.empty((n, h, w), dtype=torch.float32, device=frames_u8.device) if return_q else None
    if n:
        with torch.cuda.device(frames_u8.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.call("cgs_dense_crf2", frames_u8.data_ptr(), prob1.data_ptr(), n, h, w, ctypes.byref(prm), labels.data_ptr(),
                      q.data_ptr() if return_q else None, stream)
    return (labels, q) if return_q else labels
