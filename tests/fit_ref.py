"""The direct form of what cgs_fit_down_u8 and cgs_fit_up_joint compute (include/cgs_hip.h), the checker of tests/test_fit_host.py and
tests/test_gpu_fit.py.  Written from the formulas, not from the kernels: the box average is two dense integer matrix products over the
explicit overlap tables in int64 (object integers where the sum could pass 2^63: never at these sizes, asserted), the joint filter loops
over the 25 taps on whole float64 planes with explicit validity masks -- no column sums, no staging, no base-2 folding, no sentinel."""
import numpy as np

SIDE, RADIUS = 64, 2


def overlap(L):
    """int64 [64, L]: the length of the overlap of [L o, L o + L) and [64 s, 64 s + 64), by counting units (no min / max formula)."""
    if L < SIDE:
        raise ValueError("L >= 64")
    unit_cell = np.arange(SIDE * L, dtype=np.int64) // L             # the cell of each of the 64 L units of the axis
    unit_pixel = np.arange(SIDE * L, dtype=np.int64) // SIDE
    table = np.zeros((SIDE, L), dtype=np.int64)
    np.add.at(table, (unit_cell, unit_pixel), 1)
    return table


def down_ref(frames):
    """uint8 [n,H,W,3] -> uint8 [n,64,64,3]: (2 S + H W) // (2 H W), S = overlap(H) @ v @ overlap(W).T per channel, in int64."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    n, H, W, _ = frames.shape
    assert 255 * H * W * 2 + H * W < 2 ** 62
    wy, wx = overlap(H), overlap(W)
    S = np.einsum("oy,nyxc,px->nopc", wy, frames.astype(np.int64), wx, optimize=True)
    return ((2 * S + H * W) // (2 * H * W)).astype(np.uint8)


def home(L):
    return ((2 * np.arange(L, dtype=np.int64) + 1) * 32) // L


def up_ref(values, guide, low, sigma_s, sigma_r):
    """values [n,64,64] (float, or integer / bool labels: non-zero = 1), guide uint8 [n,H,W,3], low uint8 [n,64,64,3] -> float64 [n,H,W],
    the joint bilateral upsampling of the header, everything after the integer distances in float64."""
    values = np.asarray(values)
    m = values.astype(np.float64) if values.dtype.kind == "f" else (values != 0).astype(np.float64)
    guide, low = np.asarray(guide).astype(np.int64), np.asarray(low).astype(np.int64)
    n, H, W, _ = guide.shape
    qy0, qx0 = home(H), home(W)
    ys, xs = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    taps = []
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            qy, qx = qy0 + dy, qx0 + dx
            ok = ((qy >= 0) & (qy < SIDE))[:, None] & ((qx >= 0) & (qx < SIDE))[None, :]                  # [H,W]
            cy, cx = np.clip(qy, 0, SIDE - 1), np.clip(qx, 0, SIDE - 1)                                   # only to index; masked by ok
            fy = ((2 * ys + 1) * 64 - H * (2 * qy + 1)) / (2.0 * H)
            fx = ((2 * xs + 1) * 64 - W * (2 * qx + 1)) / (2.0 * W)
            ds = fy[:, None] ** 2 + fx[None, :] ** 2
            d2 = ((guide - low[:, cy][:, :, cx]) ** 2).sum(axis=-1)                                        # [n,H,W] int64
            taps.append((ok, ds, d2, m[:, cy][:, :, cx]))
    big = np.iinfo(np.int64).max
    d2_min = np.min([np.where(ok[None], d2, big) for ok, _, d2, _ in taps], axis=0)
    num, den = np.zeros((n, H, W)), np.zeros((n, H, W))
    for ok, ds, d2, mv in taps:
        rel = np.where(ok[None], d2 - d2_min, 0)                    # >= 0 on every valid tap; a skipped tap's own value is never used
        w = np.where(ok[None], np.exp(-(ds[None] / (2.0 * sigma_s ** 2) + rel / (2.0 * sigma_r ** 2))), 0.0)
        num += w * mv
        den += w
    return num / den


def nearest_ref(values, H, W):
    """[n,64,64] -> [n,H,W]: every pixel takes its home cell's value (what the filter is compared with)."""
    values = np.asarray(values)
    return values[:, home(H)][:, :, home(W)]
