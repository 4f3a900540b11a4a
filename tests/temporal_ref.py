"""The direct form of what cgs_temporal_smooth computes (include/cgs_hip.h), the checker of tests/test_temporal_host.py and
tests/test_gpu_temporal.py.  Written from the formula, not from the kernel: float64 throughout after the integer colour distances, explicit
loops over the taps on whole planes with explicit validity masks -- no staging, no apron, no base-2 folding.  ``smooth_emul32`` is the same
sum in float32 in the kernel's tap order (numpy's correctly rounded exp instead of the hardware's exp2): what the tolerance of the GPU test
is measured from."""
import numpy as np

SIDE = 64


def taps(radius):
    """The taps after the centre tap, in the order of the header: k ascending without 0, then dy, then dx."""
    return [(k, dy, dx) for k in list(range(-radius, 0)) + list(range(1, radius + 1)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _shifted(plane, dy, dx, fill=0):
    """out[y, x] = plane[y + dy, x + dx] where that lies inside the plane, `fill` elsewhere; and the mask of where it does."""
    h, w = plane.shape[:2]
    out = np.full_like(plane, fill)
    ok = np.zeros((h, w), dtype=bool)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[yd, xd] = plane[ys, xs]
    ok[yd, xd] = True
    return out, ok


def smooth_ref(z, low, radius, sigma_r, f0=0, f1=None):
    """z [n,64,64] float, low uint8 [n,64,64,3] -> float64 [f1 - f0,64,64]."""
    z, low = np.asarray(z, dtype=np.float64), np.asarray(low).astype(np.int64)
    n = len(z)
    f1 = n if f1 is None else f1
    assert 1 <= radius <= 8 and sigma_r > 0 and 0 <= f0 < f1 <= n and low.shape == (n, SIDE, SIDE, 3)
    sigma_t = radius / 2.0
    out = np.empty((f1 - f0, SIDE, SIDE))
    for f in range(f0, f1):
        num, den = z[f].copy(), np.ones((SIDE, SIDE))                  # the centre tap: weight exactly 1
        for k, dy, dx in taps(radius):
            g = f + k
            if not 0 <= g < n:
                continue                                               # a frame outside the stack is skipped
            zg, ok = _shifted(z[g], dy, dx)
            lg, _ = _shifted(low[g], dy, dx)
            d2 = ((lg - low[f]) ** 2).sum(axis=-1)
            w = np.where(ok, np.exp(-(k * k / (2.0 * sigma_t ** 2) + (dy * dy + dx * dx) / 2.0 + d2 / (2.0 * sigma_r ** 2))), 0.0)
            num += w * zg
            den += w
        out[f - f0] = num / den
    return out


def smooth_emul32(z, low, radius, sigma_r):
    """The same in float32, tap by tap in the kernel's order: w rounded to float32, num = fl(w z + num) (the product exact in float64,
    one rounding: a fused multiply-add), den = fl(den + w), out = fl(num / den).  float32 [n,64,64]."""
    z, low = np.asarray(z, dtype=np.float32), np.asarray(low).astype(np.int64)
    n = len(z)
    f32 = np.float32
    log2e = 1.4426950408889634
    cr, ct, cs = f32(log2e / (2.0 * sigma_r ** 2)), f32(log2e / (2.0 * (radius / 2.0) ** 2)), f32(log2e / 2.0)
    out = np.empty((n, SIDE, SIDE), dtype=np.float32)
    for f in range(n):
        num, den = z[f].copy(), np.ones((SIDE, SIDE), dtype=np.float32)
        for k, dy, dx in taps(radius):
            g = f + k
            if not 0 <= g < n:
                continue
            zg, ok = _shifted(z[g], dy, dx)
            lg, _ = _shifted(low[g], dy, dx)
            d2 = ((lg - low[f]) ** 2).sum(axis=-1).astype(np.float32)
            rest = f32(f32(k * k) * ct) + f32(f32(dy * dy) * cs + f32(dx * dx) * cs)
            arg = (d2.astype(np.float64) * np.float64(cr) + np.float64(rest)).astype(np.float32)          # one rounding: the fma
            w = np.where(ok, np.exp2(-arg.astype(np.float64)).astype(np.float32), f32(0.0))
            num = (w.astype(np.float64) * zg.astype(np.float64) + num.astype(np.float64)).astype(np.float32)
            den = den + w
        out[f] = num / den
    return out
