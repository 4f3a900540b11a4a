"""The direct forms of what cgs_temporal_flow and cgs_temporal_smooth_mc compute (include/cgs_hip.h), the checkers of
tests/test_temporal_motion_host.py and tests/test_gpu_temporal_motion.py.  Written from the formulas, not from the kernels: ``flow_ref`` in
integers with explicit loops over pairs, blocks and candidates in ranked order (no packed key, no staging), ``smooth_mc_ref`` in float64
after the integer colour distances with the path of every cell walked step by step and explicit validity masks (no apron, no clamped
reads that count, no base-2 folding).  ``smooth_mc_emul32`` is the same sum in float32 in the kernel's tap order (numpy's correctly
rounded exp instead of the hardware's exp2): what the tolerance of the GPU test is measured from.  ``pan`` builds the scenes both test
files share."""
import numpy as np

from temporal_ref import taps

SIDE, BLOCK, MAX_SEARCH = 64, 8, 4
BLOCKS = SIDE // BLOCK


def candidates(search):
    """The vectors (dy, dx), |dy|, |dx| <= search, in the order of the header: ascending dy^2 + dx^2, then dy, then dx."""
    return sorted(((dy, dx) for dy in range(-search, search + 1) for dx in range(-search, search + 1)),
                  key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))


def block_motion(src, dst, search):
    """int8 [8,8,2]: per block of `src` the candidate with the smallest SAD against `dst` displaced; a later candidate wins only with a
    strictly smaller SAD; a candidate counts only when the displaced block lies entirely inside the grid."""
    src, dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
    out = np.zeros((BLOCKS, BLOCKS, 2), dtype=np.int8)
    for by in range(BLOCKS):
        for bx in range(BLOCKS):
            y0, x0 = by * BLOCK, bx * BLOCK
            own = src[y0:y0 + BLOCK, x0:x0 + BLOCK]
            best = None
            for dy, dx in candidates(search):
                y, x = y0 + dy, x0 + dx
                if y < 0 or x < 0 or y + BLOCK > SIDE or x + BLOCK > SIDE:
                    continue
                sad = int(np.abs(own - dst[y:y + BLOCK, x:x + BLOCK]).sum())
                if best is None or sad < best:
                    best = sad
                    out[by, bx] = (dy, dx)
    return out


def flow_ref(low, search):
    """low uint8 [n,64,64,3] -> (fwd, bwd), int8 [n - 1,8,8,2]: fwd[g] from frame g to g + 1, bwd[g] from frame g + 1 to g."""
    low = np.asarray(low)
    n = len(low)
    assert low.shape == (n, SIDE, SIDE, 3) and low.dtype == np.uint8 and 1 <= search <= MAX_SEARCH
    fwd, bwd = np.zeros((n - 1, BLOCKS, BLOCKS, 2), dtype=np.int8), np.zeros((n - 1, BLOCKS, BLOCKS, 2), dtype=np.int8)
    for g in range(n - 1):
        fwd[g] = block_motion(low[g], low[g + 1], search)
        bwd[g] = block_motion(low[g + 1], low[g], search)
    return fwd, bwd


def path(fwd, bwd, f, k):
    """(my, mx), int64 [64,64] each: m_k of every cell of frame f.  m_0 = 0; m_{j+1} = m_j + field[block of p + m_j clamped into the
    grid], the field being fwd[f + j] for k > 0 and bwd[f - j - 1] for k < 0."""
    yy, xx = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    my, mx = np.zeros((SIDE, SIDE), dtype=np.int64), np.zeros((SIDE, SIDE), dtype=np.int64)
    for j in range(abs(k)):
        field = np.asarray(fwd[f + j] if k > 0 else bwd[f - j - 1]).astype(np.int64)
        qy, qx = np.clip(yy + my, 0, SIDE - 1), np.clip(xx + mx, 0, SIDE - 1)
        step = field[qy >> 3, qx >> 3]
        my, mx = my + step[..., 0], mx + step[..., 1]
    return my, mx


def _gather(plane, ty, tx):
    """plane[ty, tx] where (ty, tx) lies inside the grid (the value elsewhere is not used), and the mask of where it does."""
    ok = (ty >= 0) & (ty < SIDE) & (tx >= 0) & (tx < SIDE)
    return plane[np.clip(ty, 0, SIDE - 1), np.clip(tx, 0, SIDE - 1)], ok


def smooth_mc_ref(z, low, fwd, bwd, radius, sigma_r, f0=0, f1=None):
    """z [n,64,64] float, low uint8 [n,64,64,3], fwd / bwd int8 [n - 1,8,8,2] -> float64 [f1 - f0,64,64]."""
    z, low = np.asarray(z, dtype=np.float64), np.asarray(low).astype(np.int64)
    n = len(z)
    f1 = n if f1 is None else f1
    assert 1 <= radius <= 8 and sigma_r > 0 and 0 <= f0 < f1 <= n and low.shape == (n, SIDE, SIDE, 3)
    assert n == 1 or (np.shape(fwd) == (n - 1, BLOCKS, BLOCKS, 2) and np.shape(bwd) == (n - 1, BLOCKS, BLOCKS, 2))
    sigma_t = radius / 2.0
    yy, xx = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    out = np.empty((f1 - f0, SIDE, SIDE))
    for f in range(f0, f1):
        num, den, at = z[f].copy(), np.ones((SIDE, SIDE)), None        # the centre tap: weight exactly 1
        for k, dy, dx in taps(radius):
            g = f + k
            if not 0 <= g < n:
                continue                                               # a frame outside the stack is skipped
            if at != k:                                                # (the path depends on k alone)
                at, (my, mx) = k, path(fwd, bwd, f, k)
            zg, ok = _gather(z[g], yy + my + dy, xx + mx + dx)
            lg, _ = _gather(low[g], yy + my + dy, xx + mx + dx)
            d2 = ((lg - low[f]) ** 2).sum(axis=-1)
            w = np.where(ok, np.exp(-(k * k / (2.0 * sigma_t ** 2) + (dy * dy + dx * dx) / 2.0 + d2 / (2.0 * sigma_r ** 2))), 0.0)
            num += w * zg
            den += w
        out[f - f0] = num / den
    return out


def smooth_mc_emul32(z, low, fwd, bwd, radius, sigma_r):
    """The same in float32, tap by tap in the kernel's order: the exponent as fl(d2 cr + fl(k^2 ct + (ey + ex))) (two fused multiply-adds,
    ey + ex exact), w rounded to float32, num = fl(w z + num), den = fl(den + w), out = fl(num / den).  float32 [n,64,64]."""
    z, low = np.asarray(z, dtype=np.float32), np.asarray(low).astype(np.int64)
    n = len(z)
    f32, f64 = np.float32, np.float64
    log2e = 1.4426950408889634
    cr, ct, cs = f32(log2e / (2.0 * sigma_r ** 2)), f32(log2e / (2.0 * (radius / 2.0) ** 2)), f32(log2e / 2.0)
    yy, xx = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    out = np.empty((n, SIDE, SIDE), dtype=np.float32)
    for f in range(n):
        num, den, at = z[f].copy(), np.ones((SIDE, SIDE), dtype=np.float32), None
        for k, dy, dx in taps(radius):
            g = f + k
            if not 0 <= g < n:
                continue
            if at != k:                                                # (the path depends on k alone)
                at, (my, mx) = k, path(fwd, bwd, f, k)
            zg, ok = _gather(z[g], yy + my + dy, xx + mx + dx)
            lg, _ = _gather(low[g], yy + my + dy, xx + mx + dx)
            d2 = ((lg - low[f]) ** 2).sum(axis=-1).astype(np.float32)
            space = f32(f32(dy * dy) * cs + f32(dx * dx) * cs)                                         # 0, cs or 2 cs: exact
            rest = f32(f64(f32(k * k)) * f64(ct) + f64(space))                                         # one rounding: the fma
            arg = (d2.astype(f64) * f64(cr) + f64(rest)).astype(np.float32)                            # one rounding: the fma
            w = np.where(ok, np.exp2(-arg.astype(f64)).astype(np.float32), f32(0.0))
            num = (w.astype(f64) * zg.astype(f64) + num.astype(f64)).astype(np.float32)
            den = den + w
        out[f] = num / den
    return out


def pan(n, dy, dx, seed, noise=6, flicker=0.0, texture=False):
    """A camera pan: (z float32 [n,64,64], low uint8 [n,64,64,3], clean float32 [n,64,64]).  A canvas of blocks of random colour and
    mask value, 5 to 23 cells a side and not aligned to anything (every cell its own colour with `texture`), seen through a window that
    moves so that low[g + 1][q + (dy, dx)] = low[g][q]: the true forward vector is (dy, dx) everywhere.  The colours get +-noise per frame,
    `clean` is the mask value (0.15 .. 0.85) without flicker and z = clean +- flicker, the sign alternating from frame to frame."""
    rs = np.random.RandomState(seed)
    by, bx = (1, 1) if texture else rs.randint(5, 24, 2)
    h, w = SIDE + (n - 1) * abs(dy), SIDE + (n - 1) * abs(dx)
    hh, ww = h // by + 2, w // bx + 2
    colour = np.repeat(np.repeat(rs.randint(0, 256, (hh, ww, 3)), by, axis=0), bx, axis=1)
    value = np.repeat(np.repeat(0.15 + 0.7 * rs.rand(hh, ww), by, axis=0), bx, axis=1)
    oy, ox = rs.randint(0, by) + (n - 1) * max(dy, 0), rs.randint(0, bx) + (n - 1) * max(dx, 0)
    low = np.stack([colour[oy - g * dy:oy - g * dy + SIDE, ox - g * dx:ox - g * dx + SIDE] for g in range(n)])
    clean = np.stack([value[oy - g * dy:oy - g * dy + SIDE, ox - g * dx:ox - g * dx + SIDE] for g in range(n)]).astype(np.float32)
    if noise:
        low = low + rs.randint(-noise, noise + 1, low.shape)
    low = np.clip(low, 0, 255).astype(np.uint8)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None, None]
    z = np.clip(clean + flicker * sign, 0.0, 1.0).astype(np.float32)
    return z, low, clean
