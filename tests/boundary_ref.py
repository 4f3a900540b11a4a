"""The direct form of what cgs_boundary_score computes (include/cgs_hip.h), the checker of tests/test_boundary_host.py and
tests/test_gpu_boundary.py.  Deliberately not the kernel's algorithm: the boundary comes from neighbour lookups on a zero-padded array,
a distance is the minimum over the explicit list of boundary pixel coordinates in exact integers, and the counts are
plain sums -- no bit rows, no separable transform, no ballots."""
import numpy as np


def boundary(mask):
    """mask bool [h,w] -> bool [h,w]: on, and at least one of the four neighbours off; outside the frame is off."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = mask
    up, down, left, right = pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]
    return mask & ~(up & down & left & right)


def dist2(bnd):
    """bnd bool [h,w] -> int64 [h,w]: the squared Euclidean distance of every pixel to the nearest True pixel, -1 everywhere when there
    is none.  The minimum over the list of True pixels (256 of the list at a time, to bound the memory)."""
    bnd = np.asarray(bnd, dtype=bool)
    h, w = bnd.shape
    ys, xs = (v.astype(np.int32) for v in np.nonzero(bnd))
    if ys.size == 0:
        return np.full((h, w), -1, dtype=np.int64)
    if 2 * max(h, w) ** 2 >= 2 ** 31:
        raise ValueError("a frame this large does not fit the int32 arithmetic below")
    best = np.full((h, w), np.iinfo(np.int32).max, dtype=np.int32)
    for lo in range(0, ys.size, 256):
        dy2 = (np.arange(h, dtype=np.int32)[None, :] - ys[lo:lo + 256, None]) ** 2          # [k,h]
        dx2 = (np.arange(w, dtype=np.int32)[None, :] - xs[lo:lo + 256, None]) ** 2          # [k,w]
        best = np.minimum(best, (dy2[:, :, None] + dx2[:, None, :]).min(axis=0))
    return best.astype(np.int64)


def score_frame(pred, truth, tol2):
    """pred, truth: bool [h,w]; tol2: squared tolerances (integers).  Returns (counts int32 [4 + 4 T], dist2 int32 [2,h,w])."""
    pred, truth = np.asarray(pred, dtype=bool), np.asarray(truth, dtype=bool)
    bp, bt = boundary(pred), boundary(truth)
    dp, dt = dist2(bp), dist2(bt)
    n_p, n_t = int(bp.sum()), int(bt.sum())
    counts = [n_p, n_t, -1, -1]
    if n_p and n_t:
        counts[2], counts[3] = int(dt[bp].max()), int(dp[bt].max())
    for q in tol2:
        q = int(q)
        near_p = (dp <= q) & (dp >= 0)                                     # an empty boundary is near nothing
        near_t = (dt <= q) & (dt >= 0)
        P, G = pred & near_p, truth & near_t
        counts += [int((bp & near_t).sum()), int((bt & near_p).sum()), int((P & G).sum()), int((P | G).sum())]
    return np.array(counts, dtype=np.int32), np.stack([dp, dt]).astype(np.int32)


def score(pred, truth, tol2):
    """pred, truth: bool [n,h,w].  Returns (counts int32 [n, 4 + 4 T], dist2 int32 [n,2,h,w])."""
    frames = [score_frame(p, t, tol2) for p, t in zip(np.asarray(pred), np.asarray(truth))]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])


def split_counts(counts):
    """counts [n, 4 + 4 T] -> pred_px, truth_px, hd2_pred, hd2_truth [n] and hit_pred, hit_truth, band_inter, band_union [n,T]."""
    counts = np.asarray(counts)
    per = counts[:, 4:].reshape(counts.shape[0], -1, 4)
    return tuple(counts[:, i] for i in range(4)) + tuple(per[:, :, i] for i in range(4))


def on_pixels(src, thresh=None, inclusive=False):
    """The on-mask of a stack as the kernel reads it: non-zero for integer / bool stacks, a float32 compare otherwise (NaN is off)."""
    src = np.asarray(src)
    if thresh is None:
        return src != 0
    with np.errstate(invalid="ignore"):
        return (src.astype(np.float32) >= np.float32(thresh)) if inclusive else (src.astype(np.float32) > np.float32(thresh))


# ---------------------------------------------------------------------------------------------------------------- hand-made frames
def hand_made():
    """[(name, pred, truth)] bool [64,64], the frames of the tests' hand-made cases."""
    z = lambda: np.zeros((64, 64), dtype=bool)
    full = np.ones((64, 64), dtype=bool)
    frames = [("both_empty", z(), z()), ("empty_vs_full", z(), full.copy()), ("full_vs_empty", full.copy(), z()),
              ("full_vs_full", full.copy(), full.copy())]
    a, b = z(), z()
    a[0, 0], b[63, 63] = True, True
    frames.append(("corners", a, b))
    a, b = z(), z()
    a[20:23, 30:33], b[20:23, 31:34] = True, True
    frames.append(("block_shifted", a, b))
    ys, xs = np.mgrid[0:64, 0:64]
    checker = (ys + xs) % 2 == 0
    frames.append(("checkerboard", checker, ~checker))
    edge, col = z(), z()                                                   # every boundary pixel of this frame sits in row 63 or
    edge[63, :], edge[:, 63] = True, True                                  # column 63: the last ballot bit and the last row
    col[40:, 63] = True
    frames.append(("last_row_and_column", edge, col))
    return frames
