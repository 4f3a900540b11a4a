"""The direct form of what cgs_objects_label computes (include/cgs_hip.h), the checker of tests/test_objects_host.py and
tests/test_gpu_objects.py: a raster scan that flood-fills every unvisited on pixel with a stack, in plain Python on numpy arrays --
nothing of the kernel's runs, union-find or ballots.  A component found by the scan is found at its first pixel, so numbering the
kept ones in the order of discovery is the numbering of scipy.ndimage.label."""
import numpy as np

FIELDS = 8          # area, x0, y0, x1, y1, sum_x, sum_y, first
NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def on_pixels(src, thresh=None, inclusive=False):
    """The on mask of a stack: non-zero for bool / uint8, the float32 compare with a float32 threshold otherwise (a NaN is off)."""
    src = np.asarray(src)
    if thresh is None:
        return src != 0
    with np.errstate(invalid="ignore"):
        v, t = src.astype(np.float32), np.float32(thresh)
        return (v >= t) if inclusive else (v > t)


def label_frame(on, connectivity=8, min_area=1, max_objects=64):
    """on: bool [h,w].  Returns (labels int32 [h,w], kept_mask bool [h,w], kept, found, table int32 [max_objects,8])."""
    on = np.asarray(on, dtype=bool)
    h, w = on.shape
    steps = NEIGHBOURS[connectivity]
    seen = np.zeros((h, w), dtype=bool)
    labels = np.zeros((h, w), dtype=np.int32)
    table = np.zeros((max_objects, FIELDS), dtype=np.int32)
    kept = found = 0
    for y in range(h):
        for x in range(w):
            if not on[y, x] or seen[y, x]:
                continue
            found += 1
            seen[y, x] = True
            stack, pixels = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                pixels.append((cy, cx))
                for dy, dx in steps:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and on[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            if len(pixels) < min_area:
                continue
            kept += 1
            ys, xs = np.array([p[0] for p in pixels]), np.array([p[1] for p in pixels])
            labels[ys, xs] = kept
            if kept <= max_objects:
                table[kept - 1] = [len(pixels), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum(), y * w + x]
    return labels, labels != 0, kept, found, table


def label(on, connectivity=8, min_area=1, max_objects=64):
    """on: bool [n,h,w].  Returns (labels int32 [n,h,w], kept_mask bool [n,h,w], kept int32 [n], found int32 [n],
    table int32 [n,max_objects,8])."""
    frames = [label_frame(f, connectivity, min_area, max_objects) for f in np.asarray(on)]
    return (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.array([f[2] for f in frames], dtype=np.int32),
            np.array([f[3] for f in frames], dtype=np.int32), np.stack([f[4] for f in frames]))


# ---------------------------------------------------------------------------------------------------------------- the test patterns
def spiral(n=64):
    """A one-pixel line winding inwards with one-pixel gaps: one component at both connectivities, 2111 pixels at n = 64."""
    a = np.zeros((n, n), dtype=bool)
    y, x, (dy, dx) = 0, 0, (0, 1)
    a[0, 0] = True

    def touching(cy, cx):                      # on 4-neighbours of (cy, cx)
        return sum(bool(a[cy + sy, cx + sx]) for sy, sx in NEIGHBOURS[4] if 0 <= cy + sy < n and 0 <= cx + sx < n)

    while True:
        for _ in range(2):                     # go on, or turn right once; a step may touch nothing but the pixel it comes from
            ny, nx = y + dy, x + dx
            if 0 <= ny < n and 0 <= nx < n and not a[ny, nx] and touching(ny, nx) == 1:
                y, x = ny, nx
                a[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return a


def comb(h=64, w=64):
    a = np.zeros((h, w), dtype=bool)
    a[:, ::2] = True
    a[h - 1] = True
    return a


def serpentine(h=64, w=64):
    a = np.zeros((h, w), dtype=bool)
    a[::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        a[y, w - 1 if k % 2 == 0 else 0] = True
    return a


def checkerboard(h=64, w=64):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys + xs) % 2 == 0


def randoms():
    """The four random 64 x 64 frames, p = 0.3, 0.45, 0.593, 0.7, drawn in this order from one RandomState(0)."""
    rs = np.random.RandomState(0)
    return [rs.rand(64, 64) < p for p in (0.3, 0.45, 0.593, 0.7)]


def patterns():
    """name -> bool [64,64]."""
    out = {"spiral": spiral(), "comb": comb(), "serpentine": serpentine(), "checkerboard": checkerboard(),
           "full": np.ones((64, 64), dtype=bool), "empty": np.zeros((64, 64), dtype=bool)}
    out.update({f"random{p}": r for p, r in zip(("0.3", "0.45", "0.593", "0.7"), randoms())})
    return out
