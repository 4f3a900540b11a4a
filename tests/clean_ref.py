"""The direct form of what cgs_mask_clean computes (include/cgs_hip.h), the checker of tests/test_clean_host.py and
tests/test_gpu_clean.py: per-pixel neighbourhood loops for the two structuring elements with the stated edge rule, a raster flood fill
with a stack for hysteresis and for the holes, the counts and `gated`, in plain Python on numpy arrays -- nothing of the kernel's bit
rows, shuffles or union-find, and no scipy."""
from collections import namedtuple

import numpy as np

from objects_ref import NEIGHBOURS, on_pixels

FIELDS = 8          # on after threshold, hyst, open, close, fill; components dropped by hyst, holes found, holes filled
ELEMENT = {"square": NEIGHBOURS[8], "cross": NEIGHBOURS[4]}
Cleaned = namedtuple("Cleaned", ["mask", "gated", "counts"])


def components(on, connectivity):
    """on: bool [h,w].  The components of the on pixels, each a list of (y, x), in raster order of their first pixel."""
    on = np.asarray(on, dtype=bool)
    h, w = on.shape
    seen = np.zeros((h, w), dtype=bool)
    out = []
    for y in range(h):
        for x in range(w):
            if not on[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            stack, pixels = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                pixels.append((cy, cx))
                for dy, dx in NEIGHBOURS[connectivity]:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and on[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            out.append(pixels)
    return out


def step(on, shape, erosion):
    """One iteration with the 3 x 3 square or the 5-pixel cross.  A dilated pixel is on when it or any neighbour inside the frame is
    on (outside is off); an eroded pixel is on when it and every neighbour inside the frame are on (outside is on)."""
    on = np.asarray(on, dtype=bool)
    h, w = on.shape
    out = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            near = [on[y, x]] + [on[y + dy, x + dx] for dy, dx in ELEMENT[shape] if 0 <= y + dy < h and 0 <= x + dx < w]
            out[y, x] = all(near) if erosion else any(near)
    return out


def erode(on, r, shape="square"):
    for _ in range(r):
        on = step(on, shape, True)
    return np.asarray(on, dtype=bool)


def dilate(on, r, shape="square"):
    for _ in range(r):
        on = step(on, shape, False)
    return np.asarray(on, dtype=bool)


def opening(on, r, shape="square"):
    return dilate(erode(on, r, shape), r, shape)


def closing(on, r, shape="square"):
    return erode(dilate(on, r, shape), r, shape)


def hysteresis(on, strong, connectivity=8):
    """on, strong: bool [h,w].  (kept bool [h,w], dropped): a component of `on` stays when it holds a pixel of `strong`."""
    on, strong = np.asarray(on, dtype=bool), np.asarray(strong, dtype=bool)
    kept, dropped = np.zeros_like(on), 0
    for pixels in components(on, connectivity):
        if any(strong[p] for p in pixels):
            for p in pixels:
                kept[p] = True
        else:
            dropped += 1
    return kept, dropped


def holes(on, connectivity=8):
    """The holes of a frame: the components of its OFF pixels at the complementary connectivity without a pixel in the first or last
    row or column, as lists of (y, x)."""
    on = np.asarray(on, dtype=bool)
    h, w = on.shape
    return [c for c in components(~on, 4 if connectivity == 8 else 8)
            if not any(y in (0, h - 1) or x in (0, w - 1) for y, x in c)]


def fill_holes(on, fill_area, connectivity=8):
    """(filled bool [h,w], holes found, holes filled): the holes of at most fill_area pixels are turned on."""
    out = np.array(on, dtype=bool)
    found = holes(out, connectivity)
    small = [c for c in found if len(c) <= fill_area]
    for c in small:
        for p in c:
            out[p] = True
    return out, len(found), len(small)


def clean_frame(src, thresh=None, inclusive=False, strong=None, open=0, close=0, fill=0, shape="square", connectivity=8):
    """src: [h,w].  (mask bool [h,w], counts int32 [8]) of one frame: on, hyst, open, close, fill in this order."""
    on = on_pixels(src, thresh, inclusive)
    counts = np.zeros(FIELDS, dtype=np.int32)
    counts[0] = on.sum()
    if strong is not None:
        on, counts[5] = hysteresis(on, on_pixels(src, strong, inclusive), connectivity)
    counts[1] = on.sum()
    if open:
        on = opening(on, open, shape)
    counts[2] = on.sum()
    if close:
        on = closing(on, close, shape)
    counts[3] = on.sum()
    if fill:
        on, counts[6], counts[7] = fill_holes(on, fill, connectivity)
    counts[4] = on.sum()
    return on, counts


def gate(src, mask, thresh, inclusive=False):
    """`gated`: 0 where mask is off; where it is on, the source value when it passes the threshold compare, thresh otherwise."""
    v = np.asarray(src, dtype=np.float32)
    passes = on_pixels(v, thresh, inclusive)
    return np.where(mask, np.where(passes, v, np.float32(thresh)), np.float32(0)).astype(np.float32)


def clean(src, thresh=None, inclusive=False, strong=None, open=0, close=0, fill=0, shape="square", connectivity=8,
          want_gated=False):
    """src: [n,h,w]; the keywords of cgs_amd.clean.clean.  Cleaned(mask bool [n,h,w], gated float32 [n,h,w] or None, counts int32 [n,8])."""
    src = np.asarray(src)
    frames = [clean_frame(f, thresh, inclusive, strong, open, close, fill, shape, connectivity) for f in src]
    mask = np.stack([f[0] for f in frames])
    return Cleaned(mask, gate(src, mask, thresh, inclusive) if want_gated else None, np.stack([f[1] for f in frames]))
