"""The direct form of what cgs_overlay_compose_tracks_carried computes (include/cgs_hip.h), the checker of tests/test_overlay_fill_host.py,
tests/test_gpu_overlay_fill.py and tests/test_gpu_process_video_fill.py: tests/overlay_tracks_ref.py's pixel rules with the hatching of
the carried objects (age > 0), in Python integers and loops over pixels.  What the hatching leaves alone -- the object of a pixel, the
colours, the plate, the outline, the layouts -- is taken from overlay_tracks_ref and overlay_ref."""
import numpy as np

import overlay_ref
import overlay_tracks_ref as otr


def on_stripe(y, x, s):
    """Pixel (y, x) of the overlay panel at plate scale s."""
    return ((int(x) + int(y)) // (2 * int(s))) & 1 == 0


def decoration_of_pixel(tab, ids, age, K, y, x, H, W, B, font):
    """overlay_tracks_ref.decoration_of_pixel with the carried objects' borders hatched: the plates are whole; off the stripe a carried
    object has no border, and the later labels' borders (and, for the caller, outline and tint) apply."""
    if B <= 0:
        return None
    s = otr.scale(H, W)
    live = [l for l in range(1, K + 1) if int(tab[l - 1][0]) > 0 and int(ids[l - 1]) > 0]
    for l in live:
        t = int(ids[l - 1])
        X0, _ = otr.cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
        Y0, _ = otr.cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
        digits = str(t)
        if not (X0 <= x < X0 + s * (6 * len(digits) + 1) and Y0 <= y < Y0 + 9 * s):
            continue
        for j, ch in enumerate(digits):
            ox, oy = X0 + s * (1 + 6 * j), Y0 + s
            gx, gy = (x - ox) // s, (y - oy) // s
            if 0 <= gx < 5 and 0 <= gy < 7 and (int(font[int(ch)][gy]) >> (4 - gx)) & 1:
                return (0, 0, 0)
        return otr.colour(t, None)
    for l in live:
        if int(age[l - 1]) > 0 and not on_stripe(y, x, s):
            continue
        X0, X1 = otr.cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
        Y0, Y1 = otr.cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
        if X0 <= x <= X1 and Y0 <= y <= Y1 and min(x - X0, X1 - x, y - Y0, Y1 - y) < B:
            return otr.colour(int(ids[l - 1]), None)
    return None


def decorations(tab, ids, age, K, H, W, B, font):
    """(covered bool [H,W], rgb int64 [H,W,3]) of decoration_of_pixel over the frame; the pixels visited are those that a plate or a
    border of any object can reach (overlay_tracks_ref.decorations' set: hatching only takes pixels away)."""
    covered, rgb = np.zeros((H, W), dtype=bool), np.zeros((H, W, 3), dtype=np.int64)
    if B <= 0:
        return covered, rgb
    s = otr.scale(H, W)
    reach = np.zeros((H, W), dtype=bool)
    for l in range(1, K + 1):
        if int(tab[l - 1][0]) > 0 and int(ids[l - 1]) > 0:
            X0, X1 = otr.cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
            Y0, Y1 = otr.cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
            ring = np.ones((Y1 - Y0 + 1, X1 - X0 + 1), dtype=bool)
            ring[4:-4, 4:-4] = False
            reach[Y0:Y1 + 1, X0:X1 + 1] |= ring
            reach[Y0:Y0 + 9 * s, X0:X0 + s * (6 * len(str(int(ids[l - 1]))) + 1)] = True
    for y, x in zip(*np.nonzero(reach)):
        c = decoration_of_pixel(tab, ids, age, K, int(y), int(x), H, W, B, font)
        if c is not None:
            covered[y, x], rgb[y, x] = True, c
    return covered, rgb


def panel_ref(guide, grey, hard, labels, ids, table, age, font, color, alpha256, t, boxes):
    """The overlay panel uint8 [n,H,W,3]."""
    guide, grey, age = np.asarray(guide), np.asarray(grey), np.asarray(age)
    n, H, W = grey.shape
    K = np.asarray(ids).shape[1]
    assert guide.dtype == np.uint8 and grey.dtype == np.uint8 and guide.shape == (n, H, W, 3) and 0 <= alpha256 <= 256
    assert np.asarray(labels).shape == (n, otr.SIDE, otr.SIDE) and np.asarray(table).shape == (n, K, 8) and age.shape == (n, K)
    s = otr.scale(H, W)
    stripe = np.array([[on_stripe(y, x, s) for x in range(W)] for y in range(H)], dtype=bool)
    edge = overlay_ref.outline_ref(hard, t)
    out = np.zeros((n, H, W, 3), dtype=np.uint8)
    for f in range(n):
        objs = otr.object_map(labels[f], K, H, W)
        colours = np.array([otr.colour(0, color)] + [otr.colour(int(ids[f][l - 1]), color) for l in range(1, K + 1)], dtype=np.int64)
        carried = np.array([False] + [int(age[f][l - 1]) > 0 for l in range(1, K + 1)], dtype=bool)
        tint = colours[objs]
        q = alpha256 * grey[f].astype(np.int64)
        q = np.where(carried[objs] & ~stripe, 0, q)[..., None]
        over = (guide[f].astype(np.int64) * (65280 - q) + tint * q + 32640) // 65280
        if edge is not None:
            over = np.where(edge[f][..., None], tint, over)
        covered, rgb = decorations(table[f], ids[f], age[f], K, H, W, boxes, font)
        over = np.where(covered[..., None], rgb, over)
        assert over.min() >= 0 and over.max() <= 255
        out[f] = over
    return out


def compose_carried_ref(guide, grey, hard, labels, ids, table, age, font, color, alpha256, t, boxes, layout):
    """uint8 [n,H,k W,3] as cgs_overlay_compose_tracks_carried writes it."""
    return otr.lay_out(np.asarray(guide), grey, panel_ref(guide, grey, hard, labels, ids, table, age, font, color, alpha256, t, boxes),
                       layout)
