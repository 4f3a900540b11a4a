"""The direct form of what cgs_overlay_compose_tracks computes (include/cgs_hip.h), the checker of tests/test_overlay_tracks_host.py,
tests/test_gpu_overlay_tracks.py and tests/test_gpu_process_video_tracks.py.  Written from the pixel rules with Python integers and
loops over pixels: no bands, no staged cells, no box lists.  The tint and the outline are tests/overlay_ref.py's, with a colour per pixel."""
import numpy as np

import overlay_ref

SIDE, RADIUS = 64, 2


def colour(t, default):
    """(r, g, b) of track t; `default` for t <= 0."""
    if t <= 0:
        return tuple(int(v) for v in default)
    hsh = (int(t) * 2654435761) % (1 << 32)
    return tuple(64 + ((hsh >> (8 * c)) & 255) * 191 // 255 for c in range(3))


def home(p, L):
    return ((2 * p + 1) * 32) // L


def cell_pixels(c0, c1, L):
    """(first, last) pixel of the cells c0..c1 of an axis of length L."""
    return (c0 * L + 31) // 64, ((c1 + 1) * L + 31) // 64 - 1


def scale(H, W):
    return max(1, min(H, W) // 256)


def object_of_pixel(lab, K, y, x, H, W):
    """The label in 1..K of pixel (y, x) of an H x W frame over the label map lab [64,64]; 0 when it has no object."""
    cy, cx = home(y, H), home(x, W)
    l = int(lab[cy, cx])
    if 1 <= l <= K:
        return l
    if l > K:
        return 0
    best, pick = None, 0
    for c2y in range(cy - RADIUS, cy + RADIUS + 1):                        # raster order; a later cell wins only when strictly nearer
        for c2x in range(cx - RADIUS, cx + RADIUS + 1):
            if not (0 <= c2y < SIDE and 0 <= c2x < SIDE) or not 1 <= int(lab[c2y, c2x]) <= K:
                continue
            dxn = (2 * x + 1) * 64 - (2 * c2x + 1) * W
            dyn = (2 * y + 1) * 64 - (2 * c2y + 1) * H
            cost = dxn * dxn * H * H + dyn * dyn * W * W
            if best is None or cost < best:
                best, pick = cost, int(lab[c2y, c2x])
    return pick


def object_map(lab, K, H, W):
    """int64 [H,W]: object_of_pixel for every pixel."""
    lab = np.asarray(lab)
    out = np.zeros((H, W), dtype=np.int64)
    inside = (lab >= 1) & (lab <= K)
    for y in range(H):
        cy = home(y, H)
        for x in range(W):
            cx = home(x, W)
            if inside[cy, cx]:
                out[y, x] = lab[cy, cx]
            elif inside[max(cy - RADIUS, 0):cy + RADIUS + 1, max(cx - RADIUS, 0):cx + RADIUS + 1].any():   # (else the search finds nothing)
                out[y, x] = object_of_pixel(lab, K, y, x, H, W)
    return out


def decoration_of_pixel(tab, ids, K, y, x, H, W, B, font):
    """The colour (r, g, b) that a plate or a border puts on pixel (y, x), or None: plates first, then borders, the smallest label first."""
    if B <= 0:
        return None
    s = scale(H, W)
    live = [l for l in range(1, K + 1) if int(tab[l - 1][0]) > 0 and int(ids[l - 1]) > 0]
    for l in live:
        t = int(ids[l - 1])
        X0, _ = cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
        Y0, _ = cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
        digits = str(t)
        if not (X0 <= x < X0 + s * (6 * len(digits) + 1) and Y0 <= y < Y0 + 9 * s):
            continue
        for j, ch in enumerate(digits):
            ox, oy = X0 + s * (1 + 6 * j), Y0 + s
            gx, gy = (x - ox) // s, (y - oy) // s                         # (floor division: negative left of / above the glyph)
            if 0 <= gx < 5 and 0 <= gy < 7 and (int(font[int(ch)][gy]) >> (4 - gx)) & 1:
                return (0, 0, 0)
        return colour(t, None)
    for l in live:
        X0, X1 = cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
        Y0, Y1 = cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
        if X0 <= x <= X1 and Y0 <= y <= Y1 and min(x - X0, X1 - x, y - Y0, Y1 - y) < B:
            return colour(int(ids[l - 1]), None)
    return None


def decorations(tab, ids, K, H, W, B, font):
    """(covered bool [H,W], rgb int64 [H,W,3]) of decoration_of_pixel over the frame; only the pixels that some plate or border can reach
    are visited: the plates, and of every rectangle the pixels fewer than 4 (the thickest border) from a side."""
    covered, rgb = np.zeros((H, W), dtype=bool), np.zeros((H, W, 3), dtype=np.int64)
    if B <= 0:
        return covered, rgb
    s = scale(H, W)
    reach = np.zeros((H, W), dtype=bool)
    for l in range(1, K + 1):
        if int(tab[l - 1][0]) > 0 and int(ids[l - 1]) > 0:
            X0, X1 = cell_pixels(int(tab[l - 1][1]), int(tab[l - 1][3]), W)
            Y0, Y1 = cell_pixels(int(tab[l - 1][2]), int(tab[l - 1][4]), H)
            ring = np.ones((Y1 - Y0 + 1, X1 - X0 + 1), dtype=bool)
            ring[4:-4, 4:-4] = False
            reach[Y0:Y1 + 1, X0:X1 + 1] |= ring
            reach[Y0:Y0 + 9 * s, X0:X0 + s * (6 * len(str(int(ids[l - 1]))) + 1)] = True      # (slices clip at the frame)
    for y, x in zip(*np.nonzero(reach)):
        c = decoration_of_pixel(tab, ids, K, int(y), int(x), H, W, B, font)
        if c is not None:
            covered[y, x], rgb[y, x] = True, c
    return covered, rgb


def pixel_colours(lab, ids, K, H, W, default):
    """int64 [H,W,3]: the colour of every pixel's object's track, `default` where there is none."""
    table = np.array([colour(0, default)] + [colour(int(ids[l - 1]), default) for l in range(1, K + 1)], dtype=np.int64)
    return table[object_map(lab, K, H, W)]


def panel_ref(guide, grey, hard, labels, ids, table, font, color, alpha256, t, boxes):
    """The overlay panel uint8 [n,H,W,3]."""
    guide, grey = np.asarray(guide), np.asarray(grey)
    n, H, W = grey.shape
    K = np.asarray(ids).shape[1]
    assert guide.dtype == np.uint8 and grey.dtype == np.uint8 and guide.shape == (n, H, W, 3) and 0 <= alpha256 <= 256
    assert np.asarray(labels).shape == (n, SIDE, SIDE) and np.asarray(table).shape == (n, K, 8) and 1 <= K <= 64
    edge = overlay_ref.outline_ref(hard, t)
    out = np.zeros((n, H, W, 3), dtype=np.uint8)
    for f in range(n):
        tint = pixel_colours(labels[f], ids[f], K, H, W, color)
        q = (alpha256 * grey[f].astype(np.int64))[..., None]
        over = (guide[f].astype(np.int64) * (65280 - q) + tint * q + 32640) // 65280
        if edge is not None:
            over = np.where(edge[f][..., None], tint, over)
        covered, rgb = decorations(table[f], ids[f], K, H, W, boxes, font)
        over = np.where(covered[..., None], rgb, over)
        assert over.min() >= 0 and over.max() <= 255
        out[f] = over
    return out


def lay_out(guide, grey, panel, layout):
    if layout == "overlay":
        return panel
    if layout == "side":
        return np.concatenate((guide, panel), axis=2)
    assert layout == "triple"
    return np.concatenate((guide, panel, np.repeat(np.asarray(grey)[..., None], 3, axis=3)), axis=2)


def compose_tracks_ref(guide, grey, hard, labels, ids, table, font, color, alpha256, t, boxes, layout):
    """uint8 [n,H,k W,3] as cgs_overlay_compose_tracks writes it."""
    return lay_out(np.asarray(guide), grey, panel_ref(guide, grey, hard, labels, ids, table, font, color, alpha256, t, boxes), layout)


def table_of(labels, K):
    """int32 [n,K,8] as cgs_objects_label fills it for hand-made label maps: area, x0, y0, x1, y1, sum_x, sum_y, first."""
    labels = np.asarray(labels)
    out = np.zeros((labels.shape[0], K, 8), dtype=np.int32)
    for f, lab in enumerate(labels):
        for l in range(1, K + 1):
            ys, xs = np.nonzero(lab == l)
            if len(ys):
                out[f, l - 1] = [len(ys), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum(), (ys * lab.shape[1] + xs).min()]
    return out


def scene(K=6):
    """Hand-made (labels int32 [3,64,64], ids int32 [3,K], table int32 [3,K,8]) for K = 6 with every case of the drawing rules:
    frame 0  no object;
    frame 1  object 1 a cross that touches all four frame edges (track 8388607, 7 digits); object 2 a block inside the cross's box, so
             the two boxes overlap (track 5, 1 digit); object 3 the one cell of the bottom right corner, its plate clipped by the frame
             (track 12); a row with a track but no area (label 4: no object); a block labelled 7 > K;
    frame 2  object 1 a block (track 3); object 2 an L and object 4 a block inside the L's box (tracks 1000000 and 42); object 3 a block
             without a track; objects 5 and 6 single cells two apart in a row (tracks 77 and 78): the cell between them is a tie."""
    assert K == 6
    labels = np.zeros((3, SIDE, SIDE), dtype=np.int32)
    a = labels[1]
    a[30:34, :] = 1
    a[:, 30:34] = 1
    a[5:13, 5:13] = 2
    a[63, 63] = 3
    a[40:46, 40:46] = 7
    b = labels[2]
    b[2:21, 3:31] = 1
    b[22:41, 10:13] = 2
    b[38:41, 10:41] = 2
    b[24:31, 20:31] = 4
    b[5:12, 45:60] = 3
    b[50, 50], b[50, 52] = 5, 6
    ids = np.array([[0] * 6, [8388607, 5, 12, 9, 0, 0], [3, 1000000, 0, 42, 77, 78]], dtype=np.int32)
    return labels, ids, table_of(labels, K)
