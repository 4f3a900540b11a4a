"""The direct form of what cgs_overlay_compose computes (include/cgs_hip.h), the checker of tests/test_overlay_host.py and
tests/test_gpu_overlay.py.  Integers throughout; written from the pixel rule, not from the kernel: the erosion is t passes over whole
boolean planes padded with True (a neighbour outside the frame counts as on) -- no bit rows, no bands, no halo."""
import numpy as np


def erode_ref(hard, t):
    """bool [n,H,W] -> E_t: t times, a pixel stays on when it and its four neighbours are on, outside the frame counting as on."""
    e = np.asarray(hard) != 0
    for _ in range(t):
        p = np.pad(e, ((0, 0), (1, 1), (1, 1)), constant_values=True)
        e = p[:, 1:-1, 1:-1] & p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:]
    return e


def outline_ref(hard, t):
    """bool [n,H,W]: hard & ~E_t; nothing at t = 0 or without a mask."""
    if hard is None or t == 0:
        return None
    on = np.asarray(hard) != 0
    return on & ~erode_ref(on, t)


def compose_ref(guide, grey, hard, color, alpha256, t, layout):
    """guide uint8 [n,H,W,3], grey uint8 [n,H,W], hard [n,H,W] or None, color (r, g, b), alpha256 0..256, t 0..4, layout "overlay" /
    "side" / "triple" -> uint8 [n,H,k W,3]."""
    guide, grey = np.asarray(guide), np.asarray(grey)
    assert guide.dtype == np.uint8 and grey.dtype == np.uint8 and guide.shape[:3] == grey.shape and 0 <= alpha256 <= 256 and 0 <= t <= 4
    q = (alpha256 * grey.astype(np.int64))[..., None]                              # <= 65280
    tint = np.array(color, dtype=np.int64)
    over = (guide.astype(np.int64) * (65280 - q) + tint * q + 32640) // 65280
    edge = outline_ref(hard, t)
    if edge is not None:
        over = np.where(edge[..., None], tint, over)
    assert over.min() >= 0 and over.max() <= 255
    over = over.astype(np.uint8)
    if layout == "overlay":
        return over
    if layout == "side":
        return np.concatenate((guide, over), axis=2)
    assert layout == "triple"
    return np.concatenate((guide, over, np.repeat(grey[..., None], 3, axis=3)), axis=2)
