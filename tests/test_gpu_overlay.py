"""The frames of the overlay video on the GPU (cgs_overlay_compose, cgs_amd.overlay) against tests/overlay_ref.py, bit for bit: every
size class of the bit rows (one word, a ragged last word, several words), every load width, every outline thickness on masks chosen for
the outline's edge cases, no mask, the ends of the tint's range, the three layouts, the non-temporal stores and the entry's checks."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import overlay_ref  # noqa: E402
from cgs_amd import _lib, overlay  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = ((64, 64), (65, 67), (66, 130), (70, 128), (96, 200))
LAYOUTS = ("overlay", "side", "triple")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blobs(n, h, w, rs):
    """8 x 8 blocks on or off, a few of them shifted, and a sprinkle of single pixels switched: outlines of every local shape."""
    m = np.repeat(np.repeat(rs.rand(n, h // 8 + 2, w // 8 + 2) > 0.5, 8, axis=1), 8, axis=2)[:, 3:3 + h, 5:5 + w]
    return (m ^ (rs.rand(n, h, w) < 0.01)).astype(np.uint8)


def _inputs(n, h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8), rs.randint(0, 256, (n, h, w)).astype(np.uint8), _blobs(n, h, w, rs)


def _check(guide, grey, hard, color=(0, 255, 0), alpha256=128, t=1, layout="overlay", **kw):
    got = overlay.compose(_dev(guide), _dev(grey), _dev(hard), color=color, alpha256=alpha256, outline=t, layout=layout, **kw).cpu().numpy()
    want = overlay_ref.compose_ref(guide, grey, hard, color, alpha256, t, layout)
    assert got.shape == want.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want, err_msg=f"{guide.shape} alpha256 {alpha256} t {t} {layout}")
    return got


@pytest.mark.parametrize("h, w", SIZES)
def test_sizes(h, w):
    guide, grey, hard = _inputs(2, h, w, 100 * h + w)
    for t, layout in ((1, "overlay"), (2, "triple"), (4, "side")):
        _check(guide, grey, hard, color=(250, 40, 7), alpha256=77, t=t, layout=layout)


def test_every_load_width():
    """Rows are moved 16, 4 or 1 bytes at a time, by the alignment of guide, grey, out and W: the same frames through all three (a view
    that starts 4 or 1 bytes into an allocation moves a base; W = 128 allows 16, W = 68 only 4, W = 67 only 1)."""
    for h, w in ((70, 128), (64, 68), (66, 67)):
        guide, grey, hard = _inputs(2, h, w, h + w)
        for layout in LAYOUTS:
            k = overlay.panels(layout)
            want = overlay_ref.compose_ref(guide, grey, hard, (9, 200, 255), 200, 2, layout)
            for shift in (0, 4, 1):
                def view(a):
                    flat = torch.empty(a.size + 16, dtype=torch.uint8, device=DEV)
                    v = flat[shift:shift + a.size].view(a.shape)
                    v.copy_(_dev(a))
                    assert v.data_ptr() % 16 == shift and v.is_contiguous()
                    return v
                out = view(np.zeros((2, h, k * w, 3), dtype=np.uint8))
                got = overlay.compose(view(guide), view(grey), view(hard), color=(9, 200, 255), alpha256=200, outline=2, layout=layout, out=out)
                assert got.data_ptr() == out.data_ptr()
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{h}x{w} {layout} shift {shift}")


def _masks(h, w):
    rs = np.random.RandomState(h * w)
    yy, xx = np.mgrid[:h, :w]
    disc = lambda cy, cx, r: ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
    single = np.zeros((h, w), dtype=np.uint8)
    single[h // 2, 70] = 1
    cut = disc(0, w // 3, 9) | disc(h - 1, 2 * w // 3, 11) | disc(h // 2, 0, 8) | disc(h // 3, w - 1, 10) | disc(0, 0, 6) | disc(h - 1, w - 1, 7)
    straddle = np.zeros((h, w), dtype=np.uint8)
    straddle[10:30, 58:70] = 1                         # columns 63 / 64
    straddle[35:60, 120:136] = 1                       # columns 127 / 128
    straddle[5:8, 63:65] = 1
    straddle[62:66, 127:129] = 1
    return {"blobs": _blobs(1, h, w, rs)[0], "on": np.ones((h, w), dtype=np.uint8), "off": np.zeros((h, w), dtype=np.uint8),
            "single": single, "checkerboard": ((yy + xx) & 1).astype(np.uint8), "cut": cut, "straddle": straddle}


@pytest.mark.parametrize("kind", ["blobs", "on", "off", "single", "checkerboard", "cut", "straddle"])
def test_thickness_on_chosen_masks(kind):
    h, w = 70, 200
    guide, grey, _ = _inputs(2, h, w, 3)
    m = _masks(h, w)[kind]
    hard = np.stack((m, np.ascontiguousarray(m[::-1, ::-1])))
    plain = overlay_ref.compose_ref(guide, grey, None, (255, 0, 255), 128, 0, "overlay")
    for t in range(5):
        got = _check(guide, grey, hard, color=(255, 0, 255), alpha256=128, t=t)
        edge = (got != plain).any(axis=-1)             # (a pixel whose tint already is the colour hides; the reference has the say)
        if kind in ("on", "off") or t == 0:
            np.testing.assert_array_equal(got, plain)  # a full mask has no outline anywhere: the frame's edge counts as on
        if kind == "cut" and t:
            ring = np.zeros((h, w), dtype=bool)
            ring[[0, -1], :] = ring[:, [0, -1]] = True
            inner = overlay_ref.erode_ref(hard, t)
            assert (ring[None] & inner).any() and not (edge & inner).any()       # no line along the frame's edge inside a blob
        if kind == "checkerboard" and t:
            assert (overlay_ref.outline_ref(hard, t) == (hard != 0)).all()        # every on pixel is outline
        if kind == "single" and t:
            assert overlay_ref.outline_ref(hard, t).sum() == 2


def test_without_a_mask():
    guide, grey, hard = _inputs(2, 65, 67, 21)
    a = _check(guide, grey, None, t=3)
    b = _check(guide, grey, hard, t=0)
    np.testing.assert_array_equal(a, b)
    # bool masks are taken as they are, and any non-zero byte is on
    want = _check(guide, grey, hard, t=2)
    for other in (torch.from_numpy(hard.astype(bool)).to(DEV), _dev(hard * np.uint8(200))):
        got = overlay.compose(_dev(guide), _dev(grey), other, outline=2)
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("alpha256", [0, 1, 128, 256])
def test_ends_of_the_tint(alpha256):
    h, w = 64, 80
    rs = np.random.RandomState(alpha256)
    guide = rs.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), (2, h, w, 3))
    grey = rs.choice(np.array([0, 1, 2, 127, 128, 253, 254, 255], dtype=np.uint8), (2, h, w))
    for color in ((0, 255, 0), (255, 255, 255), (0, 0, 0), (1, 254, 128)):
        got = _check(guide, grey, None, color=color, alpha256=alpha256, t=0)
        if alpha256 == 0:
            np.testing.assert_array_equal(got, guide)                    # nothing of the tint: the frame itself
        if alpha256 == 256:
            np.testing.assert_array_equal(got[grey == 255], np.broadcast_to(np.array(color, dtype=np.uint8), got[grey == 255].shape))
            np.testing.assert_array_equal(got[grey == 0], guide[grey == 0])


def test_layouts():
    h, w = 66, 130
    guide, grey, hard = _inputs(2, h, w, 8)
    one = _check(guide, grey, hard, t=2, layout="overlay")
    two = _check(guide, grey, hard, t=2, layout="side")
    three = _check(guide, grey, hard, t=2, layout="triple")
    assert two.shape == (2, h, 2 * w, 3) and three.shape == (2, h, 3 * w, 3)
    for frame_first in (two, three):
        np.testing.assert_array_equal(frame_first[:, :, :w], guide)
        np.testing.assert_array_equal(frame_first[:, :, w:2 * w], one)
    np.testing.assert_array_equal(three[:, :, 2 * w:], np.repeat(grey[..., None], 3, axis=3))


def test_nontemporal_stores_give_the_same_bytes():
    for h, w in ((70, 128), (65, 67)):
        guide, grey, hard = _inputs(2, h, w, 4)
        for layout in LAYOUTS:
            a = _check(guide, grey, hard, t=1, layout=layout, nontemporal=True)
            b = _check(guide, grey, hard, t=1, layout=layout, nontemporal=False)
            np.testing.assert_array_equal(a, b)


def test_entry_argument_checks():
    """The C entry refuses bad arguments before anything is launched."""
    lib = _lib.load()
    fr = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=DEV)
    gr = torch.zeros((1, 64, 64), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 64, 64, 3), 9, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(guide=fr.data_ptr(), grey=gr.data_ptr(), hard=None, n=1, h=64, w=64, r=0, g=255, b=0, a=128, t=1, layout=1, flags=0,
             out_=out.data_ptr()):
        return lib.cgs_overlay_compose(guide, grey, hard, n, h, w, r, g, b, a, t, layout, flags, out_, st)
    bad = _lib.ERR_BADARG
    assert call(guide=None) == bad and call(grey=None) == bad and call(out_=None) == bad
    assert call(n=0) == bad and call(n=65536) == bad and call(h=0) == bad and call(w=-1) == bad
    assert call(r=256) == bad and call(g=-1) == bad and call(b=1000) == bad and call(a=-1) == bad and call(a=257) == bad
    assert call(t=-1) == bad and call(t=5) == bad and call(layout=0) == bad and call(layout=4) == bad and call(flags=2) == bad
    assert call(h=63) == _lib.ERR_UNSUPPORTED and call(w=4097) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                        # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # the module's own checks
    for kw in (dict(color=(0, 256, 0)), dict(alpha256=257), dict(alpha256=0.5), dict(outline=5), dict(layout="quad")):
        with pytest.raises(ValueError):
            overlay.compose(fr, gr, **kw)
    with pytest.raises(ValueError):
        overlay.compose(fr, gr[:, :32])
    with pytest.raises(ValueError):
        overlay.compose(fr, gr, hard=gr.float())
