"""The frames of the overlay video with tracked objects on the GPU (cgs_overlay_compose_tracks, cgs_amd.overlay.compose_tracks) against
tests/overlay_tracks_ref.py, bit for bit, on the hand-made scene of that file: every load width, every layout, boxes 0 / 1 / 4, outline
0 / 2, no mask, a frame big enough for digits of two pixels a font pixel, the link to cgs_overlay_compose (no labels: its bytes) and the
entry's checks.  The reference of a size is computed once and shared."""
import functools
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
import overlay_tracks_ref as ref  # noqa: E402
from cgs_amd import _lib, overlay  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 6
COLOR, ALPHA = (250, 40, 7), 150
LAYOUTS = ("overlay", "side", "triple")
LABELS, IDS, TABLE = ref.scene(K)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(h, w, frames=(0, 1, 2)):
    """(guide, grey, hard) of the scene's frames at h x w: random frames, a grey byte that is non-zero almost everywhere and independent
    of the labels (so unlabelled cells next to and far from objects, and the block labelled above K, are tinted), a blocky mask."""
    rs = np.random.RandomState(1000 * h + w)
    n = len(frames)
    guide = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    grey = rs.randint(0, 256, (n, h, w)).astype(np.uint8)
    hard = np.repeat(np.repeat(rs.rand(n, h // 8 + 2, w // 8 + 2) > 0.5, 8, axis=1), 8, axis=2)[:, 3:3 + h, 5:5 + w]
    hard = (hard ^ (rs.rand(n, h, w) < 0.01)).astype(np.uint8)
    for a in (guide, grey, hard):
        a.setflags(write=False)
    return guide, grey, hard


@functools.lru_cache(maxsize=None)
def _tints(h, w, frames=(0, 1, 2)):
    """Per frame the colour of every pixel's object (the slow part of the reference), once per size."""
    return tuple(ref.pixel_colours(LABELS[f], IDS[f], K, h, w, COLOR) for f in frames)


@functools.lru_cache(maxsize=None)
def _decor(h, w, boxes, frames=(0, 1, 2)):
    return tuple(ref.decorations(TABLE[f], IDS[f], K, h, w, boxes, overlay.FONT) for f in frames)


@functools.lru_cache(maxsize=None)
def _panel(h, w, boxes, t, with_hard, frames=(0, 1, 2)):
    """ref.panel_ref from the shared pieces (the same arithmetic, line for line)."""
    guide, grey, hard = _inputs(h, w, frames)
    edge = overlay_ref.outline_ref(hard if with_hard else None, t)
    out = np.zeros(guide.shape, dtype=np.uint8)
    for i in range(len(frames)):
        tint = _tints(h, w, frames)[i]
        q = (ALPHA * grey[i].astype(np.int64))[..., None]
        over = (guide[i].astype(np.int64) * (65280 - q) + tint * q + 32640) // 65280
        if edge is not None:
            over = np.where(edge[i][..., None], tint, over)
        covered, rgb = _decor(h, w, boxes, frames)[i]
        out[i] = np.where(covered[..., None], rgb, over)
    return out


def _gpu(h, w, boxes, t, with_hard, layout, frames=(0, 1, 2), **kw):
    guide, grey, hard = _inputs(h, w, frames)
    pick = list(frames)
    return overlay.compose_tracks(_dev(guide), _dev(grey), _dev(hard) if with_hard else None, _dev(LABELS[pick]), _dev(IDS[pick]),
                                  _dev(TABLE[pick]), color=COLOR, alpha256=ALPHA, outline=t, boxes=boxes, layout=layout, **kw).cpu().numpy()


def _check(h, w, boxes, t, with_hard, layout, frames=(0, 1, 2)):
    guide, grey, _ = _inputs(h, w, frames)
    got = _gpu(h, w, boxes, t, with_hard, layout, frames)
    want = ref.lay_out(guide, grey, _panel(h, w, boxes, t, with_hard, frames), layout)
    assert got.shape == want.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w} boxes {boxes} outline {t} hard {with_hard} {layout}")
    return got


def test_the_shared_pieces_are_the_reference():
    """_panel puts ref.panel_ref together from cached pieces: on the smallest size both are computed and compared."""
    guide, grey, hard = _inputs(64, 64)
    want = ref.panel_ref(guide, grey, hard, LABELS, IDS, TABLE, overlay.FONT, COLOR, ALPHA, 2, 1)
    np.testing.assert_array_equal(_panel(64, 64, 1, 2, True), want)


def test_the_scene_holds_every_case():
    """Conditions on the inputs, so that the comparisons below cannot pass without meeting the cases they are for."""
    h, w = 72, 100
    _, grey, _ = _inputs(h, w)
    hy, hx = ref.home(np.arange(h), h), ref.home(np.arange(w), w)
    assert not LABELS[0].any() and (grey[0] > 0).any()                                      # a frame with no object
    assert tuple(TABLE[1, 0, 1:5]) == (0, 0, 63, 63)                                        # an object touching all four edges
    assert tuple(TABLE[1, 2, 1:5]) == (63, 63, 63, 63) and IDS[1, 2] >= 10                  # bottom right corner: the plate is clipped
    x0, y0, x1, y1 = TABLE[1, 1, 1:5]
    assert TABLE[1, 0, 1] <= x0 and x1 <= TABLE[1, 0, 3] and TABLE[1, 0, 2] <= y0 and y1 <= TABLE[1, 0, 4]     # two overlapping boxes
    a, b = TABLE[2, 1, 1:5], TABLE[2, 3, 1:5]
    assert a[0] <= b[0] and b[2] <= a[2] and a[1] <= b[1] and b[3] <= a[3]
    above = LABELS[1][hy][:, hx] > K
    assert (above & (grey[1] > 0)).any()                                                    # a label above K with grey > 0
    assert len(str(IDS.max())) == 7 and 1 <= IDS[1, 1] <= 9                                 # 7 digits and 1 digit
    assert TABLE[1, 3, 0] == 0 and IDS[1, 3] > 0 and TABLE[2, 2, 0] > 0 and IDS[2, 2] == 0  # a track without an area, an area without a track
    # unlabelled home cells 1, 2 and 3 cells from an object, grey > 0: found by the search, or left to the default colour
    lab = LABELS[1]
    on = (lab >= 1) & (lab <= K)
    near = {r: np.zeros_like(on) for r in (1, 2, 3)}
    for cy, cx in zip(*np.nonzero(lab == 0)):
        d = min(r for r in (1, 2, 3, 99) if r == 99 or on[max(cy - r, 0):cy + r + 1, max(cx - r, 0):cx + r + 1].any())
        if d in near:
            near[d][cy, cx] = True
    found = ref.object_map(lab, K, h, w)
    for r in (1, 2, 3):
        px = near[r][hy][:, hx] & (grey[1] > 0)
        assert px.any() and ((found[px] > 0).all() if r <= 2 else (found[px] == 0).all()), r


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h, w", [(64, 64), (72, 100), (66, 70)])
def test_sizes_and_parameters(h, w, layout):
    """64 x 64: identity cells, 16 pixels a thread; 72 x 100: 4; 66 x 70: 1, and rows below 64 in a last band of 2."""
    for boxes in (0, 1, 4):
        for t in (0, 2):
            _check(h, w, boxes, t, True, layout)
    _check(h, w, 1, 2, False, layout)                                     # hard=None: no outline


def test_misaligned_views_take_the_narrow_paths():
    """128 x 192 allows 16 pixels a thread; a view that starts 4 or 1 bytes into an allocation forces 4 and 1 on the same frames."""
    h, w = 128, 192
    guide, grey, hard = _inputs(h, w)
    for layout in LAYOUTS:
        k = overlay.panels(layout)
        want = ref.lay_out(guide, grey, _panel(h, w, 1, 2, True), layout)
        for shift in (0, 4, 1):
            def view(a):
                flat = torch.empty(a.size + 16, dtype=torch.uint8, device=DEV)
                v = flat[shift:shift + a.size].view(a.shape)
                v.copy_(_dev(a))
                assert v.data_ptr() % 16 == shift and v.is_contiguous()
                return v
            out = view(np.zeros((3, h, k * w, 3), dtype=np.uint8))
            got = overlay.compose_tracks(view(guide), view(grey), view(hard), _dev(LABELS), _dev(IDS), _dev(TABLE), color=COLOR,
                                         alpha256=ALPHA, outline=2, boxes=1, layout=layout, out=out)
            assert got.data_ptr() == out.data_ptr()
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{layout} shift {shift}")


def test_scale_two():
    """One frame of 600 x 520: s = 2, every font pixel is 2 x 2."""
    assert ref.scale(600, 520) == 2 == overlay.scale(600, 520)
    _check(600, 520, 1, 2, True, "triple", frames=(1,))
    _check(600, 520, 4, 0, True, "overlay", frames=(1,))
    _check(600, 520, 0, 2, False, "side", frames=(1,))


def test_without_labels_it_is_compose():
    """No labelled cell: every pixel has the default colour and nothing is drawn -- cgs_overlay_compose's bytes."""
    for h, w in ((64, 64), (66, 70), (72, 100)):
        guide, grey, hard = _inputs(h, w)
        for layout, t in (("overlay", 1), ("triple", 3)):
            want = overlay.compose(_dev(guide), _dev(grey), _dev(hard), color=COLOR, alpha256=ALPHA, outline=t, layout=layout).cpu().numpy()
            np.testing.assert_array_equal(want, overlay_ref.compose_ref(guide, grey, hard, COLOR, ALPHA, t, layout))
            got = overlay.compose_tracks(_dev(guide), _dev(grey), _dev(hard), _dev(np.zeros_like(LABELS)), _dev(IDS), _dev(TABLE * 0),
                                         color=COLOR, alpha256=ALPHA, outline=t, boxes=4, layout=layout).cpu().numpy()
            np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w} {layout}")


def test_nontemporal_stores_and_a_device_font_give_the_same_bytes():
    a = _gpu(72, 100, 1, 2, True, "side", nontemporal=True)
    b = _gpu(72, 100, 1, 2, True, "side", nontemporal=False)
    c = _gpu(72, 100, 1, 2, True, "side", font=_dev(overlay.FONT))
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    other = np.array(overlay.FONT)
    other[5] = other[8]                                                   # the font is read from the pointer: another font, other bytes
    d = _gpu(72, 100, 1, 2, True, "side", font=other)
    assert (a != d).any()


def test_entry_argument_checks():
    """The C entry refuses bad arguments before anything is launched; the module's own checks raise ValueError."""
    lib = _lib.load()
    fr = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=DEV)
    gr = torch.zeros((1, 64, 64), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((1, 64, 64), dtype=torch.int32, device=DEV)
    ids = torch.zeros((1, K), dtype=torch.int32, device=DEV)
    tab = torch.zeros((1, K, 8), dtype=torch.int32, device=DEV)
    font = _dev(overlay.FONT)
    out = torch.full((1, 64, 64, 3), 9, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(guide=fr.data_ptr(), grey=gr.data_ptr(), hard=None, labels=lab.data_ptr(), ids_=ids.data_ptr(), table=tab.data_ptr(),
             font_=font.data_ptr(), n=1, h=64, w=64, k=K, r=0, g=255, b=0, a=128, t=1, boxes=1, layout=1, flags=0, out_=out.data_ptr()):
        return lib.cgs_overlay_compose_tracks(guide, grey, hard, labels, ids_, table, font_, n, h, w, k, r, g, b, a, t, boxes, layout, flags,
                                              out_, st)
    bad = _lib.ERR_BADARG
    assert call(guide=None) == bad and call(grey=None) == bad and call(out_=None) == bad and call(labels=None) == bad
    assert call(ids_=None) == bad and call(table=None) == bad and call(font_=None) == bad and call(labels=lab.data_ptr() + 2) == bad
    assert call(n=0) == bad and call(n=65536) == bad and call(h=0) == bad and call(w=-1) == bad and call(k=0) == bad
    assert call(r=256) == bad and call(g=-1) == bad and call(b=1000) == bad and call(a=-1) == bad and call(a=257) == bad
    assert call(t=-1) == bad and call(t=5) == bad and call(layout=0) == bad and call(layout=4) == bad and call(flags=2) == bad
    assert call(boxes=-1) == bad and call(boxes=5) == bad
    assert call(h=63) == _lib.ERR_UNSUPPORTED and call(w=4097) == _lib.ERR_UNSUPPORTED and call(k=65) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                        # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    ok = dict(guide=fr, grey=gr, hard=None, labels=lab, ids=ids, table=tab)
    for kw in (dict(color=(0, 256, 0)), dict(alpha256=257), dict(outline=5), dict(boxes=5), dict(boxes=True), dict(layout="quad"),
               dict(labels=lab.long()), dict(labels=lab[:, :32]), dict(ids=ids.float()), dict(ids=torch.zeros((1, 65), dtype=torch.int32, device=DEV)),
               dict(table=tab[:, :, :7]), dict(table=tab[:, :3]), dict(grey=gr[:, :32]), dict(hard=gr.float()),
               dict(font=np.zeros((10, 8), dtype=np.uint8)), dict(font=overlay.FONT.astype(np.int32))):
        with pytest.raises(ValueError):
            overlay.compose_tracks(**{**ok, **kw})
    with pytest.raises(_lib.CgsError):
        overlay.compose_tracks(**{**ok, "labels": lab.cpu()})
