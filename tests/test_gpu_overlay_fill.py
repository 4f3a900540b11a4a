"""Carried objects drawn hatched on the GPU (cgs_overlay_compose_tracks_carried, cgs_amd.overlay.compose_tracks(age=)) against
tests/overlay_fill_ref.py, bit for bit, on the hand-made scene of tests/overlay_tracks_ref.py with ages mixed 0 and > 0 in one frame:
every load width, every layout, boxes 0 / 1 / 4, with and without the outline, overlapping boxes of a carried and a segmented object
both ways round, a frame at plate scale 2, and all ages <= 0 against the existing entry byte for byte."""
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

import overlay_fill_ref as ref  # noqa: E402
import overlay_ref  # noqa: E402
import overlay_tracks_ref as otr  # noqa: E402
from cgs_amd import overlay  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 6
COLOR, ALPHA = (250, 40, 7), 150
LAYOUTS = ("overlay", "side", "triple")
LABELS, IDS, TABLE = otr.scene(K)
# frame 1: the cross (1) is carried, the block inside its box (2) is not, the corner cell (3) is; a row without an area (4) has an age
# frame 2: the L (2) is segmented, the block inside its box (4) is carried; of the two single cells 5 is carried, 6 is not
AGES = {"a": np.array([[0] * 6, [3, 0, 1, 2, 0, 0], [0, 0, 5, 8, 1, 0]], dtype=np.int32),
        # the other way round: the inner boxes' owners swap with the outer ones; a negative age is no carried object
        "b": np.array([[7] * 6, [0, 2, 0, 0, -4, 0], [2, 1, 0, -1, 0, 0x7FFFFFFF]], dtype=np.int32)}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(h, w):
    rs = np.random.RandomState(1000 * h + w + 7)
    guide = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    grey = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
    hard = np.repeat(np.repeat(rs.rand(3, h // 8 + 2, w // 8 + 2) > 0.5, 8, axis=1), 8, axis=2)[:, 3:3 + h, 5:5 + w]
    hard = (hard ^ (rs.rand(3, h, w) < 0.01)).astype(np.uint8)
    for a in (guide, grey, hard):
        a.setflags(write=False)
    return guide, grey, hard


@functools.lru_cache(maxsize=None)
def _objects(h, w):
    """Per frame the object of every pixel (the slow part of the reference), once per size."""
    return tuple(otr.object_map(LABELS[f], K, h, w) for f in range(3))


@functools.lru_cache(maxsize=None)
def _decor(h, w, boxes, ages):
    return tuple(ref.decorations(TABLE[f], IDS[f], AGES[ages][f], K, h, w, boxes, overlay.FONT) for f in range(3))


@functools.lru_cache(maxsize=None)
def _panel(h, w, boxes, t, with_hard, ages):
    """ref.panel_ref from the shared pieces (the same arithmetic, line for line)."""
    guide, grey, hard = _inputs(h, w)
    s = otr.scale(h, w)
    stripe = ((np.arange(h)[:, None] + np.arange(w)[None, :]) // (2 * s)) & 1 == 0        # ref.on_stripe for all pixels at once
    edge = overlay_ref.outline_ref(hard if with_hard else None, t)
    out = np.zeros(guide.shape, dtype=np.uint8)
    for f in range(3):
        objs = _objects(h, w)[f]
        colours = np.array([otr.colour(0, COLOR)] + [otr.colour(int(IDS[f][l - 1]), COLOR) for l in range(1, K + 1)], dtype=np.int64)
        carried = np.array([False] + [int(AGES[ages][f][l - 1]) > 0 for l in range(1, K + 1)], dtype=bool)
        tint = colours[objs]
        q = np.where(carried[objs] & ~stripe, 0, ALPHA * grey[f].astype(np.int64))[..., None]
        over = (guide[f].astype(np.int64) * (65280 - q) + tint * q + 32640) // 65280
        if edge is not None:
            over = np.where(edge[f][..., None], tint, over)
        covered, rgb = _decor(h, w, boxes, ages)[f]
        out[f] = np.where(covered[..., None], rgb, over)
    return out


def _gpu(h, w, boxes, t, with_hard, layout, age, views=None, **kw):
    guide, grey, hard = (_dev(a) for a in _inputs(h, w))
    if views is not None:
        guide, grey = views(guide), views(grey)
    return overlay.compose_tracks(guide, grey, hard if with_hard else None, _dev(LABELS), _dev(IDS), _dev(TABLE), color=COLOR,
                                  alpha256=ALPHA, outline=t, boxes=boxes, layout=layout, age=None if age is None else _dev(age), **kw)


def _check(h, w, boxes, t, with_hard, layout, ages):
    guide, grey, _ = _inputs(h, w)
    got = _gpu(h, w, boxes, t, with_hard, layout, AGES[ages]).cpu().numpy()
    want = otr.lay_out(guide, grey, _panel(h, w, boxes, t, with_hard, ages), layout)
    assert got.shape == want.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w} boxes {boxes} outline {t} hard {with_hard} {layout} ages {ages}")
    return got


def test_the_shared_pieces_are_the_reference():
    guide, grey, hard = _inputs(64, 64)
    want = ref.panel_ref(guide, grey, hard, LABELS, IDS, TABLE, AGES["a"], overlay.FONT, COLOR, ALPHA, 2, 1)
    np.testing.assert_array_equal(_panel(64, 64, 1, 2, True, "a"), want)


def test_the_scene_holds_every_case():
    """Conditions on the inputs, so that the comparisons cannot pass without meeting the cases they are for."""
    h, w = 72, 100
    guide, grey, _ = _inputs(h, w)
    for ages, (f, outer, inner) in (("a", (1, 1, 2)), ("b", (1, 1, 2)), ("a", (2, 2, 4)), ("b", (2, 2, 4))):
        age = AGES[ages][f]
        assert (age[outer - 1] > 0) != (age[inner - 1] > 0)                # overlapping boxes of a carried and a segmented object
        a, b = TABLE[f, outer - 1, 1:5], TABLE[f, inner - 1, 1:5]
        assert a[0] <= b[0] and b[2] <= a[2] and a[1] <= b[1] and b[3] <= a[3]
    for ages in AGES:
        assert ((AGES[ages] > 0).any(axis=1) & (AGES[ages] <= 0).any(axis=1))[1:].all()      # mixed in one frame
        # the hatching shows: tint and border pixels differ from the plain entry's reference, and not all of a carried object's do
        plain = otr.panel_ref(guide, grey, None, LABELS, IDS, TABLE, overlay.FONT, COLOR, ALPHA, 0, 1)
        hatched = _panel(h, w, 1, 0, False, ages)
        objs = np.stack(_objects(h, w))
        carried = np.stack([np.concatenate(([False], AGES[ages][f] > 0))[objs[f]] for f in range(3)])
        differs = (plain != hatched).any(axis=-1)
        assert differs[carried].any() and not differs[carried].all() and differs[~carried].sum() < differs[carried].sum()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h, w", [(64, 64), (72, 100), (66, 70)])
def test_sizes_and_parameters(h, w, layout):
    """64 x 64: 16 pixels a thread; 72 x 100: 4; 66 x 70: 1, and rows below 64 in a last band of 2."""
    for boxes in (0, 1, 4):
        _check(h, w, boxes, 2, True, layout, "a")
    _check(h, w, 1, 0, True, layout, "b")
    _check(h, w, 4, 2, False, layout, "b")                                # hard=None: no outline


def test_scale_2():
    """512 x 520: s = 2, stripes 4 sums wide, plates of 2 x 2 font pixels; 4 pixels a thread."""
    _check(512, 520, 4, 1, True, "side", "a")


@pytest.mark.parametrize("h, w", [(64, 64), (72, 100), (66, 70), (128, 192)])
def test_all_ages_zero_is_the_existing_entry(h, w):
    """Byte for byte at every load width (128 x 192 through views that force 16, 4 and 1), every layout and every box thickness."""
    for layout in LAYOUTS:
        for boxes in (0, 1, 4):
            for shift in ((0, 4, 1) if (h, w) == (128, 192) else (0,)):
                def view(a):
                    flat = torch.empty(a.numel() + 16, dtype=torch.uint8, device=DEV)
                    v = flat[shift:shift + a.numel()].view(a.shape)
                    v.copy_(a)
                    return v
                want = _gpu(h, w, boxes, 2, True, layout, None, views=view)
                for age in (np.zeros_like(IDS), -np.abs(AGES["a"]) - (AGES["b"] > 0)):
                    got = _gpu(h, w, boxes, 2, True, layout, age, views=view)
                    assert torch.equal(got, want), (h, w, layout, boxes, shift)
    if (h, w) == (72, 100):                                               # and a carried object does change the bytes
        assert not torch.equal(_gpu(h, w, 1, 2, True, "overlay", AGES["a"]), _gpu(h, w, 1, 2, True, "overlay", None))
