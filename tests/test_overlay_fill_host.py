"""--overlay-fill without a GPU: the flag and its refusals (cli.check_video_flags), the argument errors of objects.FillStream,
objects.fill(frames=) and overlay.compose_tracks(age=), which all come before the GPU, the two C entries' declarations and argument
checks, and tests/overlay_fill_ref.py -- against tests/overlay_tracks_ref.py with all ages 0, and against stripes and borders worked out
by hand at plate scale 1 and 2."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import overlay_fill_ref as ref  # noqa: E402
import overlay_tracks_ref as otr  # noqa: E402
from cgs_amd import _lib, build, cli, objects, overlay  # noqa: E402

VIDEO = ["--model", "m", "-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4"]
TRACKS = ["--overlay-tracks", "0.3"]


# ---------------------------------------------------------------- the flag
def test_flag_parses():
    a = cli.parse_args(VIDEO + TRACKS + ["--overlay-gap", "2", "--overlay-fill"])
    assert a.overlay_fill is True and a.overlay_gap == 2 and a.overlay_tracks == 0.3
    for extra in (["--overlay-motion", "2"], ["--smooth", "2"], ["--overlay-clean", "open=1"], ["--smooth", "1", "--overlay-motion", "1"]):
        assert cli.parse_args(VIDEO + TRACKS + ["--overlay-gap", "8", "--overlay-fill"] + extra).overlay_fill is True
    assert cli.parse_args(VIDEO + TRACKS + ["--overlay-gap", "2"]).overlay_fill is False       # default off
    assert cli.parse_args(["--model", "m", "-process"]).overlay_fill is False


@pytest.mark.parametrize("argv, words", [
    (VIDEO + ["--overlay-fill"], ["--overlay-fill", "--overlay-tracks"]),
    (VIDEO + ["--overlay-gap", "2", "--overlay-fill"], ["--overlay-fill", "--overlay-tracks"]),
    (VIDEO + TRACKS + ["--overlay-fill"], ["--overlay-fill", "--overlay-gap"]),
    (VIDEO + TRACKS + ["--overlay-gap", "0", "--overlay-fill"], ["--overlay-fill", "--overlay-gap"]),
    (["--model", "m", "-process", "--overlay-fill"], ["--overlay-fill", "--source-video"]),
    (["--model", "m", "-process", "-objects", "--track-iou", "0.3", "--track-gap", "2", "--overlay-fill"], ["--overlay-fill", "--source-video"]),
])
def test_refusals_name_their_flag(argv, words):
    with pytest.raises(ValueError) as e:
        cli.parse_args(argv)
    for word in words:
        assert word in str(e.value), (word, str(e.value))


def test_track_fill_on_a_video_is_still_refused():
    for extra in ([], ["--overlay-tracks", "0.3", "--overlay-gap", "2", "--overlay-fill"]):
        with pytest.raises(ValueError, match="--track-fill with --source-video") as e:
            cli.parse_args(VIDEO + ["-objects", "--track-iou", "0.3", "--track-gap", "2", "--track-fill"] + extra)
        assert "look --overlay-gap frames" in str(e.value) and "--overlay-fill" in str(e.value)


# ---------------------------------------------------------------- argument errors come before the GPU
def test_fill_stream_arguments():
    for iou in (0, -0.5, 1.5, 0.3333, "0.5", None, True):
        with pytest.raises(ValueError):
            objects.FillStream(iou, max_gap=1)
    for g in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_gap"):
            objects.FillStream(0.3, max_gap=g)
    for k in (0, 65):
        with pytest.raises(ValueError):
            objects.FillStream(0.3, max_objects=k, max_gap=2)
    fs = objects.FillStream(0.25, max_gap=8, motion=True)
    assert (fs.iou, fs.max_objects, fs.max_gap, fs.motion) == (0.25, 64, 8, True) and int(fs.n_tracks) == 0 and fs.totals is None
    with pytest.raises(ValueError, match="nothing was pushed"):
        fs.flush()
    with pytest.raises(ValueError, match="bwd"):
        fs.push(torch.zeros((1, 64, 64), dtype=torch.int32))              # motion=True needs the vectors
    fs = objects.FillStream(0.25, max_gap=2)
    for bad in (np.zeros((1, 4, 4), dtype=np.int32), torch.zeros((1, 4, 4)), torch.zeros((4, 4), dtype=torch.int32),
                torch.zeros((0, 4, 4), dtype=torch.int32)):
        with pytest.raises(ValueError):
            fs.push(bad)
    with pytest.raises(ValueError, match="frames"):
        fs.push(torch.zeros((objects.TRACK_MAX_FRAMES - 3, 1, 1), dtype=torch.int32))     # the chunk and 2 G frames of window
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CgsError):
            fs.push(torch.zeros((1, 4, 4), dtype=torch.int32))            # objects.track has no CPU path
        assert fs._pushed == 0 and fs._labels is None                     # and the stream holds nothing of the failed push


def _cpu_tracks(n, K, G):
    z = torch.zeros((n, K), dtype=torch.int32)
    s = torch.zeros((), dtype=torch.int32)
    return objects.Tracks(z, z.clone(), s, s, s, s, torch.zeros((1, 8), dtype=torch.int32), None, None, z.clone(),
                          torch.zeros(G + 1, dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32))


def test_fill_frames_argument():
    labels = torch.zeros((5, 7, 9), dtype=torch.int32)
    tr = _cpu_tracks(5, 64, 2)
    for bad in ((0,), (0, 1, 2), 3, "01", (1.5, 2), (True, 2), (-1, 2), (3, 2), (0, 6), (6, 6)):
        with pytest.raises(ValueError, match="frames"):
            objects.fill(labels, tr, frames=bad)
    if not torch.cuda.is_available():
        for ok in (None, (0, 5), (2, 2), (5, 5), [1, 4]):
            with pytest.raises(_lib.CgsError, match="cgs_objects_track_fill"):
                objects.fill(labels, tr, frames=ok)


def test_compose_tracks_age_argument():
    n, K = 2, 6
    guide, grey = torch.zeros((n, 64, 64, 3), dtype=torch.uint8), torch.zeros((n, 64, 64), dtype=torch.uint8)
    labels, ids = torch.zeros((n, 64, 64), dtype=torch.int32), torch.zeros((n, K), dtype=torch.int32)
    table = torch.zeros((n, K, 8), dtype=torch.int32)
    for bad in (np.zeros((n, K), dtype=np.int32), torch.zeros((n, K), dtype=torch.int64), torch.zeros((n, K + 1), dtype=torch.int32),
                torch.zeros((n + 1, K), dtype=torch.int32), torch.zeros((n * K,), dtype=torch.int32)):
        with pytest.raises(ValueError, match="age"):
            overlay.compose_tracks(guide, grey, None, labels, ids, table, age=bad)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CgsError, match="cgs_overlay_compose_tracks_carried"):
            overlay.compose_tracks(guide, grey, None, labels, ids, table, age=torch.zeros((n, K), dtype=torch.int32))
        with pytest.raises(_lib.CgsError, match=r"cgs_overlay_compose_tracks\)"):
            overlay.compose_tracks(guide, grey, None, labels, ids, table)


# ---------------------------------------------------------------- the C entries
def test_entries_are_declared_and_built():
    text = open(os.path.join(REPO, "include", "cgs_hip.h")).read()
    assert re.search(r"int cgs_objects_track_fill_window\(", text) and re.search(r"int cgs_overlay_compose_tracks_carried\(", text)
    assert "0 <= f0 <= f1 <= n" in text and "((x + y) / (2 s)) & 1 == 0" in text
    assert "objects_fill.hip" in build.SOURCES and "overlay_tracks.hip" in build.SOURCES
    assert len(_lib.SIGNATURES["cgs_objects_track_fill_window"][1]) == 18 and len(_lib.SIGNATURES["cgs_overlay_compose_tracks_carried"][1]) == 22
    assert len(_lib.SIGNATURES["cgs_objects_track_fill"][1]) == 16 and len(_lib.SIGNATURES["cgs_overlay_compose_tracks"][1]) == 21      # as before
    lib = _lib.load()
    one = 1 << 12                                                         # (any non-NULL, 4-byte aligned address: nothing is dereferenced)
    keys = ("labels", "bwd", "n", "h", "w", "k", "g", "prev", "gap", "track", "f0", "f1", "out_labels", "out_track", "age", "table", "totals",
            "stream")
    base = dict(labels=one, bwd=None, n=8, h=64, w=64, k=64, g=2, prev=one, gap=one, track=one, f0=0, f1=8, out_labels=2 * one,
                out_track=one, age=one, table=None, totals=one, stream=None)
    call = lambda **kw: lib.cgs_objects_track_fill_window(*[{**base, **kw}[key] for key in keys])
    for kw in (dict(labels=None), dict(prev=None), dict(totals=None), dict(age=None), dict(f0=-1), dict(f0=5, f1=4), dict(f1=9), dict(f0=9, f1=9),
               dict(g=0), dict(g=9), dict(out_labels=one), dict(track=one + 2), dict(n=0, f1=0)):
        assert call(**kw) == _lib.ERR_BADARG, kw
    for kw in (dict(h=65), dict(k=65), dict(bwd=one, h=32)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
    keys = ("guide", "grey", "hard", "labels", "ids", "table", "age", "font", "n", "h", "w", "k", "r", "g", "b", "a", "t", "boxes", "layout",
            "flags", "out", "stream")
    base = dict(guide=one, grey=one, hard=None, labels=one, ids=one, table=one, age=one, font=one, n=1, h=64, w=64, k=64, r=0, g=255, b=0,
                a=128, t=1, boxes=1, layout=1, flags=0, out=one, stream=None)
    call = lambda **kw: lib.cgs_overlay_compose_tracks_carried(*[{**base, **kw}[key] for key in keys])
    for kw in (dict(age=None), dict(age=one + 2), dict(guide=None), dict(labels=None), dict(ids=None), dict(table=None), dict(font=None),
               dict(out=None), dict(n=0), dict(k=0), dict(boxes=5), dict(t=5), dict(layout=4), dict(flags=2), dict(a=257)):
        assert call(**kw) == _lib.ERR_BADARG, kw
    for kw in (dict(h=63), dict(w=4097), dict(k=65)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw


def test_documents_name_the_flag_and_the_entries():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "--overlay-fill" in text and "cgs_objects_track_fill_window" in text and "cgs_overlay_compose_tracks_carried" in text, doc
        assert "no fill on the video path" not in text, doc


# ---------------------------------------------------------------- the reference
def _frames(H, W, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (3, H, W), dtype=np.uint8)


@pytest.mark.parametrize("boxes, layout", [(0, "overlay"), (1, "triple"), (4, "side")])
def test_all_ages_zero_is_the_tracked_reference(boxes, layout):
    H, W = 66, 70
    labels, ids, table = otr.scene()
    guide, grey = _frames(H, W)
    hard = grey >= 128
    for age in (np.zeros_like(ids), -np.abs(ids)):                        # (a negative age is no carried object either)
        got = ref.compose_carried_ref(guide, grey, hard, labels, ids, table, age, overlay.FONT, (9, 200, 30), 128, 2, boxes, layout)
        want = otr.compose_tracks_ref(guide, grey, hard, labels, ids, table, overlay.FONT, (9, 200, 30), 128, 2, boxes, layout)
        assert np.array_equal(got, want)


def test_stripes_by_hand():
    # s = 1: (x + y) // 2 even -- sums 0, 1 on, 2, 3 off, 4, 5 on
    assert [ref.on_stripe(0, x, 1) for x in range(8)] == [True, True, False, False, True, True, False, False]
    assert [ref.on_stripe(y, 3, 1) for y in range(4)] == [False, True, True, False]
    # s = 2: (x + y) // 4 even -- sums 0..3 on, 4..7 off, 8..11 on
    assert [ref.on_stripe(0, x, 2) for x in range(12)] == [True] * 4 + [False] * 4 + [True] * 4
    assert ref.on_stripe(5, 2, 2) is False and ref.on_stripe(5, 3, 2) is True and ref.on_stripe(7, 9, 2) is True
    assert otr.scale(64, 64) == 1 and otr.scale(512, 600) == 2 and otr.scale(768, 767) == 2 and otr.scale(768, 768) == 3


def test_tint_by_hand_at_scale_1():
    labels = np.zeros((1, 64, 64), dtype=np.int32)
    labels[0, 10:20, 10:20], labels[0, 30:40, 30:40] = 1, 2
    ids, age = np.array([[5, 6]], dtype=np.int32), np.array([[2, 0]], dtype=np.int32)
    table = otr.table_of(labels, 2)
    guide, grey = np.full((1, 64, 64, 3), 100, dtype=np.uint8), np.full((1, 64, 64), 255, dtype=np.uint8)
    c5, c6 = otr.colour(5, None), otr.colour(6, None)
    half = lambda c: tuple((100 * 32640 + v * 32640 + 32640) // 65280 for v in c)
    out = ref.panel_ref(guide, grey, None, labels, ids, table, age, overlay.FONT, (9, 9, 9), 128, 0, 0)
    # object 1, carried: sums 20 and 21 are stripe 10 (on), 22 and 23 stripe 11 (off): the frame's pixel passes through
    assert tuple(out[0, 10, 10]) == half(c5) and tuple(out[0, 10, 11]) == half(c5)
    assert tuple(out[0, 10, 12]) == (100, 100, 100) and tuple(out[0, 11, 12]) == (100, 100, 100) and tuple(out[0, 12, 12]) == half(c5)
    # object 2, segmented: whole, on and off the stripe (sums 60: on, 62: off)
    assert tuple(out[0, 30, 30]) == half(c6) and tuple(out[0, 30, 32]) == half(c6)
    # no object: the default colour, on and off the stripe
    assert tuple(out[0, 0, 0]) == half((9, 9, 9)) and tuple(out[0, 0, 2]) == half((9, 9, 9))
    # with boxes: the plate (7 x 9 from (10, 10)) is whole, the border hatched: row 19 is the bottom border, outside the plate
    out = ref.panel_ref(guide, grey, None, labels, ids, table, age, overlay.FONT, (9, 9, 9), 128, 0, 1)
    assert tuple(out[0, 10, 12]) == c5 and tuple(out[0, 10, 16]) == c5    # the plate's top row, sums 22 (off) and 26 (off): still drawn
    assert tuple(out[0, 19, 13]) == c5                                    # sum 32, stripe 16: border
    assert tuple(out[0, 19, 11]) == (100, 100, 100)                       # sum 30, stripe 15: no border, and a carried pixel without tint
    assert tuple(out[0, 10, 17]) == (100, 100, 100) and tuple(out[0, 10, 19]) == c5      # the top border right of the plate: sums 27 (stripe 13: off), 29 (14: on)
    assert tuple(out[0, 39, 31]) == c6 and tuple(out[0, 39, 33]) == c6    # object 2's border is whole (sums 70: off, 72: on)


def test_overlapping_borders_by_hand():
    """Object 1 (cells 20..39 square, track 5) and object 2 (cells 10..30 x 30..50, track 6) at 64 x 64; the plates (7 x 9 from each top
    left corner) reach none of the pixels below.  (30, 20) lies on the left border of 1 and the top border of 2, its sum 50 is stripe 25:
    off.  (39, 30), bottom border of 1 and right border of 2, sum 69, stripe 34: on."""
    tab = np.zeros((2, 8), dtype=np.int32)
    tab[0], tab[1] = [400, 20, 20, 39, 39, 0, 0, 0], [441, 10, 30, 30, 50, 0, 0, 0]
    ids = np.array([5, 6])
    c5, c6 = otr.colour(5, None), otr.colour(6, None)
    deco = lambda age, y, x: ref.decoration_of_pixel(tab, ids, np.array(age), 2, y, x, 64, 64, 1, overlay.FONT)
    assert deco([0, 0], 30, 20) == c5 and deco([3, 0], 30, 20) == c6 and deco([0, 3], 30, 20) == c5 and deco([3, 3], 30, 20) is None
    assert deco([0, 0], 39, 30) == c5 and deco([3, 0], 39, 30) == c5 and deco([3, 3], 39, 30) == c5
    # 1's bottom border alone: (39, 25) sum 64, stripe 32, on; (39, 27) sum 66, stripe 33, off and inside 2's box, which has no border there
    assert deco([3, 0], 39, 25) == c5 and deco([3, 0], 39, 27) is None and deco([0, 0], 39, 27) == c5
    # 2's top border alone: (30, 18) sum 48, stripe 24, on; (30, 21) sum 51, stripe 25, off and inside 1's box
    assert deco([0, 3], 30, 18) == c6 and deco([0, 3], 30, 21) is None and deco([0, 0], 30, 21) == c6 and deco([3, 0], 30, 21) == c6
    # without a track an object has no box, carried or not
    assert ref.decoration_of_pixel(tab, np.array([0, 6]), np.array([3, 0]), 2, 39, 25, 64, 64, 1, overlay.FONT) is None


def test_border_by_hand_at_scale_2():
    """512 x 512: a cell is 8 pixels, s = 2, a stripe 4 sums wide.  The box of cells 2..5 is the pixels 16..47; the plate of a 1-digit
    number is 14 x 18 from (16, 16); the border is 2 thick: rows 46 and 47 at the bottom."""
    tab = np.zeros((1, 8), dtype=np.int32)
    tab[0] = [16, 2, 2, 5, 5, 0, 0, 0]
    ids, c7 = np.array([7]), otr.colour(7, None)
    deco = lambda age, y, x: ref.decoration_of_pixel(tab, ids, np.array([age]), 1, y, x, 512, 512, 2, overlay.FONT)
    assert deco(1, 47, 17) == c7 and deco(1, 47, 20) == c7                # sums 64 and 67: stripe 16, on
    assert deco(1, 47, 21) is None and deco(1, 47, 24) is None and deco(0, 47, 21) == c7      # sums 68 and 71: stripe 17, off
    assert deco(1, 46, 21) == c7 and deco(1, 46, 22) is None              # the second border row: sum 67 on, 68 off
    assert deco(1, 40, 40) is None and deco(0, 40, 40) is None            # inside the box: no border either way
    assert deco(1, 16, 24) == c7 and deco(1, 16, 29) == c7 and deco(1, 17, 28) == c7          # the plate is whole: sums 40 (on), 45, 45 (off)
