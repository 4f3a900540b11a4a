"""--overlay-tracks without a GPU: the flag table of cli.check_video_flags, overlay.FONT, tests/overlay_tracks_ref.py against
expectations written out by hand (the pixels of a run of cells, a plate and its digits, a tie of the nearest-cell search, the priority of
overlapping boxes), objects.stream_remap on a hand-made result, and the C entry's declaration."""
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

import overlay_tracks_ref as ref  # noqa: E402
from cgs_amd import _lib, build, cli, fit, objects, overlay  # noqa: E402

VIDEO = ["--model", "m", "-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4"]


# ---------------------------------------------------------------- the flags
def test_flags_parse_and_fill_in_defaults():
    a = cli.parse_args(VIDEO + ["--overlay-tracks", "0.3"])
    assert (a.overlay_tracks, a.overlay_min_area, a.overlay_boxes) == (0.3, 1, 1) and a.fit
    a = cli.parse_args(VIDEO + ["--overlay-tracks", "1", "--overlay-min-area", "9", "--overlay-boxes", "0"])
    assert (a.overlay_tracks, a.overlay_min_area, a.overlay_boxes) == (1.0, 9, 0)
    a = cli.parse_args(VIDEO + ["--overlay-tracks", "0.001", "--overlay-boxes", "4"])
    assert (a.overlay_tracks, a.overlay_boxes) == (0.001, 4)
    a = cli.parse_args(VIDEO)                                             # without the flag nothing is filled in
    assert a.overlay_tracks is None and a.overlay_min_area is None and a.overlay_boxes is None


@pytest.mark.parametrize("argv, words", [
    (["--model", "m", "-process", "--overlay-tracks", "0.3"], ["--overlay-tracks", "belong to --source-video"]),
    (["--model", "m", "-process", "--overlay-min-area", "2"], ["--overlay-min-area", "belong to --source-video"]),
    (["--model", "m", "-process", "-objects", "--overlay-boxes", "2"], ["--overlay-boxes", "belong to --source-video"]),
    (VIDEO + ["--overlay-min-area", "2"], ["--overlay-min-area", "--overlay-tracks"]),
    (VIDEO + ["--overlay-boxes", "2"], ["--overlay-boxes", "--overlay-tracks"]),
    (VIDEO + ["--overlay-min-area", "2", "--overlay-boxes", "0"], ["--overlay-min-area", "--overlay-boxes", "--overlay-tracks"]),
    (VIDEO + ["--overlay-tracks", "0.3", "--binarymaskthreshold", "0"], ["--overlay-tracks", "--binarymaskthreshold 0"]),
    (VIDEO + ["--overlay-tracks", "0"], ["--overlay-tracks", "(0, 1]"]),
    (VIDEO + ["--overlay-tracks", "1.001"], ["--overlay-tracks", "(0, 1]"]),
    (VIDEO + ["--overlay-tracks", "0.3333"], ["--overlay-tracks", "thousandths"]),
    (VIDEO + ["--overlay-tracks", "0.3-0.5"], ["--overlay-tracks", "one number"]),
    (VIDEO + ["--overlay-tracks", "nan"], ["--overlay-tracks"]),
    (VIDEO + ["--overlay-tracks", "0.3", "--overlay-min-area", "0"], ["--overlay-min-area"]),
    (VIDEO + ["--overlay-tracks", "0.3", "--overlay-min-area", "-4"], ["--overlay-min-area"]),
    (VIDEO + ["--overlay-tracks", "0.3", "--overlay-boxes", "5"], ["--overlay-boxes", "0..4"]),
    (VIDEO + ["--overlay-tracks", "0.3", "--overlay-boxes", "-1"], ["--overlay-boxes", "0..4"]),
])
def test_refusals_name_their_flag(argv, words):
    with pytest.raises(ValueError) as e:
        cli.parse_args(argv)
    for word in words:
        assert word in str(e.value), (word, str(e.value))
    assert "--track-iou" not in str(e.value)                              # the parser is --track-iou's, the message is not


def test_objects_on_a_video_is_still_refused():
    for extra in ([], ["--overlay-tracks", "0.3"]):
        with pytest.raises(ValueError) as e:
            cli.parse_args(VIDEO + ["-objects"] + extra)
        assert "-objects" in str(e.value) and "outside this build" in str(e.value)
    for flag in ("--track-iou", "--min-area", "--connectivity"):          # and these still belong to -objects
        with pytest.raises(ValueError, match="belong to -objects"):
            cli.parse_args(VIDEO + ["--overlay-tracks", "0.3", flag, "0.5" if flag == "--track-iou" else "8"])


# ---------------------------------------------------------------- the font
def test_font():
    f = overlay.FONT
    assert f.dtype == np.uint8 and f.shape == (10, 7) == (_lib.OVERLAY_FONT_GLYPHS, _lib.OVERLAY_FONT_ROWS) and not f.flags.writeable
    assert (f <= 0b11111).all()                                           # bits 0..4 only
    assert all(g.any() for g in f) and len({g.tobytes() for g in f}) == 10
    text = open(os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd", "csrc", "overlay_tracks.hip")).read()
    assert "font[" in text and not re.search(r"0b[01]{5}|0x[0-9a-fA-F]{2}\s*,\s*0x[0-9a-fA-F]{2}\s*,", text)     # no second table in the kernel
    assert overlay.scale(64, 64) == 1 and overlay.scale(255, 4096) == 1 and overlay.scale(512, 600) == 2 and overlay.scale(4096, 4096) == 16
    for ok in (0, 1, 4):
        assert overlay.check_boxes(ok) == ok
    for bad in (-1, 5, True, 1.0, "1"):
        with pytest.raises(ValueError):
            overlay.check_boxes(bad)


# ---------------------------------------------------------------- the reference, by hand
def test_colour_is_the_track_painters():
    import objects_track_ref
    for t in (1, 2, 10, 255, 8388607, 2 ** 31 - 1):
        assert ref.colour(t, None) == tuple(int(v) for v in objects_track_ref.colours(np.array([t]))[0])
        assert min(ref.colour(t, None)) >= 64
    assert ref.colour(1, None) == (64 + 0xB1 * 191 // 255, 64 + 0x79 * 191 // 255, 64 + 0x37 * 191 // 255)       # 2654435761 = 0x9E3779B1
    assert ref.colour(0, (1, 2, 3)) == (1, 2, 3) == ref.colour(-5, (1, 2, 3))


def test_cells_tile_the_pixels():
    assert ref.cell_pixels(3, 5, 64) == (3, 5)
    assert ref.cell_pixels(3, 5, 100) == (5, 8)
    assert ref.cell_pixels(3, 5, 1080) == (51, 100)
    for L in (64, 65, 100, 127, 1080, 4096):                              # the tiling is fit.home_cells': a pixel lies in its home cell's run
        homes = fit.home_cells(L)
        for c in range(64):
            a, b = ref.cell_pixels(c, c, L)
            assert list(np.flatnonzero(homes == c)) == list(range(a, b + 1)), (L, c)
        assert ref.cell_pixels(0, 63, L) == (0, L - 1)


PLATE_10 = """
.............
...#....###..
..##...#...#.
...#...#..##.
...#...#.#.#.
...#...##..#.
...#...#...#.
..###...###..
.............
"""


def test_plate_and_digits_of_track_10():
    """An object whose box starts at cell (x 2, y 3) of a 64 x 64 frame, s = 1: a plate of 13 x 9 pixels from (2, 3)."""
    tab = np.zeros((2, 8), dtype=np.int32)
    tab[0] = [40, 2, 3, 30, 20, 0, 0, 0]
    ids = np.array([10, 0], dtype=np.int32)
    c10 = ref.colour(10, None)
    rows = PLATE_10.strip().split("\n")
    assert len(rows) == 9 and all(len(r) == 13 for r in rows)
    for py, row in enumerate(rows):
        for px, ch in enumerate(row):
            got = ref.decoration_of_pixel(tab, ids, 2, 3 + py, 2 + px, 64, 64, 1, overlay.FONT)
            assert got == ((0, 0, 0) if ch == "#" else c10), (px, py)
    dec = lambda y, x, B=1: ref.decoration_of_pixel(tab, ids, 2, y, x, 64, 64, B, overlay.FONT)
    assert dec(3, 15) == c10 and dec(4, 15) is None and dec(4, 15, B=2) == c10 and dec(12, 3) is None     # right of / below the plate
    assert dec(20, 30) == c10 and dec(21, 30) is None and dec(20, 31) is None and dec(2, 2) is None        # the rectangle's far corner
    assert dec(17, 27, B=4) == c10 and dec(16, 26, B=4) is None
    assert dec(3, 2, B=0) is None                                         # no boxes, no numbers
    # s = 2 on a 600 x 520 frame: the same glyphs, every font pixel 2 x 2
    X0, Y0 = ref.cell_pixels(2, 2, 520)[0], ref.cell_pixels(3, 3, 600)[0]
    for py, row in enumerate(rows):
        for px, ch in enumerate(row):
            for sy in (0, 1):
                for sx in (0, 1):
                    got = ref.decoration_of_pixel(tab, ids, 2, Y0 + 2 * py + sy, X0 + 2 * px + sx, 600, 520, 1, overlay.FONT)
                    assert got == ((0, 0, 0) if ch == "#" else c10), (px, py, sx, sy)
    # clipped by the frame, not by the rectangle: a one-cell object in the bottom right corner.  Object 1: a plate of 13 x 9 and a border
    # of 29 x 18 pixels that share 13 + 9 - 1 pixels
    tab[1], ids[1] = [1, 63, 63, 63, 63, 63, 63, 4095], 12
    covered, rgb = ref.decorations(tab, ids, 2, 64, 64, 1, overlay.FONT)
    assert covered[63, 63] and tuple(rgb[63, 63]) == ref.colour(12, None) and covered.sum() == 13 * 9 + (2 * 29 + 2 * 18 - 4 - 21) + 1


def test_nearest_cell_and_its_ties():
    lab = np.zeros((64, 64), dtype=np.int32)
    lab[10, 9], lab[10, 11] = 2, 1
    assert ref.object_of_pixel(lab, 4, 10, 10, 64, 64) == 2               # left and right are equally far: the first in raster order
    lab[9, 10] = 3
    assert ref.object_of_pixel(lab, 4, 10, 10, 64, 64) == 3               # above comes before left
    assert ref.object_of_pixel(lab, 4, 10, 9, 64, 64) == 2                # a labelled home cell is its own answer
    assert ref.object_of_pixel(lab, 4, 12, 13, 64, 64) == 1 and ref.object_of_pixel(lab, 4, 13, 13, 64, 64) == 0      # radius 2, not 3
    assert ref.object_of_pixel(lab, 2, 10, 10, 64, 64) == 2               # a label above K is not found ...
    lab[10, 10] = 9
    assert ref.object_of_pixel(lab, 4, 10, 10, 64, 64) == 0               # ... and on the home cell it ends the search
    # between two cells at 100 pixels a side the nearer centre wins: cells 9 and 12 have their centres at 14.84 and 19.53 pixels, the
    # pixels 16, 17, 18 between them (homes 10, 11, 11) theirs at 16.5, 17.5, 18.5
    lab = np.zeros((64, 64), dtype=np.int32)
    lab[10, 9], lab[10, 12] = 2, 1
    y = ref.cell_pixels(10, 10, 100)[0]
    assert [ref.home(x, 100) for x in (15, 16, 17, 18, 19)] == [9, 10, 11, 11, 12]
    assert [ref.object_of_pixel(lab, 4, y, x, 100, 100) for x in (15, 16, 17, 18, 19)] == [2, 2, 1, 1, 1]
    assert ref.object_of_pixel(lab, 4, 0, 0, 100, 100) == 0 and ref.object_of_pixel(lab[::-1, ::-1], 4, 99, 99, 100, 100) == 0


def test_priority_where_boxes_overlap():
    """Object 1 (track 8) x 10..30, y 10..30 and object 2 (track 7) x 30..50, y 5..20 share the column x = 30."""
    tab = np.zeros((2, 8), dtype=np.int32)
    tab[0], tab[1] = [5, 10, 10, 30, 30, 0, 0, 0], [5, 30, 5, 50, 20, 0, 0, 0]
    ids = np.array([8, 7], dtype=np.int32)
    dec = lambda y, x, B=1: ref.decoration_of_pixel(tab, ids, 2, y, x, 64, 64, B, overlay.FONT)
    assert dec(15, 30) == ref.colour(8, None)                             # two borders: the smaller label, not the smaller track
    assert dec(10, 30) == ref.colour(7, None)                             # object 2's plate (margin column) over object 1's corner
    assert dec(10, 32) == (0, 0, 0) and dec(10, 33) == ref.colour(7, None)     # ... and its digit: 7's row 4 is 01000
    assert dec(12, 11) == (0, 0, 0) and dec(12, 12) == ref.colour(8, None) and dec(10, 11) == ref.colour(8, None)     # 8's row 1 is 10001
    assert dec(20, 40) == ref.colour(7, None) and dec(19, 40) is None and dec(17, 40, B=4) == ref.colour(7, None)
    # plate over plate: the smaller label
    tab[1, 1:5] = [12, 12, 50, 20]
    assert dec(13, 13) == ref.colour(8, None) == dec(13, 13, B=3)         # inside both plates: object 1's (8's row 2 is 10001), not 7's top bar
    assert dec(13, 17) == (0, 0, 0) and dec(12, 19) == ref.colour(7, None)      # right of object 1's plate: 7's top bar; then object 2's border
    # the whole panel: decoration, then outline, then tint
    guide = np.full((1, 64, 64, 3), 100, dtype=np.uint8)
    grey = np.full((1, 64, 64), 255, dtype=np.uint8)
    hard = np.zeros((1, 64, 64), dtype=np.uint8)
    hard[0, 40:50, 40:50] = 1
    labels = np.zeros((1, 64, 64), dtype=np.int32)
    labels[0, 40:50, 40:50] = 1
    full = np.zeros((1, 2, 8), dtype=np.int32)
    full[0, 0] = [100, 40, 40, 49, 49, 0, 0, 0]
    out = ref.panel_ref(guide, grey, hard, labels, np.array([[8, 0]], dtype=np.int32), full, overlay.FONT, (9, 9, 9), 128, 2, 1)
    c8, half = ref.colour(8, None), lambda c: tuple((100 * 32640 + v * 32640 + 32640) // 65280 for v in c)
    assert tuple(out[0, 49, 49]) == c8 and tuple(out[0, 48, 48]) == c8    # border, then the outline of thickness 2 in the object's colour
    assert tuple(out[0, 47, 47]) == half(c8) and tuple(out[0, 0, 0]) == half((9, 9, 9)) and tuple(out[0, 45, 45]) == (0, 0, 0)   # 8's row 4
    assert tuple(out[0, 51, 45]) == half(c8) and tuple(out[0, 52, 45]) == half((9, 9, 9))     # two cells off: the object's, three: the default


# ---------------------------------------------------------------- the stream's arithmetic
def test_stream_remap_by_hand():
    """A carried frame with objects 1 and 2 (stream numbers 7 and 9) and no object 3; 11 tracks so far.  In the joint run the carried
    objects head the local tracks 1 and 2; local 3 and 4 are new: 12 and 13."""
    local = torch.tensor([[3, 0, 1], [4, 2, 0]], dtype=torch.int32)
    got = objects.stream_remap(local, torch.tensor([1, 2, 0], dtype=torch.int32), torch.tensor([7, 9, 0], dtype=torch.int32), 2, 11)
    assert got.tolist() == [[12, 0, 7], [13, 9, 0]]
    got = objects.stream_remap(local, torch.tensor([1, 2, 0]), torch.tensor([7, 9, 0]), torch.tensor(2), torch.tensor(11, dtype=torch.int32))
    assert got.tolist() == [[12, 0, 7], [13, 9, 0]] and got.dtype == torch.int64
    # an empty carried frame: every local number is new
    got = objects.stream_remap(torch.tensor([[1, 2], [1, 3]]), torch.tensor([0, 0]), torch.tensor([0, 0]), 0, 5)
    assert got.tolist() == [[6, 7], [6, 8]]
    # the largest local number a chunk can hold fits the table
    m, K = 3, 2
    local = torch.arange(1, m * K + 1).reshape(m, K) + K
    got = objects.stream_remap(local, torch.tensor([1, 2]), torch.tensor([4, 2]), 2, 4)
    assert got.tolist() == [[5, 6], [7, 8], [9, 10]]


def test_stream_arguments_without_a_gpu():
    for iou in (0, -0.5, 1.5, 0.3333, "0.5", None, True):
        with pytest.raises(ValueError):
            objects.TrackStream(iou)
    for k in (0, 65, 1.5):
        with pytest.raises(ValueError):
            objects.TrackStream(0.5, max_objects=k)
    ts = objects.TrackStream(0.25)
    assert ts.iou == 0.25 and ts.max_objects == 64 and int(ts.n_tracks) == 0
    for bad in (np.zeros((1, 4, 4), dtype=np.int32), torch.zeros((1, 4, 4)), torch.zeros((4, 4), dtype=torch.int32),
                torch.zeros((0, 4, 4), dtype=torch.int32)):
        with pytest.raises(ValueError):
            ts.push(bad)
    with pytest.raises(ValueError, match="frames"):
        ts.push(torch.zeros((objects.TRACK_MAX_FRAMES, 1, 1), dtype=torch.int32))
    with pytest.raises(_lib.CgsError):
        ts.push(torch.zeros((1, 4, 4), dtype=torch.int32))                # objects.track has no CPU path


# ---------------------------------------------------------------- the C entry
def test_entry_is_declared_and_built():
    text = open(os.path.join(REPO, "include", "cgs_hip.h")).read()
    assert re.search(r"int cgs_overlay_compose_tracks\(", text)
    assert re.search(r"CGS_OVERLAY_MAX_TRACK_OBJECTS\s*=\s*64\b", text) and re.search(r"CGS_OVERLAY_MAX_BOXES\s*=\s*4\b", text)
    assert re.search(r"CGS_OVERLAY_FONT_GLYPHS\s*=\s*10\b", text) and re.search(r"CGS_OVERLAY_FONT_ROWS\s*=\s*7\b", text)
    assert "overlay_tracks.hip" in build.SOURCES and "cgs_overlay_compose_tracks" in _lib.SIGNATURES
    assert (overlay.MAX_TRACK_OBJECTS, overlay.MAX_BOXES) == (64, 4) == (objects.MATCH_MAX_OBJECTS, overlay.MAX_OUTLINE)
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    # bad arguments are refused before anything touches a device
    one = 1 << 12                                                         # (any non-NULL, 4-byte aligned address: nothing is dereferenced)
    call = lambda **kw: lib.cgs_overlay_compose_tracks(*[{**dict(guide=one, grey=one, hard=None, labels=one, ids=one, table=one, font=one, n=1,
                                                                 h=64, w=64, k=64, r=0, g=255, b=0, a=128, t=1, boxes=1, layout=1, flags=0,
                                                                 out=one, stream=None), **kw}[key]
                                                         for key in ("guide", "grey", "hard", "labels", "ids", "table", "font", "n", "h", "w", "k",
                                                                     "r", "g", "b", "a", "t", "boxes", "layout", "flags", "out", "stream")])
    for kw in (dict(guide=None), dict(labels=None), dict(ids=None), dict(table=None), dict(font=None), dict(out=None), dict(ids=one + 1),
               dict(n=0), dict(k=0), dict(boxes=5), dict(boxes=-1), dict(t=5), dict(layout=4), dict(flags=2), dict(a=257), dict(r=256)):
        assert call(**kw) == _lib.ERR_BADARG, kw
    for kw in (dict(h=63), dict(w=4097), dict(k=65)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
