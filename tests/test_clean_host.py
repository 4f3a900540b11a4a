"""CPU checks of the mask clean-up's host side: the checker of tests/clean_ref.py against scipy.ndimage and against the figures the
feature was specified with, the algebra of opening and closing under the frame-edge rule, clean.parse_clean, the CLI's refusals, the
argument checks of cgs_amd.clean and of the entry point.  Nothing here needs a GPU."""
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

import clean_ref  # noqa: E402
import objects_ref  # noqa: E402
from cgs_amd import _lib, build, clean, cli  # noqa: E402

PATTERNS = objects_ref.patterns()
SQUARE = np.ones((3, 3), dtype=bool)
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def _hole_figures(on, conn, fill_area):
    found = clean_ref.holes(on, conn)
    small = [c for c in found if len(c) <= fill_area]
    return len(found), len(small), sum(len(c) for c in small)


# ---------------------------------------------------------------- the checker
def test_checker_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(2)
    frames = dict(PATTERNS)
    frames.update({"5x7": rs.rand(5, 7) < 0.5, "17x33": rs.rand(17, 33) < 0.6, "1x1": np.ones((1, 1), dtype=bool)})
    for name, on in frames.items():
        for shape, element in (("square", SQUARE), ("cross", CROSS)):
            for r in (1, 2):
                np.testing.assert_array_equal(clean_ref.erode(on, r, shape),
                                              ndimage.binary_erosion(on, structure=element, iterations=r, border_value=1), err_msg=name)
                np.testing.assert_array_equal(clean_ref.dilate(on, r, shape),
                                              ndimage.binary_dilation(on, structure=element, iterations=r, border_value=0), err_msg=name)
        for conn, hole_element in ((8, CROSS), (4, SQUARE)):                      # the holes are connected the complementary way
            filled, found, done = clean_ref.fill_holes(on, 4096, conn)
            assert found == done
            np.testing.assert_array_equal(filled, ndimage.binary_fill_holes(on, structure=hole_element), err_msg=f"{name} {conn}")
            # hysteresis by labels: a component stays when the strong mask marks one of its pixels
            strong = on & (rs.rand(*on.shape) < 0.02)
            labels, k = ndimage.label(on, structure=SQUARE if conn == 8 else CROSS)
            marked = np.unique(labels[strong])
            want = np.isin(labels, marked[marked > 0])
            kept, dropped = clean_ref.hysteresis(on, strong, conn)
            np.testing.assert_array_equal(kept, want, err_msg=f"{name} {conn}")
            assert dropped == k - len(marked[marked > 0])


@pytest.mark.parametrize("shape", ["square", "cross"])
def test_open_inside_input_inside_close_and_idempotent(shape):
    rs = np.random.RandomState(3)
    frames = dict(PATTERNS)
    frames["17x33"] = rs.rand(17, 33) < 0.6
    for name, on in frames.items():
        for r in (1, 2, 3, 4):
            lo, hi = clean_ref.opening(on, r, shape), clean_ref.closing(on, r, shape)
            assert not (lo & ~on).any() and not (on & ~hi).any(), (name, r)
            np.testing.assert_array_equal(clean_ref.opening(lo, r, shape), lo, err_msg=f"{name} {r}")
            np.testing.assert_array_equal(clean_ref.closing(hi, r, shape), hi, err_msg=f"{name} {r}")


def test_pinned_figures():
    """Statements about the checker under the stated rules: every switch is observable."""
    r45 = PATTERNS["random0.45"]
    assert _hole_figures(r45, 8, 4096) == (186, 186, 1474)
    assert _hole_figures(r45, 8, 4) == (186, 145, 207)
    for fill_area in (1, 4, 4096):
        assert _hole_figures(r45, 4, fill_area) == (5, 5, 5)
    assert _hole_figures(PATTERNS["checkerboard"], 8, 1) == (1922, 1922, 1922)
    assert _hole_figures(PATTERNS["checkerboard"], 4, 4096)[0] == 0
    assert clean_ref.opening(PATTERNS["random0.593"], 1, "square").sum() == 292
    assert clean_ref.opening(PATTERNS["random0.593"], 1, "cross").sum() == 1135
    assert clean_ref.closing(PATTERNS["random0.3"], 1, "square").sum() == 3214
    assert clean_ref.closing(PATTERNS["random0.3"], 1, "cross").sum() == 2229
    for name in ("spiral", "comb", "serpentine"):
        assert clean_ref.holes(PATTERNS[name], 4) == [] and clean_ref.holes(PATTERNS[name], 8) == []


def test_checker_counts_and_gated():
    v = np.zeros((1, 6, 7), dtype=np.float32)
    v[0, 1:5, 1:5] = 0.6
    v[0, 2, 2] = 0.1                                   # a one-pixel hole
    v[0, 1, 1] = 0.9                                   # the strong pixel
    v[0, 5, 6] = 0.7                                   # a weak speck
    v[0, 0, 6] = np.nan
    got = clean_ref.clean(v, thresh=0.5, inclusive=True, strong=0.8, fill=1, want_gated=True)
    assert got.counts.tolist() == [[16, 15, 15, 15, 16, 1, 1, 1]]
    assert got.mask[0, 2, 2] and not got.mask[0, 5, 6] and not got.mask[0, 0, 6]
    assert got.gated[0, 2, 2] == np.float32(0.5) and got.gated[0, 1, 1] == np.float32(0.9) and got.gated[0, 5, 6] == 0
    np.testing.assert_array_equal(got.gated >= np.float32(0.5), got.mask)


# ---------------------------------------------------------------- the parser
def test_parse_clean():
    assert clean.parse_clean("hyst=0.8;open=1;close=2;fill=16;shape=cross;conn=4") == \
        {"hyst": 0.8, "open": 1, "close": 2, "fill": 16, "shape": "cross", "conn": 4}
    assert clean.parse_clean("fill=4096") == {"hyst": None, "open": 0, "close": 0, "fill": 4096, "shape": "square", "conn": 8}
    assert clean.parse_clean(" conn=4 ; open = 4 ") == {"hyst": None, "open": 4, "close": 0, "fill": 0, "shape": "square", "conn": 4}
    assert clean.parse_clean("hyst=0.5")["hyst"] == 0.5
    assert clean.spec_text(clean.parse_clean("close=1;hyst=0.75")) == "hyst=0.75;open=0;close=1;fill=0;shape=square;conn=8"
    for bad in ("", "open=1;", ";open=1", "open=1;;close=1", "open", "open=", "=1", "erode=1", "open=1;open=2", "open=one", "open=1.5",
                "open=5", "open=-1", "close=5", "fill=4097", "fill=-1", "fill=2.0", "hyst=nan", "hyst=inf", "hyst=-inf", "hyst=high",
                "shape=disc", "conn=6", "conn=eight", "shape=cross", "conn=4", "open=0;close=0;fill=0", "shape=square;conn=8",
                "open=1,2"):
        with pytest.raises(ValueError, match="--clean"):
            clean.parse_clean(bad)
    with pytest.raises(ValueError, match="--overlay-clean"):
        clean.parse_clean("open=9", "--overlay-clean")


def test_clean_report():
    spec = clean.parse_clean("open=1;fill=4")
    counts = np.array([[10, 10, 8, 8, 9, 0, 2, 1], [5, 5, 5, 5, 5, 0, 0, 0]], dtype=np.int32)
    want = {"spec": spec, "frames": 2, "on": 15, "after_hyst": 15, "after_open": 13, "after_close": 13, "after_fill": 14,
            "components_dropped": 0, "holes_found": 2, "holes_filled": 1}
    assert clean.clean_report(counts, spec) == want
    assert clean.clean_report(torch.from_numpy(counts), spec) == want


# ---------------------------------------------------------------- the command line
def test_cli_clean_flags_parse_and_refuse():
    a = cli.parse_args([])
    assert a.clean is None and a.overlay_clean is None
    a = cli.parse_args(["-process", "--clean", "open=1;fill=4"])
    assert a.clean == {"hyst": None, "open": 1, "close": 0, "fill": 4, "shape": "square", "conn": 8}
    assert cli.parse_args(["-eval", "--clean", "hyst=0.8"]).clean["hyst"] == 0.8
    assert cli.parse_args(["-process", "-fit", "--clean", "close=2"]).clean["close"] == 2
    assert cli.parse_args(["-process", "-concatenated", "--clean", "hyst=0.5"]).clean["hyst"] == 0.5          # hyst = the threshold
    assert cli.parse_args(["-process", "-crf", "--clean", "fill=8", "--binarymaskthreshold", "0"]).clean["fill"] == 8
    assert cli.parse_args(["-process", "-objects", "--track-iou", "0.5", "--clean", "open=1"]).clean["open"] == 1
    a = cli.parse_args(["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--overlay-clean", "hyst=0.9;close=1"])
    assert a.overlay_clean["hyst"] == 0.9 and a.clean is None
    for bad in (["--clean", "open=1"], ["-train", "--clean", "open=1"],                                      # neither -process nor -eval
                ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--clean", "open=1"],  # --overlay-clean there
                ["-process", "--overlay-clean", "open=1"], ["-eval", "--overlay-clean", "open=1"],            # no --source-video
                ["-process", "--clean", "open=5"], ["-eval", "--clean", "conn=4"], ["-process", "--clean", "open=1;;fill=2"],
                ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--overlay-clean", "fill=-1"],
                ["-process", "-crf", "--clean", "hyst=0.8"], ["-eval", "-crf", "--clean", "hyst=0.8;open=1"],  # a hard source
                ["-process", "--clean", "hyst=0.4"], ["-process", "--binarymaskthreshold", "0.7", "--clean", "hyst=0.6"],
                ["-eval", "--eval-thresh", "0.5", "--clean", "hyst=0.4"],
                ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--overlay-clean", "hyst=0.3"],
                ["-process", "--binarymaskthreshold", "0", "--clean", "open=1"],
                ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--binarymaskthreshold", "0", "--overlay-clean",
                 "open=1"]):
        with pytest.raises(ValueError, match="clean"):
            cli.parse_args(bad)
    with pytest.raises(ValueError):
        cli.main(["--clean", "open=1", "--source-imgs", "nowhere"])    # before a Handler (a GPU) is asked for


# ---------------------------------------------------------------- the library
def test_clean_argument_errors():
    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    for bad in (dict(connectivity=6), dict(shape="disc"), dict(open=5), dict(close=-1), dict(open=1.5), dict(fill=4097), dict(fill=-1),
                dict(fill=True), dict(thresh=0.5), dict(strong=0.5), dict(want_gated=True)):
        with pytest.raises(ValueError):
            clean.clean(m, **bad)
    f = m.float()
    for bad in (dict(), dict(thresh=float("nan")), dict(thresh=0.5, strong=0.4), dict(thresh=0.5, strong=float("inf")),
                dict(thresh=0.5, strong=float("nan")), dict(thresh=0.0, want_gated=True), dict(thresh=-1.0, want_gated=True)):
        with pytest.raises(ValueError):
            clean.clean(f, **bad)
    with pytest.raises(ValueError):
        clean.clean(m.double(), thresh=0.5)
    with pytest.raises(ValueError):
        clean.clean(m.to(torch.int32))
    for shape in ((8,), (1, 2, 8, 8), (2, 65, 8), (2, 8, 65), (0, 8, 8), (2, 0, 8)):
        with pytest.raises(ValueError):
            clean.clean(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        clean.clean(np.zeros((2, 8, 8), dtype=bool))


def test_no_cpu_path():
    """A tensor in host memory: CgsError, with or without a GPU in the machine."""
    with pytest.raises(_lib.CgsError):
        clean.clean(torch.zeros(2, 8, 8, dtype=torch.bool), open=1)
    with pytest.raises(_lib.CgsError):
        clean.clean(torch.rand(8, 8), thresh=0.5, inclusive=True, strong=0.8, want_gated=True)


def test_clean_entry_point_is_declared_and_checks_its_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_mask_clean\s*\(", text)
    assert "CGS_CLEAN_FIELDS = 8" in text and "CGS_CLEAN_MAX_RADIUS = 4" in text
    assert "clean.hip" in build.SOURCES and "cgs_mask_clean" in _lib.SIGNATURES
    lib = _lib.load()
    # argument checks come before anything is launched: safe without a GPU (the pointers are never followed)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    ok = dict(src=p, kind=2, thresh=0.5, hyst=0, strong=0.0, n=1, h=4, w=4, conn=8, shape=0, open=0, close=0, fill=0, out=p, gated=None,
              counts=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cgs_mask_clean(a["src"], a["kind"], a["thresh"], a["hyst"], a["strong"], a["n"], a["h"], a["w"], a["conn"], a["shape"],
                                  a["open"], a["close"], a["fill"], a["out"], a["gated"], a["counts"], None)

    for bad in (dict(src=None), dict(out=None), dict(counts=None), dict(n=0), dict(n=-2), dict(kind=3), dict(kind=-1), dict(conn=6),
                dict(conn=0), dict(shape=2), dict(shape=-1), dict(open=5), dict(open=-1), dict(close=5), dict(close=-1), dict(fill=4097),
                dict(fill=-1),
                dict(kind=0, hyst=1, strong=1.0), dict(hyst=1, strong=float("inf")), dict(hyst=1, strong=float("nan")),
                dict(hyst=1, strong=0.4), dict(hyst=1, strong=float("-inf")),
                dict(kind=0, gated=p), dict(gated=p, thresh=0.0), dict(gated=p, thresh=-0.5),
                dict(src=p + 2), dict(counts=p + 2), dict(gated=p + 1), dict(kind=1, src=p + 1)):
        assert call(**bad) == _lib.ERR_BADARG, bad
    for bad in (dict(h=65), dict(w=65), dict(h=0), dict(w=0), dict(w=-1), dict(h=65, w=4096)):
        assert call(**bad) == _lib.ERR_UNSUPPORTED, bad
    assert call(h=65, conn=6) == _lib.ERR_BADARG                      # a bad argument is reported before an unsupported size
