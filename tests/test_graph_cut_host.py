"""The host side of --graph-cut without a GPU: graphcut.parse_spec / spec_band / tables / cut_report, cli.check_cut_flags' refusals and
defaults, and tests/graph_cut_ref.py (the rule of cgs_graph_cut in Python integers with scipy's max flow) on frames small enough to
work out by hand."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_cut_ref as ref  # noqa: E402
from cgs_amd import _lib, cli, graphcut  # noqa: E402


# ---------------------------------------------------------------- the spec
def test_parse_spec_defaults_and_values():
    assert graphcut.parse_spec("") == {"lo": None, "hi": None, "lambda": 50, "it": 3, "bins": 8, "conn": 8}
    assert graphcut.parse_spec("lo=0.1;hi=0.9;lambda=50;it=3;bins=8;conn=8") == {"lo": 0.1, "hi": 0.9, "lambda": 50, "it": 3, "bins": 8, "conn": 8}
    spec = graphcut.parse_spec(" conn=4 ; bins=4;it=8;lambda=0 ")
    assert spec == {"lo": None, "hi": None, "lambda": 0, "it": 8, "bins": 4, "conn": 4}
    assert graphcut.spec_text(spec) == "lambda=0;it=8;bins=4;conn=4"
    assert graphcut.parse_spec(graphcut.spec_text(spec)) == spec
    assert graphcut.spec_kwargs(spec) == dict(lo=None, hi=None, lam=0, iters=8, bins=4, connectivity=4)
    assert graphcut.default_band(0.5) == (0.25, 0.75) and graphcut.default_band(0.05) == (0.025, 0.525)
    assert graphcut.spec_band(spec, 0.5) == (0.25, 0.75)
    assert graphcut.spec_band(graphcut.parse_spec("lo=0.5;hi=0.5"), 0.5) == (0.5, 0.5)          # equality is allowed on both sides


@pytest.mark.parametrize("text", ["lo", "lo=", "=3", "lo=0.1;;hi=0.9", "weight=3", "lo=0.1;lo=0.2", "lo=x", "lo=nan", "hi=inf",
                                  "lambda=101", "lambda=-1", "lambda=2.5", "it=0", "it=9", "bins=6", "bins=16", "conn=6", "conn=x",
                                  "lo=0.9;hi=0.1", ";"])
def test_parse_spec_refuses(text):
    with pytest.raises(ValueError, match="--graph-cut"):
        graphcut.parse_spec(text)


def test_spec_band_refuses_a_band_that_misses_the_threshold():
    for text, thr in (("lo=0.6", 0.5), ("hi=0.4", 0.5), ("lo=0.1;hi=0.2", 0.5), ("", float("nan"))):
        with pytest.raises(ValueError):
            graphcut.spec_band(graphcut.parse_spec(text), thr)


# ---------------------------------------------------------------- the command line
def _args(*argv):
    return cli.parse_args(["--model", "m", *argv])


def test_cli_parses_and_fills_in():
    a = _args("-process", "--graph-cut", "lambda=30;it=2")
    assert a.graph_cut == {"lo": None, "hi": None, "lambda": 30, "it": 2, "bins": 8, "conn": 8}
    assert _args("-eval", "--graph-cut", "").graph_cut == graphcut.parse_spec("")
    assert _args("-process").graph_cut is None and _args("-eval").graph_cut is None
    assert _args("-test", "--graph-cut", "conn=4").graph_cut["conn"] == 4                      # (-test switches -eval on and -crf off)
    assert _args("-process", "-grabcut").graph_cut is None and _args("-process", "-grabcut").grabcut is True     # the reference's no-op stays one
    a = _args("-process", "-objects", "--clean", "open=1", "--graph-cut", "", "-fit")
    assert a.graph_cut is not None and a.clean["open"] == 1


@pytest.mark.parametrize("argv, match", [
    (["--graph-cut", ""], "-process or -eval"),
    (["-train", "--graph-cut", ""], "-process or -eval"),
    (["-process", "--source-video", "a.mp4", "--overlay-video", "b.mp4", "--graph-cut", ""], "--source-video"),
    (["-process", "-crf", "--graph-cut", ""], "-crf"),
    (["-eval", "-crf", "--graph-cut", ""], "-crf"),
    (["-process", "--graph-cut", "lambda=500"], "lambda"),
    (["-process", "--graph-cut", "speed=3"], "KEY=value"),
    (["-eval", "--graph-cut", "it=0"], "it is"),
    (["-process", "--graph-cut", "lo=0.6"], "lo <= thresh <= hi"),                          # --binarymaskthreshold 0.5
    (["-process", "--binarymaskthreshold", "0.95", "--graph-cut", "hi=0.9"], "--binarymaskthreshold"),
    (["-eval", "--graph-cut", "lo=0.1"], "--eval-thresh"),                                    # --eval-thresh 0.05
    (["-eval", "--eval-thresh", "0.5", "--graph-cut", "hi=0.4"], "lo <= thresh <= hi"),
    (["-process", "--clean", "hyst=0.8", "--graph-cut", ""], "hyst"),
])
def test_cli_refuses(argv, match):
    with pytest.raises(ValueError, match=match):
        _args(*argv)


# ---------------------------------------------------------------- the tables and the report
def test_tables():
    for lam in (0, 1, 50, 100):
        WA, WD, L = graphcut.tables(lam)
        assert WA.dtype == WD.dtype == L.dtype == np.int32
        assert WA.shape == WD.shape == (1024,) and L.shape == (4096 + 512 + 1,)
        assert WA[0] == 16 * lam and L[1] == 0 and L[0] == 0
        assert (np.diff(WA) <= 0).all() and (np.diff(WD) <= 0).all() and (np.diff(L[1:]) >= 0).all()
        assert (WD <= WA).all() and (WA >= 0).all() and (WD >= 0).all()
        assert 4 * int(WA[0]) + 4 * int(WD[0]) < 8 * int(WA[0]) + 1 and 4096 * (8 * int(WA[0]) + 1) < 2 ** 31
        assert 2 * int(WA[0]) < 2 ** 16                                     # the 16-bit residuals of the kernel
    WA, WD, L = graphcut.tables(50)
    assert WA[128] == round(800 * np.exp(-1.0)) and WD[0] == round(800 / np.sqrt(2.0)) and L[4608] == round(16 * np.log(4608.0))
    assert WA[1023] == 0                                                    # a strong edge carries nothing at the default lambda
    for bad in (-1, 101, 2.0, True, None):
        with pytest.raises(ValueError):
            graphcut.tables(bad)
    assert (_lib.CUT_TABLE, _lib.CUT_LOG_TABLE, _lib.CUT_SCALE) == (1024, 4609, 16)


def test_cut_report():
    spec = graphcut.parse_spec("it=2")
    stats = np.array([[0, 2, 5, 100, 10, 12, 30, 4], [graphcut.EARLY, 1, 9, 50, 3, 3, 7, 0], [graphcut.EMPTY, 0, 0, 0, 0, 0, 2, 0],
                      [graphcut.NOT_CONVERGED | graphcut.EARLY, 1, 64, 7, 1, 1, 1, 0]], dtype=np.int32)
    want = {"spec": spec, "frames": 4, "empty": 1, "early": 2, "not_converged": 1, "iterations": 4, "energy": 157, "seed_on": 14, "on": 16,
            "unknown": 40, "changed": 4, "rounds": 64}
    assert graphcut.cut_report(stats, spec) == want == graphcut.cut_report(torch.from_numpy(stats), spec)
    assert graphcut.cut_report(stats[0], spec)["frames"] == 1
    assert graphcut.STATS == ("status", "iterations", "rounds", "energy", "seed_on", "on", "unknown", "changed")


def test_cut_checks_its_arguments_before_the_gpu():
    f, z = torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.float32)
    for bad in (dict(lo=0.6), dict(hi=0.4), dict(lam=101), dict(iters=0), dict(bins=16), dict(connectivity=6), dict(max_rounds=0),
                dict(sweeps=8)):
        with pytest.raises(ValueError):
            graphcut.cut(f, z, 0.5, **bad)
    with pytest.raises(ValueError):
        graphcut.cut(f.numpy(), z, 0.5)
    with pytest.raises(ValueError):
        graphcut.cut(f, z, None)
    with pytest.raises(_lib.CgsError, match="no CPU fallback"):           # valid arguments, tensors on the host: no quiet fall-back
        graphcut.cut(f, z, 0.5)


# ---------------------------------------------------------------- the reference on frames worked out by hand
def _two_colour(h=6, w=8, edge=4):
    frame = np.zeros((h, w, 3), dtype=np.uint8)
    frame[:, :edge], frame[:, edge:] = (255, 0, 0), (0, 0, 255)
    return frame


def test_ref_two_colours_cut_on_the_colour_edge():
    """Hard foreground in the first column, hard background in the last, everything between unknown and off: the colour models and the
    nearly empty links across the colour edge (6 of the 82 pairs, so idx = 64 * 130050 // 9515 = 874 and WA[874] = rint(800 exp(-874 / 128))
    = 1 against 800 within a colour) put the cut exactly on it, for both neighbourhoods."""
    frame = _two_colour()
    z = np.full((6, 8), 0.4, dtype=np.float32)
    z[:, 0], z[:, -1] = 1.0, 0.0
    links, m = ref.n_links(frame, 4, *(t.astype(np.int64) for t in graphcut.tables(50)[:2]))
    across = [c for p, q, c in links if (p % 8 < 4) != (q % 8 < 4)]
    within = [c for p, q, c in links if (p % 8 < 4) == (q % 8 < 4)]
    assert m == 6 * 2 * 255 * 255 // (6 * 7 + 5 * 8) and set(across) == {1} and set(within) == {800} and len(across) == 6
    for conn in (4, 8):
        mask, stats = ref.cut_frame(frame, z, 0.5, connectivity=conn)
        np.testing.assert_array_equal(mask, np.repeat((np.arange(8) < 4)[None], 6, axis=0))
        assert stats[ref.STATUS] == ref.EARLY and stats[ref.ITERATIONS] == 2                 # the second cut returns the first one's labelling
        assert stats[ref.SEED_ON] == 6 and stats[ref.ON] == 24 and stats[ref.UNKNOWN] == 36 and stats[ref.CHANGED] == 18
    one = ref.cut_frame(frame, z, 0.5, iters=1)[1]
    assert one[ref.STATUS] == 0 and one[ref.ITERATIONS] == 1 and one[ref.ON] == 24          # stopped by `it`, not early


def test_ref_flat_frame():
    """Every d2 is 0: m = max(1, 0) = 1, every link has the full weight WA[0] / WD[0], and one histogram bin holds everything."""
    frame = np.full((5, 7, 3), 97, dtype=np.uint8)
    links, m = ref.n_links(frame, 8, *(t.astype(np.int64) for t in graphcut.tables(50)[:2]))
    assert m == 1 and {c for _, _, c in links} == {800, 566} and len(links) == 5 * 6 + 4 * 7 + 2 * 4 * 6
    z = np.full((5, 7), 0.4, dtype=np.float32)
    z[2, 3] = 1.0
    mask, stats = ref.cut_frame(frame, z, 0.5)
    # N1 = 1, N0 = 34: cost_fg = L[513] - L[2] = 89, cost_bg = L[546] - L[35] = 44 for each of the 34 unknown cells.  A foreground cell
    # pays its sink link, cost_fg: everything on costs 34 * 89 = 3026; the seed alone costs its 4 axial + 4 diagonal links and every
    # other cell's cost_bg, 5464 + 34 * 44 = 6960, and any set between cuts at least three full links more than it saves
    L = graphcut.tables(50)[2]
    assert (L[513] - L[2], L[546] - L[35]) == (89, 44)
    assert mask.all() and stats[ref.ENERGY] == 34 * 89 and stats[ref.ITERATIONS] == 1 and stats[ref.ON] == 35
    assert stats[ref.STATUS] == ref.EMPTY                                   # the second cut finds no background left to model
    assert ref.cut_frame(frame, z, 0.5, iters=1)[1].tolist() == [0, 1, 0, 34 * 89, 1, 35, 34, 34]


def test_ref_single_cell_and_empty_sides():
    frame = np.array([[[9, 8, 7]]], dtype=np.uint8)
    for z0, on in ((0.9, 1), (0.1, 0), (0.5, 0), (np.nan, 0)):
        mask, stats = ref.cut_frame(frame, np.array([[z0]], dtype=np.float32), 0.5)
        assert mask.shape == (1, 1) and mask[0, 0] == bool(on)
        assert stats.tolist() == [ref.EMPTY, 0, 0, 0, on, on, int(z0 == 0.5), 0]
    assert ref.cut_frame(frame, np.array([[0.5]], dtype=np.float32), 0.5, inclusive=True)[1].tolist() == [ref.EMPTY, 0, 0, 0, 1, 1, 1, 0]
    # no foreground seed in a real frame: the labelling stays all off
    rs = np.random.RandomState(3)
    frame = rs.randint(0, 256, (4, 5, 3)).astype(np.uint8)
    mask, stats = ref.cut_frame(frame, rs.uniform(0.3, 0.45, (4, 5)).astype(np.float32), 0.5)
    assert not mask.any() and stats.tolist() == [ref.EMPTY, 0, 0, 0, 0, 0, 20, 0]


def test_ref_lambda_zero_decides_cell_by_cell():
    """No n-links: every unknown cell goes where its histogram cost is lower (foreground when cost_bg > cost_fg: the source side is
    the largest one, so a tie is foreground too), and the energy is the sum of the lower costs."""
    rs = np.random.RandomState(5)
    frame = rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    z = rs.uniform(0, 1, (9, 11)).astype(np.float32)
    mask, stats = ref.cut_frame(frame, z, 0.5, lam=0, iters=1, bins=4)
    seed, hard_bg, hard_fg = ref.trimap(z, 0.5, False, 0.25, 0.75)
    L = graphcut.tables(0)[2].astype(np.int64)
    bins = ((frame.astype(np.int64) >> 6) * np.array([16, 4, 1])).sum(axis=-1)
    want, energy = np.zeros((9, 11), dtype=bool), 0
    for y in range(9):
        for x in range(11):
            if hard_fg[y, x] or hard_bg[y, x]:
                want[y, x] = hard_fg[y, x]
                continue
            h1, h0 = int((bins[seed] == bins[y, x]).sum()), int((bins[~seed] == bins[y, x]).sum())
            fg, bg = L[seed.sum() + 64] - L[h1 + 1], L[(~seed).sum() + 64] - L[h0 + 1]
            want[y, x] = bg >= fg
            energy += min(fg, bg)
    np.testing.assert_array_equal(mask, want)
    assert stats[ref.ENERGY] == energy and stats[ref.CHANGED] == (want != seed).sum() > 0
    assert 8 * int(graphcut.tables(0)[0][0]) + 1 == 1                      # BIG is 1 here, and the hard cells still hold (no links to pay)
