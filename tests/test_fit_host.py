"""Host side of -process -fit (cgs_amd.fit, cli.check_fit_flags) and the properties of its checker tests/fit_ref.py.  No GPU: the
kernels themselves are checked in tests/test_gpu_fit.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import fit_ref  # noqa: E402
from cgs_amd import _lib, build, cli, fit  # noqa: E402

LENGTHS = (64, 65, 127, 128, 1080, 4096)


# ---------------------------------------------------------------- flags
def test_flags_parse_and_defaults():
    a = cli.parse_args([])
    assert a.fit is False and a.fit_spatial is None and a.fit_range is None
    a = cli.parse_args(["-process", "-fit"])
    assert a.fit is True and a.fit_spatial == 1.0 and a.fit_range == 16.0
    a = cli.parse_args(["-process", "-fit", "--fit-spatial", "0.5", "--fit-range", "2"])
    assert (a.fit_spatial, a.fit_range) == (0.5, 2.0)
    a = cli.parse_args(["-process", "-fit", "-crf", "-concatenated", "-objects", "--track-iou", "0.3", "-fp16"])
    assert a.fit and a.crf and a.objects and a.fp16
    a = cli.parse_args(["-process"])                      # without -fit nothing is filled in
    assert a.fit is False and a.fit_spatial is None and a.fit_range is None


@pytest.mark.parametrize("argv, word", [
    (["-process", "--fit-spatial", "1"], "--fit-spatial"),
    (["-process", "--fit-range", "8"], "--fit-range"),
    (["--fit-spatial", "1", "--fit-range", "8"], "--fit-spatial / --fit-range"),
    (["-fit"], "-process"),
    (["-fit", "-eval"], "-process"),
    (["-process", "-fit", "-eval"], "-eval"),
    (["-process", "-fit", "-test"], "-eval"),
    (["-process", "-fit", "-salience"], "-salience"),
    (["-process", "-fit", "-salience", "-process_salience"], "-salience"),
    (["-process", "-fit", "-process_salience"], "-process_salience"),
    (["-process", "-fit", "--fit-spatial", "0.49"], "--fit-spatial"),
    (["-process", "-fit", "--fit-spatial", "0"], "--fit-spatial"),
    (["-process", "-fit", "--fit-spatial", "-1"], "--fit-spatial"),
    (["-process", "-fit", "--fit-spatial", "nan"], "--fit-spatial"),
    (["-process", "-fit", "--fit-spatial", "inf"], "--fit-spatial"),
    (["-process", "-fit", "--fit-range", "0"], "--fit-range"),
    (["-process", "-fit", "--fit-range", "-3"], "--fit-range"),
    (["-process", "-fit", "--fit-range", "nan"], "--fit-range"),
    (["-process", "-fit", "--fit-range", "inf"], "--fit-range"),
    (["-process", "-fit", "-objects", "--binarymaskthreshold", "0"], "--binarymaskthreshold 0"),      # the existing check, as it is
])
def test_flags_refused(argv, word):
    with pytest.raises(ValueError) as e:
        cli.parse_args(argv)
    assert word in str(e.value)


# ---------------------------------------------------------------- host helpers
@pytest.mark.parametrize("L", LENGTHS)
def test_box_weights(L):
    w = fit.box_weights(L)
    assert w.shape == (64, L) and w.dtype == np.int64 and w.min() >= 0 and w.max() <= 64
    np.testing.assert_array_equal(w.sum(axis=1), np.full(64, L))
    np.testing.assert_array_equal(w.sum(axis=0), np.full(L, 64))
    np.testing.assert_array_equal(w, fit_ref.overlap(L))                 # the checker's table comes from counting units, not min / max
    if L == 64:
        np.testing.assert_array_equal(w, 64 * np.eye(64, dtype=np.int64))
    if L % 64 == 0:                                                      # the plain block mean
        np.testing.assert_array_equal(w, 64 * np.repeat(np.eye(64, dtype=np.int64), L // 64, axis=1))


@pytest.mark.parametrize("L", LENGTHS)
def test_home_cells(L):
    q = fit.home_cells(L)
    assert q.shape == (L,) and q.min() == 0 and q.max() == 63
    assert (np.diff(q) >= 0).all() and (np.diff(q) <= 1).all()
    np.testing.assert_array_equal(np.unique(q), np.arange(64))
    np.testing.assert_array_equal(q, fit_ref.home(L))
    centre = (np.arange(L) + 0.5) * 64 / L                               # the pixel's centre in cells
    np.testing.assert_array_equal(q, np.floor(centre).astype(np.int64))
    for cell in (0, 31, 63):                                             # the band arithmetic the kernel uses for its rows
        rows = np.flatnonzero(q == cell)
        assert rows[0] == (cell * L + 31) >> 6 and rows[-1] + 1 == ((cell + 1) * L + 31) >> 6


def test_check_size():
    assert fit.check_size(64, 4096) == (64, 4096) and fit.check_size(np.int64(360), 640) == (360, 640)
    for h, w, word in ((63, 64, "h"), (64, 63, "w"), (4097, 64, "h"), (64, 4097, "w"), (64.0, 64, "h"), (True, 64, "h"), (64, "64", "w")):
        with pytest.raises(ValueError) as e:
            fit.check_size(h, w)
        assert str(e.value).startswith(word)
    for bad in (63, 4097):
        with pytest.raises(ValueError):
            fit.box_weights(bad)
        with pytest.raises(ValueError):
            fit.home_cells(bad)


# ---------------------------------------------------------------- the checker's own properties
def test_down_ref_of_replicated_frames_and_identity():
    rs = np.random.RandomState(0)
    x = rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)
    np.testing.assert_array_equal(fit_ref.down_ref(x), x)
    for ky, kx in ((2, 2), (3, 3), (2, 3)):
        big = np.repeat(np.repeat(x, ky, axis=1), kx, axis=2)
        np.testing.assert_array_equal(fit_ref.down_ref(big), x)
    # rounds half up: a 128 x 64 frame whose row pairs are (0, 1) averages to 0.5 -> 1
    half = np.zeros((1, 128, 64, 3), dtype=np.uint8)
    half[:, 1::2] = 1
    assert (fit_ref.down_ref(half) == 1).all()
    # against the definition itself, with Python integers, on an odd size
    y = rs.randint(0, 256, (1, 65, 67, 3)).astype(np.uint8)
    got = fit_ref.down_ref(y)
    wy, wx = fit.box_weights(65), fit.box_weights(67)
    for oy, ox, c in ((0, 0, 0), (63, 63, 2), (17, 40, 1)):
        S = sum(int(wy[oy, a]) * int(wx[ox, b]) * int(y[0, a, b, c]) for a in range(65) for b in range(67))
        assert got[0, oy, ox, c] == (2 * S + 65 * 67) // (2 * 65 * 67)


def test_up_ref_of_a_constant_map_is_that_constant():
    rs = np.random.RandomState(1)
    guide = rs.randint(0, 256, (1, 65, 67, 3)).astype(np.uint8)
    low = fit_ref.down_ref(guide)
    for value in (0.0, 0.37, 1.0):
        out = fit_ref.up_ref(np.full((1, 64, 64), value, dtype=np.float32), guide, low, 1.0, 16.0)
        assert out.shape == (1, 65, 67) and np.abs(out - np.float32(value)).max() < 1e-15
    ones = fit_ref.up_ref(np.ones((1, 64, 64), dtype=np.uint8) * 7, guide, low, 0.5, 2.0)        # labels: non-zero = 1
    assert np.abs(ones - 1.0).max() < 1e-15


def test_up_ref_at_the_grid_centre_with_a_flat_guide_is_the_gaussian():
    """64 x 64 'upsampling' with a constant guide: every pixel sits on its cell's centre and the weights are the plain 5 x 5 Gaussian."""
    guide = np.full((1, 64, 64, 3), 90, dtype=np.uint8)
    m = np.zeros((1, 64, 64), dtype=np.float32)
    m[0, 30, 30] = 1.0
    out = fit_ref.up_ref(m, guide, guide, 1.0, 16.0)[0]
    g = np.exp(-np.arange(-2, 3) ** 2 / 2.0)
    np.testing.assert_allclose(out[28:33, 28:33], np.outer(g, g) / g.sum() ** 2, rtol=1e-13)
    assert out[27, 30] == 0.0 and out[30, 33] == 0.0
    top = np.zeros((1, 64, 64), dtype=np.float32)
    top[0, 0] = 1.0                                                      # taps off the grid are skipped: rows 0, 1, 2 share the weight
    np.testing.assert_allclose(fit_ref.up_ref(top, guide, guide, 1.0, 16.0)[0, 0, 5], g[2] / g[2:].sum(), rtol=1e-13)


# ---------------------------------------------------------------- registration
def test_registered_in_build_and_signature_table():
    assert "fit.hip" in build.SOURCES
    assert "cgs_fit_down_u8" in _lib.SIGNATURES and "cgs_fit_up_joint" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_fit_down_u8"][1]) == 6 and len(_lib.SIGNATURES["cgs_fit_up_joint"][1]) == 15
    assert (fit.SIDE, fit.MAX_SIDE, fit.RADIUS) == (64, 4096, 2)


# ---------------------------------------------------------------- argument errors come before the library is touched
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_down_argument_errors(no_library):
    for bad, word in ((np.zeros((1, 64, 64, 3), np.uint8), "torch tensor"), (torch.zeros((1, 64, 64, 3)), "uint8"),
                      (torch.zeros((64, 64, 3), dtype=torch.uint8), "[n,H,W,3]"), (torch.zeros((1, 64, 64, 4), dtype=torch.uint8), "[n,H,W,3]"),
                      (torch.zeros((0, 64, 64, 3), dtype=torch.uint8), "at least one"), (torch.zeros((1, 63, 64, 3), dtype=torch.uint8), "h = 63"),
                      (torch.zeros((1, 64, 4097, 3), dtype=torch.uint8), "w = 4097")):
        with pytest.raises(ValueError) as e:
            fit.down(bad)
        assert "frames_u8" in str(e.value) and word in str(e.value)


def test_up_argument_errors(no_library):
    guide = torch.zeros((2, 65, 67, 3), dtype=torch.uint8)
    vals = torch.zeros((2, 64, 64), dtype=torch.float32)
    low = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    cases = [
        (dict(values=vals.double()), "values"), (dict(values=vals[:1]), "values"), (dict(values=vals[:, :32]), "values"),
        (dict(values=vals.numpy()), "values"), (dict(guide=guide.float()), "guide"), (dict(guide=guide[0]), "guide"),
        (dict(guide=guide[:, :63]), "guide"), (dict(low=low[:1]), "low"), (dict(low=low.float()), "low"),
        (dict(sigma_s=0.49), "sigma_s"), (dict(sigma_s=float("nan")), "sigma_s"), (dict(sigma_s="wide"), "sigma_s"),
        (dict(sigma_r=0.0), "sigma_r"), (dict(sigma_r=-1.0), "sigma_r"), (dict(sigma_r=float("inf")), "sigma_r"),
        (dict(want=("hard",)), "thresh"), (dict(want=("soft", "hard")), "thresh"), (dict(want=("hard",), thresh=float("nan")), "thresh"),
        (dict(want=()), "want"), (dict(want=("mask",)), "want"),
    ]
    for kw, word in cases:
        args = dict(values=vals, guide=guide, low=low)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            fit.up(**args)
        assert word in str(e.value), (kw, str(e.value))


def test_no_cpu_path():
    """Host tensors are refused with CgsError, with or without a GPU in the machine."""
    with pytest.raises(_lib.CgsError):
        fit.down(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
    with pytest.raises(_lib.CgsError):
        fit.up(torch.zeros((1, 64, 64)), torch.zeros((1, 64, 64, 3), dtype=torch.uint8), torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
