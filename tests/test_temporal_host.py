"""Host side of -process --source-video --smooth (cgs_amd.temporal) and the properties of its checker tests/temporal_ref.py.  No GPU: the
kernel itself is checked in tests/test_gpu_temporal.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import temporal_ref  # noqa: E402
from cgs_amd import _lib, build, temporal  # noqa: E402


def _flat(n, colour=90):
    return np.full((n, 64, 64, 3), colour, dtype=np.uint8)


# ---------------------------------------------------------------- the checker against hand-worked cases
def test_tap_order():
    assert temporal_ref.taps(1)[:3] == [(-1, -1, -1), (-1, -1, 0), (-1, -1, 1)] and temporal_ref.taps(1)[9] == (1, -1, -1)
    assert len(temporal_ref.taps(8)) == 16 * 9 and all(k != 0 for k, _, _ in temporal_ref.taps(8))
    assert [k for k, _, _ in temporal_ref.taps(2)][::9] == [-2, -1, 1, 2]


def test_ref_of_a_constant_stack_is_that_constant():
    rs = np.random.RandomState(0)
    low = rs.randint(0, 256, (5, 64, 64, 3)).astype(np.uint8)
    for value in (0.0, 0.37, 1.0):
        out = temporal_ref.smooth_ref(np.full((5, 64, 64), value, dtype=np.float32), low, 3, 16.0)
        assert out.shape == (5, 64, 64) and np.abs(out - np.float32(value)).max() < 1e-15


def test_ref_of_one_frame_is_the_frame():
    z = np.random.RandomState(1).rand(1, 64, 64).astype(np.float32)
    np.testing.assert_array_equal(temporal_ref.smooth_ref(z, _flat(1), 8, 16.0), z.astype(np.float64))


def test_ref_on_a_flat_guide_is_the_separable_gaussian():
    """Constant colour, one bright cell in the middle frame, radius 2 (sigma_t = 1): a cell of another frame sees it through the time and
    space Gaussians alone; the frame itself keeps only its centre tap."""
    z = np.zeros((5, 64, 64), dtype=np.float32)
    z[2, 30, 30] = 1.0
    out = temporal_ref.smooth_ref(z, _flat(5), 2, 16.0)
    wt = {1: np.exp(-0.5), 2: np.exp(-2.0)}
    ws = np.exp(-0.5)
    den_mid = 1 + 2 * (wt[1] + wt[2]) * (1 + 4 * ws + 4 * ws * ws)       # a middle frame: four neighbours, nine cells each
    assert abs(out[2, 30, 30] - 1.0 / den_mid) < 1e-15
    assert out[2, 30, 31] == 0.0                                          # the same frame: only the centre tap
    den1 = 1 + (2 * wt[1] + wt[2]) * (1 + 4 * ws + 4 * ws * ws)          # frame 1 has the frames 0, 2, 3
    assert abs(out[1, 30, 30] - wt[1] / den1) < 1e-15
    assert abs(out[1, 31, 31] - wt[1] * ws * ws / den1) < 1e-15
    assert out[1, 30, 32] == 0.0 and out[1, 32, 30] == 0.0                # outside the 3 x 3 search
    den0 = 1 + (wt[1] + wt[2]) * (1 + 4 * ws + 4 * ws * ws)              # frame 0 has the frames 1 and 2: missing frames are skipped
    assert abs(out[0, 30, 29] - wt[2] * ws / den0) < 1e-15


def test_ref_skips_cells_outside_the_grid():
    z = np.zeros((2, 64, 64), dtype=np.float32)
    z[1, 0, 0] = 1.0
    out = temporal_ref.smooth_ref(z, _flat(2), 1, 16.0)
    wt, ws = np.exp(-2.0), np.exp(-0.5)
    assert abs(out[0, 0, 0] - wt / (1 + wt * (1 + 2 * ws + ws * ws))) < 1e-15      # four cells in reach, not nine
    assert abs(out[0, 0, 1] - wt * ws / (1 + wt * (1 + 3 * ws + 2 * ws * ws))) < 1e-15


def test_ref_range_term_uses_the_centre_frames_colour():
    """Two cells of one colour distance apart: d2 = 3 x 10^2 = 300 against sigma_r = 10 is exp(-1.5)."""
    low = _flat(2, 100)
    low[1] = 110
    z = np.zeros((2, 64, 64), dtype=np.float32)
    z[1] = 1.0
    out = temporal_ref.smooth_ref(z, low, 1, 10.0)
    w = np.exp(-2.0) * np.exp(-1.5) * (1 + 4 * np.exp(-0.5) + 4 * np.exp(-1.0))
    assert abs(out[0, 30, 30] - w / (1 + w)) < 1e-15


def test_ref_sub_range():
    rs = np.random.RandomState(2)
    z, low = rs.rand(7, 64, 64).astype(np.float32), rs.randint(0, 256, (7, 64, 64, 3)).astype(np.uint8)
    full = temporal_ref.smooth_ref(z, low, 2, 16.0)
    np.testing.assert_array_equal(temporal_ref.smooth_ref(z, low, 2, 16.0, 2, 5), full[2:5])
    np.testing.assert_array_equal(temporal_ref.smooth_ref(z[1:7], low[1:7], 2, 16.0, 2, 4), full[3:5])      # a window with its halo


def test_emulation_tracks_the_reference():
    rs = np.random.RandomState(3)
    z, low = rs.rand(4, 64, 64).astype(np.float32), rs.randint(100, 120, (4, 64, 64, 3)).astype(np.uint8)
    e = temporal_ref.smooth_emul32(z, low, 2, 16.0)
    assert e.dtype == np.float32 and np.abs(e.astype(np.float64) - temporal_ref.smooth_ref(z, low, 2, 16.0)).max() < 2e-6


# ---------------------------------------------------------------- host helpers and registration
def test_radius_and_sigma_t():
    assert temporal.check_radius(1) == 1 and temporal.check_radius(np.int64(8)) == 8 and temporal.check_radius(0, least=0) == 0
    for bad in (0, 9, -1, 2.0, True, "3"):
        with pytest.raises(ValueError):
            temporal.check_radius(bad)
    assert temporal.sigma_t(3) == 1.5 and temporal.sigma_t(8) == 4.0


def test_registered_in_build_and_signature_table():
    assert "temporal.hip" in build.SOURCES
    assert "cgs_temporal_smooth" in _lib.SIGNATURES and len(_lib.SIGNATURES["cgs_temporal_smooth"][1]) == 9
    assert (temporal.SIDE, temporal.MAX_RADIUS) == (64, 8)
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        header = fp.read()
    assert "int cgs_temporal_smooth(const float* z, const uint8_t* low, int32_t n, int32_t f0, int32_t f1, int32_t radius, float sigma_r" in header
    assert "CGS_TEMPORAL_MAX_RADIUS = 8" in header


def test_the_documents_name_the_entry():
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(REPO, doc)) as fp:
            assert "cgs_temporal_smooth" in fp.read(), doc


# ---------------------------------------------------------------- argument errors come before the library is touched
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_smooth_argument_errors(no_library):
    z, low = torch.zeros((4, 64, 64)), torch.zeros((4, 64, 64, 3), dtype=torch.uint8)
    cases = [(dict(z=z.double()), "z"), (dict(z=z[:, :32]), "z"), (dict(z=z.numpy()), "torch"), (dict(low=low[:3]), "low"),
             (dict(low=low.float()), "low"), (dict(radius=0), "radius"), (dict(radius=9), "radius"), (dict(radius=1.5), "radius"),
             (dict(sigma_r=0.0), "sigma_r"), (dict(sigma_r=float("nan")), "sigma_r"), (dict(f0=2, f1=2), "range"),
             (dict(f1=5), "range"), (dict(f0=-1), "range")]
    for kw, word in cases:
        args = dict(z=z, low=low, radius=2)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            temporal.smooth(**args)
        assert word in str(e.value), (kw, str(e.value))


def test_no_cpu_path():
    with pytest.raises(_lib.CgsError):
        temporal.smooth(torch.zeros((2, 64, 64)), torch.zeros((2, 64, 64, 3), dtype=torch.uint8), 1)
