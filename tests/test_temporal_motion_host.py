"""Host side of -process --source-video --smooth R --smooth-motion S (cgs_amd.temporal, cgs_amd.cli) and the properties of its checker
tests/temporal_motion_ref.py.  No GPU: the kernels themselves are checked in tests/test_gpu_temporal_motion.py, whose tolerance is
derived here on that file's own inputs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import temporal_motion_ref as ref  # noqa: E402
import temporal_ref  # noqa: E402
import test_gpu_temporal_motion as gpu  # noqa: E402
from cgs_amd import _lib, build, cli, temporal  # noqa: E402


# ---------------------------------------------------------------- the checkers against each other and against hand-worked cases
def test_zero_fields_give_the_plain_reference_exactly():
    z, low = gpu.drifting(6)
    zero = np.zeros((5, 8, 8, 2), dtype=np.int8)
    for radius, sigma_r in ((1, 16.0), (3, 4.0), (8, 64.0)):
        np.testing.assert_array_equal(ref.smooth_mc_ref(z, low, zero, zero, radius, sigma_r), temporal_ref.smooth_ref(z, low, radius, sigma_r))
    np.testing.assert_array_equal(ref.smooth_mc_ref(z, low, zero, zero, 2, 16.0, 1, 4), temporal_ref.smooth_ref(z, low, 2, 16.0, 1, 4))
    np.testing.assert_array_equal(ref.smooth_mc_ref(z[:1], low[:1], None, None, 8, 16.0), z[:1].astype(np.float64))


@pytest.mark.parametrize("dy, dx, valid", [(0, 3, 56), (2, -3, 49), (-4, 4, 49), (1, 0, 56)])
def test_flow_ref_finds_a_translation(dy, dx, valid):
    """A noise-free random texture moved by (dy, dx): every block whose true candidate is valid gets exactly that vector, forward, and
    its negation backward."""
    _, low, _ = ref.pan(3, dy, dx, seed=4, noise=0, texture=True)
    fwd, bwd = ref.flow_ref(low, 4)
    ok_f = np.array([[0 <= by * 8 + dy <= 56 and 0 <= bx * 8 + dx <= 56 for bx in range(8)] for by in range(8)])
    ok_b = np.array([[0 <= by * 8 - dy <= 56 and 0 <= bx * 8 - dx <= 56 for bx in range(8)] for by in range(8)])
    assert ok_f.sum() == valid and ok_b.sum() == valid
    for g in range(2):
        assert (fwd[g][ok_f] == (dy, dx)).all() and (bwd[g][ok_b] == (-dy, -dx)).all()
        assert not (fwd[g][~ok_f] == (dy, dx)).all(axis=-1).any()      # out of reach there: some other candidate


def test_flow_ref_on_constant_frames_is_zero():
    low = np.full((3, 64, 64, 3), 200, dtype=np.uint8)
    fwd, bwd = ref.flow_ref(low, 4)
    assert fwd.shape == (2, 8, 8, 2) and fwd.dtype == np.int8 and not fwd.any() and not bwd.any()


def test_candidate_order_and_ties_by_hand():
    c = ref.candidates(1)
    assert c == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
    assert len(ref.candidates(4)) == 81 and ref.candidates(4)[:5] == c[:5] and ref.candidates(4)[-1] == (4, 4)
    assert [d for d in ref.candidates(4) if max(abs(d[0]), abs(d[1])) <= 2] == ref.candidates(2)      # a smaller S: the same order
    # Two blocks by hand, S = 1.  Frame 0 is black but for block (0, 0) = 10 and block (3, 3) = 10; frame 1 is black everywhere.
    # Block (0, 0): every valid candidate -- (0, 0), (0, 1), (1, 0), (1, 1) -- has SAD 64 * 30: the tie goes to (0, 0).
    low = np.zeros((2, 64, 64, 3), dtype=np.uint8)
    low[0, 0:8, 0:8] = 10
    low[0, 24:32, 24:32] = 10
    # Frame 1 carries block (3, 3) one cell up and, as well, one cell to the left: SAD 0 at (-1, 0) and at (0, -1); (-1, 0) ranks first.
    low[1, 23:31, 24:32] = 10
    low[1, 24:32, 23:31] = 10
    fwd, bwd = ref.flow_ref(low, 1)
    assert tuple(fwd[0, 0, 0]) == (0, 0)
    assert tuple(fwd[0, 3, 3]) == (-1, 0)
    # with the upward copy spoilt by one grey level in one cell, (0, -1) is strictly smaller and wins although it ranks later
    low[1, 23, 24, 0] = 11
    assert tuple(ref.flow_ref(low, 1)[0][0, 3, 3]) == (0, -1)
    # backward, from the black block (0, 0) of frame 1: (1, 1) leaves the fewest cells of frame 0's bright block under it, 49 x 30
    assert tuple(bwd[0, 0, 0]) == (1, 1)


def test_paths_clamp_the_lookup_not_the_tap():
    """Every forward vector (0, 40) is no legal field but shows the rule: after one step a cell of column 30 stands at column 70, the
    second step reads the block of column 63 and the path goes on to 110; no tap of frames 1 and 2 lies inside the grid."""
    fwd = np.zeros((2, 8, 8, 2), dtype=np.int8)
    fwd[..., 1] = 40
    my, mx = ref.path(fwd, fwd, 0, 2)
    assert (my == 0).all() and (mx == 80).all()
    fwd[1, :, 7, 1] = -50                                              # the block the clamped cell (row, 63) lies in
    my, mx = ref.path(fwd, fwd, 0, 2)
    assert (mx[:, 16:] == -10).all() and (mx[:, :16] == 80).all()      # from column 16 on a cell stands in or beyond block 7 after one step
    z = np.random.RandomState(0).rand(3, 64, 64).astype(np.float32)
    low = np.full((3, 64, 64, 3), 90, dtype=np.uint8)
    far = np.full((2, 8, 8, 2), 100, dtype=np.int8)
    np.testing.assert_array_equal(ref.smooth_mc_ref(z, low, far, far, 2, 16.0), z.astype(np.float64))


def test_emulation_tracks_the_reference():
    z, low, _ = ref.pan(4, 1, 2, seed=3, flicker=0.1)
    fwd, bwd = ref.flow_ref(low, 3)
    e = ref.smooth_mc_emul32(z, low, fwd, bwd, 2, 16.0)
    assert e.dtype == np.float32 and np.abs(e.astype(np.float64) - ref.smooth_mc_ref(z, low, fwd, bwd, 2, 16.0)).max() < 2e-6


def test_tolerance_is_derived_from_the_emulation():
    """The fp32 emulation against float64 on the inputs of the GPU tests; EMUL_ERR_MC is the largest of these figures, rounded up: 8.92e-7
    (scene diag, radius 8, sigma_r 64); the smallest of a stack with a neighbour frame is 2.3e-7 (two frames), the single frame gives 0."""
    worst = 0.0
    for sc, fl, n, radius, sigma_r in gpu.CASES:
        z, low, _ = gpu.scene(sc, n)
        emul = ref.smooth_mc_emul32(z, low, *gpu.field(fl, n), radius, sigma_r)
        err = float(np.abs(emul.astype(np.float64) - gpu.want(sc, fl, n, radius, sigma_r)).max())
        print(f"emulation scene {sc} field {fl} n {n} radius {radius} sigma_r {sigma_r}: max |fp32 - float64| = {err:.3e}")
        worst = max(worst, err)
    assert worst <= gpu.EMUL_ERR_MC and gpu.EMUL_ERR_MC <= 1.25 * worst          # the constant is the measurement, rounded up
    assert gpu.TOL == 30 * gpu.EMUL_ERR_MC and gpu.TOL < 0.25 / 255


def test_the_ordering_of_the_flicker_test_holds_in_float64():
    """What tests/test_gpu_temporal_motion.py asserts on the GPU, first with the two float64 references: under a pan of 3 cells a frame
    the filter along the motion is closer to the flicker-free mask than the plain filter, and that closer than no filter."""
    with_motion, without, unsmoothed = gpu.flicker_figures(
        lambda z, low: temporal_ref.smooth_ref(z, low, 3, 16.0), lambda z, low: ref.smooth_mc_ref(z, low, *gpu.field("x3"), 3, 16.0))
    print(f"mean |out - clean|: {with_motion:.4f} along the motion, {without:.4f} without, {unsmoothed:.4f} unsmoothed")
    assert with_motion < without < unsmoothed
    assert abs(unsmoothed - 0.15) < 1e-6                               # the flicker itself; nothing was clipped


# ---------------------------------------------------------------- host helpers, flags and registration
def test_check_search():
    assert temporal.check_search(1) == 1 and temporal.check_search(np.int64(4)) == 4 and temporal.check_search(0, least=0) == 0
    for bad in (0, 5, -1, 2.0, True, "3"):
        with pytest.raises(ValueError):
            temporal.check_search(bad)
    with pytest.raises(ValueError, match="--smooth-motion"):
        temporal.check_search(5, least=0, name="--smooth-motion")
    assert (temporal.BLOCK, temporal.MAX_SEARCH) == (8, 4) == (_lib.TEMPORAL_BLOCK, _lib.TEMPORAL_MAX_SEARCH)


def test_flag_checks():
    video = ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4"]
    a = cli.parse_args(video)
    assert a.smooth == 0 and a.smooth_motion == 0
    a = cli.parse_args(video + ["--smooth", "3"])
    assert a.smooth == 3 and a.smooth_motion == 0
    a = cli.parse_args(video + ["--smooth", "3", "--smooth-motion", "4"])
    assert a.smooth == 3 and a.smooth_motion == 4
    assert cli.parse_args(video + ["--smooth", "3", "--smooth-motion", "0"]).smooth_motion == 0
    assert cli.parse_args(video + ["--smooth-motion", "0"]).smooth_motion == 0
    with pytest.raises(ValueError, match="--source-video"):
        cli.parse_args(["-process", "--smooth-motion", "2"])
    with pytest.raises(ValueError, match="give --smooth R"):
        cli.parse_args(video + ["--smooth-motion", "2"])
    with pytest.raises(ValueError, match="give --smooth R"):
        cli.parse_args(video + ["--smooth", "0", "--smooth-motion", "2"])
    with pytest.raises(ValueError, match="--smooth-motion = 5"):
        cli.parse_args(video + ["--smooth", "2", "--smooth-motion", "5"])
    with pytest.raises(ValueError, match="--smooth-motion = -1"):
        cli.parse_args(video + ["--smooth", "2", "--smooth-motion", "-1"])
    assert cli.parse_args([]).smooth_motion is None                      # not a video: the flag is left alone, as --smooth is


def test_registered_in_build_and_signature_table():
    assert "temporal_motion.hip" in build.SOURCES and "temporal.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "temporal_motion.hip"))
    assert len(_lib.SIGNATURES["cgs_temporal_flow"][1]) == 6 and len(_lib.SIGNATURES["cgs_temporal_smooth_mc"][1]) == 11
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        header = fp.read()
    assert "int cgs_temporal_flow(const uint8_t* low, int32_t n, int32_t search, int8_t* fwd, int8_t* bwd, cgs_stream_t stream);" in header
    assert "int cgs_temporal_smooth_mc(const float* z, const uint8_t* low, const int8_t* fwd, const int8_t* bwd, int32_t n, int32_t f0" in header
    assert "enum { CGS_TEMPORAL_BLOCK = 8, CGS_TEMPORAL_MAX_SEARCH = 4 };" in header
    assert "enum { CGS_TEMPORAL_SIDE = 64, CGS_TEMPORAL_MAX_RADIUS = 8 };" in header          # the enum that was there is as it was


def test_the_documents_name_the_entries():
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(REPO, doc)) as fp:
            text = fp.read()
        assert "cgs_temporal_flow" in text and "cgs_temporal_smooth_mc" in text and "--smooth-motion" in text, doc


# ---------------------------------------------------------------- argument errors come before the library is touched
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_argument_errors(no_library):
    z, low = torch.zeros((4, 64, 64)), torch.zeros((4, 64, 64, 3), dtype=torch.uint8)
    fwd = torch.zeros((3, 8, 8, 2), dtype=torch.int8)
    for kw, word in [(dict(low=low.float()), "low"), (dict(low=low[:, :32]), "low"), (dict(low=low.numpy()), "torch"), (dict(low=low[:0]), "low"),
                     (dict(search=0), "search"), (dict(search=5), "search"), (dict(search=2.0), "search")]:
        args = dict(low=low, search=2)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            temporal.flow(**args)
        assert word in str(e.value), (kw, str(e.value))
    for motion, word in [((fwd, fwd[:2]), "bwd"), ((fwd.short(), fwd), "fwd"), ((fwd[:, :4], fwd), "fwd"), (fwd, "pair"), ((fwd,), "pair"),
                         ((fwd.numpy(), fwd.numpy()), "pair")]:
        with pytest.raises(ValueError) as e:
            temporal.smooth(z, low, 2, motion=motion)
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="radius"):                      # the checks that were there come first
        temporal.smooth(z, low, 0, motion=(fwd, fwd))


def test_no_cpu_path():
    low = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(_lib.CgsError):
        temporal.flow(low, 2)
    with pytest.raises(_lib.CgsError):
        temporal.smooth(torch.zeros((2, 64, 64)), low, 1, motion=(torch.zeros((1, 8, 8, 2), dtype=torch.int8),) * 2)
