"""Block-matched motion and the temporal filter along it on the GPU (cgs_temporal_flow, cgs_temporal_smooth_mc, cgs_amd.temporal)
against tests/temporal_motion_ref.py: the vectors bit for bit, the filter with all-zero fields bit for bit against cgs_temporal_smooth,
with estimated and with hand-made fields against float64 within TOL, one case worked by hand, the flicker of a panned scene damped more
with the motion than without, a chunked run against the one-call run bit for bit, and both entries' argument checks.

TOL: an fp32 emulation of the formula in numpy in the kernel's tap order (temporal_motion_ref.smooth_mc_emul32) stays within EMUL_ERR_MC
of float64 over every input that is compared with float64 here (CASES): 2.3e-7 to 8.92e-7 (0 on the single frame), measured on the CPU on
exactly these inputs,
figure by figure, in tests/test_temporal_motion_host.py::test_tolerance_is_derived_from_the_emulation.  Thirty times that -- the margin
tests/test_gpu_temporal.py gives the hardware exponential and the base-2 folding -- is still far below a quarter of a grey level
(9.8e-4).  The largest GPU error seen is printed by every test that compares with float64; on an MI355X it is 8.92e-7 (scene
diag, radius 8, sigma_r 64), and case by case the emulation's own figure to within 8 %."""
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

import temporal_motion_ref as ref  # noqa: E402
from test_gpu_temporal import drifting  # noqa: E402
from cgs_amd import _lib, temporal  # noqa: E402

DEV = "cuda"
EMUL_ERR_MC = 9.0e-7       # the largest |emulation - float64| over CASES, measured on the CPU
TOL = 30 * EMUL_ERR_MC
SETTINGS = tuple((r, s) for r in (1, 3, 8) for s in (4.0, 16.0, 64.0))
SHORT = (1, 2, 5)                                  # stacks shorter than the window of radius 8: both ends clipped at once
PANS = {"x3": (0, 3), "diag": (2, -3)}             # cells a frame
HAND = ("down_right", "up", "random")


@functools.lru_cache(maxsize=None)
def scene(name, n=12):
    """(z, low, clean) of a pan: +-6 colour noise, +-0.15 alternating flicker on z."""
    dy, dx = PANS[name]
    out = ref.pan(n, dy, dx, seed=31 + n + 7 * dy, flicker=0.15)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def field(name, n=12, search=4):
    """flow_ref of the scene, or a hand-made field for the 12 frames of scene x3: every vector (4, 4) -- at radius 8 a path runs 32 cells
    and leaves the grid --, every vector (-4, 0), and random vectors in -4 .. 4."""
    if name in PANS:
        out = ref.flow_ref(scene(name, n)[1], search)
    else:
        rs = np.random.RandomState(17)
        shape = (n - 1, 8, 8, 2)
        one = {"down_right": lambda: np.full(shape, 4), "up": lambda: np.stack((np.full(shape[:3], -4), np.zeros(shape[:3])), axis=-1),
               "random": lambda: rs.randint(-4, 5, shape)}[name]
        out = (one().astype(np.int8), one().astype(np.int8))
    for a in out:
        a.setflags(write=False)
    return out


# every comparison with float64 below: (scene, field, n, radius, sigma_r)
CASES = ([(s, s, 12, r, sr) for s in PANS for r, sr in SETTINGS] + [("x3", "x3", n, 8, 16.0) for n in SHORT] +
         [("x3", h, 12, 8, 16.0) for h in HAND])


@functools.lru_cache(maxsize=None)
def want(sc, fl, n, radius, sigma_r):
    z, low, _ = scene(sc, n)
    out = ref.smooth_mc_ref(z, low, *field(fl, n), radius, sigma_r)
    out.setflags(write=False)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def _flow(low, search=4):
    return tuple(m.cpu().numpy() for m in temporal.flow(_dev(low), search))


def _smooth(z, low, radius, sigma_r=16.0, motion=None, **kw):
    motion = None if motion is None else tuple(_dev(m) for m in motion)
    return temporal.smooth(_dev(z), _dev(low), radius, sigma_r, motion=motion, **kw).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the vectors
def _flow_inputs():
    rs = np.random.RandomState(5)
    yield "pan x3 S4", scene("x3")[1], 4
    yield "pan diag S4", scene("diag")[1], 4
    yield "pan x3 S2 (out of reach)", scene("x3")[1], 2
    yield "pan diag S1 (few candidates at the border)", scene("diag")[1][:5], 1
    yield "noise n 8", rs.randint(0, 256, (8, 64, 64, 3)).astype(np.uint8), 4
    yield "noise n 2", rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8), 3
    yield "constant n 8", np.full((8, 64, 64, 3), 117, dtype=np.uint8), 4
    yield "constant n 2", np.full((2, 64, 64, 3), 0, dtype=np.uint8), 1


@pytest.mark.gpu
def test_flow_bit_for_bit():
    for what, low, search in _flow_inputs():
        fwd, bwd = _flow(low, search)
        wf, wb = ref.flow_ref(low, search)
        assert fwd.shape == (len(low) - 1, 8, 8, 2) and fwd.dtype == np.int8 and bwd.shape == fwd.shape and bwd.dtype == np.int8, what
        np.testing.assert_array_equal(fwd, wf, err_msg=what + " fwd")
        np.testing.assert_array_equal(bwd, wb, err_msg=what + " bwd")
        assert np.abs(fwd).max() <= search and np.abs(bwd).max() <= search
        if what.startswith("constant"):
            assert not fwd.any() and not bwd.any()
    # what the scenes are for: the pan is found where it is in reach, and saturates where it is not
    fwd, bwd = _flow(scene("x3")[1], 4)
    assert (fwd[:, :, :7] == (0, 3)).all(axis=-1).mean() > 0.5 and (bwd[:, :, 1:] == (0, -3)).all(axis=-1).mean() > 0.5
    fwd2, _ = _flow(scene("x3")[1], 2)
    assert (np.abs(fwd2).max(axis=-1) == 2).mean() > 0.3
    # one frame: no pair, no launch
    f1, b1 = temporal.flow(_dev(scene("x3")[1][:1]), 4)
    assert tuple(f1.shape) == (0, 8, 8, 2) and tuple(b1.shape) == (0, 8, 8, 2) and f1.dtype == torch.int8 and f1.is_cuda


# ---------------------------------------------------------------------------------------------------------------- the filter
@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 3, 8])
def test_zero_field_is_the_plain_filter_bit_for_bit(radius):
    z, low = drifting(12)
    zd, ld = _dev(z), _dev(low)
    zero = torch.zeros((11, 8, 8, 2), dtype=torch.int8, device=DEV)
    for sigma_r in (4.0, 16.0, 64.0):
        plain = temporal.smooth(zd, ld, radius, sigma_r)
        assert torch.equal(temporal.smooth(zd, ld, radius, sigma_r, motion=(zero, zero)), plain)
    assert torch.equal(temporal.smooth(zd, ld, radius, f0=3, f1=9, motion=(zero, zero)), temporal.smooth(zd, ld, radius)[3:9])
    assert not torch.equal(temporal.smooth(zd, ld, radius, motion=temporal.flow(ld, 4)), temporal.smooth(zd, ld, radius))


@pytest.mark.gpu
@pytest.mark.parametrize("sc, n, radius, sigma_r", [c[:1] + c[2:] for c in CASES if c[1] in PANS])
def test_against_float64(sc, n, radius, sigma_r):
    z, low, _ = scene(sc, n)
    zd, ld = _dev(z), _dev(low)
    motion = temporal.flow(ld, 4)
    for got, ours in zip(motion, field(sc, n)):
        np.testing.assert_array_equal(got.cpu().numpy(), ours)
    out = temporal.smooth(zd, ld, radius, sigma_r, motion=motion).cpu().numpy()
    assert out.shape == (n, 64, 64) and out.dtype == np.float32
    assert not np.isnan(out).any() and out.min() >= 0.0 and out.max() <= 1.0
    err = float(np.abs(out.astype(np.float64) - want(sc, sc, n, radius, sigma_r)).max())
    print(f"temporal.smooth motion {sc} n {n} radius {radius} sigma_r {sigma_r}: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL
    if n > 1:
        assert np.abs(out - z).max() > 100 * TOL                       # the filter did something
    ones = temporal.smooth(torch.ones_like(zd), ld, radius, sigma_r, motion=motion)
    assert bool((ones == 1.0).all())                                   # ones in, ones out exactly


@pytest.mark.gpu
@pytest.mark.parametrize("name", HAND)
def test_hand_made_fields(name):
    z, low, _ = scene("x3")
    out = _smooth(z, low, 8, 16.0, motion=field(name))
    assert not np.isnan(out).any() and out.min() >= 0.0 and out.max() <= 1.0
    err = float(np.abs(out.astype(np.float64) - want("x3", name, 12, 8, 16.0)).max())
    print(f"temporal.smooth field {name}: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL
    assert np.abs(out - _smooth(z, low, 8, 16.0)).max() > 100 * TOL    # the field moved the taps
    assert (_smooth(np.ones_like(z), low, 8, 16.0, motion=field(name)) == np.float32(1.0)).all()


@pytest.mark.gpu
def test_extreme_int8_fields_read_nothing_out_of_range():
    """Components beyond +-4 are the caller's error, but every read stays in range: at +-127 a frame and radius 8 every path has left the
    grid after one step, every tap but the centre is skipped and the output is the input bit for bit -- as float64 has it."""
    z, low, _ = scene("x3")
    for v in (127, -128):
        far = np.full((11, 8, 8, 2), v, dtype=np.int8)
        out = _smooth(z, low, 8, 16.0, motion=(far, far))
        np.testing.assert_array_equal(out, z)
    np.testing.assert_array_equal(ref.smooth_mc_ref(z[:4], low[:4], far[:3], far[:3], 3, 16.0), z[:4].astype(np.float64))


@pytest.mark.gpu
def test_one_bright_cell_is_found_two_columns_away():
    """Constant colour, two frames, z = 1 at cell (30, 32) of frame 1 alone, every forward vector (0, 2), every backward vector (0, -2),
    radius 1 (sigma_t = 0.5).  By hand: cell (30, 30) of frame 0 is carried to (30, 32) of frame 1, the bright cell is its centre tap there."""
    low = np.full((2, 64, 64, 3), 90, dtype=np.uint8)
    z = np.zeros((2, 64, 64), dtype=np.float32)
    z[1, 30, 32] = 1.0
    fwd = np.zeros((1, 8, 8, 2), dtype=np.int8)
    fwd[..., 1] = 2
    out = _smooth(z, low, 1, motion=(fwd, -fwd)).astype(np.float64)
    err = float(np.abs(out - ref.smooth_mc_ref(z, low, fwd, -fwd, 1, 16.0)).max())
    print(f"temporal.smooth one bright cell: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL
    wt, ws = np.exp(-1 / (2 * 0.25)), np.exp(-0.5)
    nine = wt * (1 + 4 * ws + 4 * ws * ws)                              # the nine cells of the other frame, all inside the grid
    assert abs(out[0, 30, 30] - wt / (1.0 + nine)) < 1e-6               # two columns away: the centre tap of the moved 3 x 3
    assert abs(out[0, 30, 31] - wt * ws / (1.0 + nine)) < 1e-6          # its taps sit around (30, 33): the bright cell is at dx = -1
    assert abs(out[0, 29, 29] - wt * ws * ws / (1.0 + nine)) < 1e-6     # around (29, 31): the diagonal neighbour
    assert out[0, 30, 32] == 0.0 and out[0, 30, 28] == 0.0              # around (30, 34) and (30, 30): out of the 3 x 3
    assert abs(out[1, 30, 32] - 1.0 / (1.0 + nine)) < 1e-6              # frame 1 keeps its cell and sees nine dark cells around (30, 30)
    # a cell at the right edge: the taps around (30, 63 + 2) have one column, dx = -1, inside the grid
    assert out[0, 30, 63] == 0.0
    z[1, 30, 32], z[1, 30, 63] = 0.0, 1.0
    out = _smooth(z, low, 1, motion=(fwd, -fwd)).astype(np.float64)
    assert abs(out[0, 30, 62] - wt * ws / (1.0 + wt * (ws + 2 * ws * ws))) < 1e-6             # around (30, 64): the three cells of column 63
    assert abs(out[0, 30, 61] - wt / (1.0 + wt * (1 + 3 * ws + 2 * ws * ws))) < 1e-6          # around (30, 63): six cells inside
    # without the field the cell two columns away sees nothing
    assert _smooth(z, low, 1)[0, 30, 61] == 0.0


# ---------------------------------------------------------------------------------------------------------------- the point of it
def flicker_figures(smooth_plain, smooth_motion):
    """Mean |out - clean| over frames 2 .. n - 3 of scene x3 at radius 3: (with the motion, without it, unsmoothed)."""
    z, low, clean = scene("x3")
    inner = slice(2, len(z) - 2)
    return tuple(float(np.abs(np.asarray(a, dtype=np.float64)[inner] - clean[inner]).mean())
                 for a in (smooth_motion(z, low), smooth_plain(z, low), z))


@pytest.mark.gpu
def test_flicker_under_a_pan_is_damped_more_with_the_motion():
    with_motion, without, unsmoothed = flicker_figures(
        lambda z, low: _smooth(z, low, 3), lambda z, low: _smooth(z, low, 3, motion=_flow(low, 4)))
    print(f"mean |out - clean| under a pan of 3 cells a frame: {with_motion:.4f} along the motion, {without:.4f} without, "
          f"{unsmoothed:.4f} unsmoothed")
    assert with_motion < without < unsmoothed


# ---------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.gpu
def test_chunks_equal_the_full_call():
    z, low, _ = (a[:13] for a in ref.pan(13, 1, -2, seed=9, flicker=0.15))
    zd, ld = _dev(z), _dev(low)
    whole = temporal.flow(ld, 4)
    full = temporal.smooth(zd, ld, 3, motion=whole)
    assert torch.equal(temporal.smooth(zd, ld, 3, f0=4, f1=9, motion=whole), full[4:9])
    parts, fields = [], []
    for lo in range(0, 13, 5):                                          # windows of 5 frames with 3-frame halos, the motion per window
        a, b = max(0, lo - 3), min(13, lo + 5 + 3)
        motion = temporal.flow(ld[a:b], 4)
        assert torch.equal(motion[0], whole[0][a:b - 1]) and torch.equal(motion[1], whole[1][a:b - 1])
        parts.append(temporal.smooth(zd[a:b], ld[a:b], 3, f0=lo - a, f1=min(13, lo + 5) - a, motion=motion))
    assert torch.equal(torch.cat(parts), full)
    # a halo one frame short is seen: the test can fail
    short = temporal.smooth(zd[3:13], ld[3:13], 3, f0=2, f1=7, motion=temporal.flow(ld[3:13], 4))
    assert not torch.equal(short[0], full[5]) and torch.equal(short[1:], full[6:10])


# ---------------------------------------------------------------------------------------------------------------- the entries' checks
@pytest.mark.gpu
def test_entry_argument_checks():
    """Both C entries refuse bad arguments before anything is launched."""
    lib = _lib.load()
    z = torch.zeros((4, 64, 64), dtype=torch.float32, device=DEV)
    low = torch.zeros((4, 64, 64, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((4, 64, 64), 7.0, dtype=torch.float32, device=DEV)
    fwd = torch.full((3, 8, 8, 2), 9, dtype=torch.int8, device=DEV)
    bwd = torch.full((3, 8, 8, 2), 9, dtype=torch.int8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    bad, unsupported = _lib.ERR_BADARG, _lib.ERR_UNSUPPORTED

    def flow(low_=low.data_ptr(), n=4, search=2, fwd_=fwd.data_ptr(), bwd_=bwd.data_ptr()):
        return lib.cgs_temporal_flow(low_, n, search, fwd_, bwd_, st)
    assert flow(low_=None) == bad and flow(fwd_=None) == bad and flow(bwd_=None) == bad
    assert flow(n=1) == bad and flow(n=0) == bad and flow(search=0) == bad and flow(search=-1) == bad and flow(search=5) == unsupported
    torch.cuda.synchronize()
    assert bool((fwd == 9).all()) and bool((bwd == 9).all())            # nothing was launched
    assert flow() == _lib.OK
    torch.cuda.synchronize()
    assert bool((fwd == 0).all()) and bool((bwd == 0).all())            # constant frames

    def call(z_=z.data_ptr(), low_=low.data_ptr(), fwd_=fwd.data_ptr(), bwd_=bwd.data_ptr(), n=4, f0=0, f1=4, radius=2, sr=16.0,
             out_=out.data_ptr()):
        return lib.cgs_temporal_smooth_mc(z_, low_, fwd_, bwd_, n, f0, f1, radius, sr, out_, st)
    assert call(z_=None) == bad and call(low_=None) == bad and call(out_=None) == bad and call(fwd_=None) == bad and call(bwd_=None) == bad
    assert call(radius=0) == bad and call(radius=-1) == bad and call(radius=9) == unsupported
    assert call(f0=2, f1=2) == bad and call(f0=3, f1=2) == bad and call(f1=5) == bad and call(f0=-1) == bad and call(n=0, f1=0) == bad
    assert call(sr=0.0) == bad and call(sr=-1.0) == bad and call(sr=float("nan")) == bad and call(sr=float("inf")) == bad
    assert call(z_=z.data_ptr() + 2) == bad and call(out_=out.data_ptr() + 1) == bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                     # nothing was launched
    assert call(fwd_=None, bwd_=None, n=1, f1=1) == _lib.OK             # one frame: the fields are not read
    torch.cuda.synchronize()
    assert bool((out[0] == 0.0).all()) and bool((out[1:] == 7.0).all())
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    # the module's own checks
    with pytest.raises(ValueError):
        temporal.flow(low, 0)
    with pytest.raises(ValueError):
        temporal.flow(low, 5)
    with pytest.raises(ValueError):
        temporal.flow(low.float(), 2)
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, motion=(fwd, bwd[:2]))
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, motion=(fwd, bwd.cpu()))
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, motion=(fwd.short(), bwd))
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, motion=fwd)
