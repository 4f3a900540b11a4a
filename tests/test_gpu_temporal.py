"""Masks smoothed along time on the GPU (cgs_temporal_smooth, cgs_amd.temporal) against tests/temporal_ref.py: the filter against float64
within TOL, the cases that are exact in fp32 bit for bit, the sub-range and a chunked run against the one-call run bit for bit, border
cells and missing frames skipped, and the entry's argument checks.

TOL: an fp32 emulation of the formula in numpy in the kernel's tap order (temporal_ref.smooth_emul32) stays within EMUL_ERR of float64
over the nine (radius, sigma_r) settings and the three short stacks below: 3.8e-7 to 8.65e-7 at n = 12, at most 5.0e-7 on the short stacks (measured on the CPU on exactly these inputs, figure by figure
in test_tolerance_is_derived_from_the_emulation); thirty times that leaves room for the hardware exponential and the base-2 folding -- the
margin tests/test_gpu_fit.py gives them -- and is still far below a quarter of a grey level (9.8e-4).  The largest GPU error seen is
printed by every test that compares with float64."""
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

import temporal_ref  # noqa: E402
from cgs_amd import _lib, temporal  # noqa: E402

DEV = "cuda"
EMUL_ERR = 8.7e-7          # the largest |emulation - float64| over SETTINGS and SHORT, measured on the CPU
TOL = 30 * EMUL_ERR
SETTINGS = tuple((r, s) for r in (1, 3, 8) for s in (4.0, 16.0, 64.0))
SHORT = (1, 2, 5)                                  # stacks shorter than the window of radius 8: both ends clipped at once
A, B = (200, 30, 30), (20, 60, 220)


def drifting(n, seed=11):
    """(z float32 [n,64,64], low uint8 [n,64,64,3]): blocks of random colour and mask value, 5 to 23 cells a side and not aligned to
    anything, drifting one cell a frame, the colours with +-6 noise and z with +-0.05 noise per frame."""
    rs = np.random.RandomState(seed)
    by, bx = rs.randint(5, 24, 2)
    hh, ww = 64 // by + 2, (64 + n) // bx + 2
    colour = np.repeat(np.repeat(rs.randint(0, 256, (hh, ww, 3)), by, axis=0), bx, axis=1)
    value = np.repeat(np.repeat(rs.rand(hh, ww), by, axis=0), bx, axis=1)
    oy, ox = rs.randint(0, by), rs.randint(0, bx)
    low = np.stack([colour[oy:oy + 64, ox + f:ox + f + 64] for f in range(n)])
    z = np.stack([value[oy:oy + 64, ox + f:ox + f + 64] for f in range(n)])
    low = np.clip(low + rs.randint(-6, 7, low.shape), 0, 255).astype(np.uint8)
    z = np.clip(z + rs.uniform(-0.05, 0.05, z.shape), 0.0, 1.0).astype(np.float32)
    return z, low


@functools.lru_cache(maxsize=None)
def _case(n):
    z, low = drifting(n, seed=11 + n)
    z.setflags(write=False)
    low.setflags(write=False)
    return z, low


@functools.lru_cache(maxsize=None)
def _want(n, radius, sigma_r):
    out = temporal_ref.smooth_ref(*_case(n), radius, sigma_r)
    out.setflags(write=False)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def _smooth(z, low, radius, sigma_r=16.0, **kw):
    return temporal.smooth(_dev(z), _dev(low), radius, sigma_r, **kw).cpu().numpy()


def test_tolerance_is_derived_from_the_emulation():
    """No GPU: the fp32 emulation against float64 on the inputs of the GPU tests; EMUL_ERR is the largest of these figures."""
    worst = 0.0
    for n, radius, sigma_r in [(12, r, s) for r, s in SETTINGS] + [(n, 8, 16.0) for n in SHORT]:
        z, low = _case(n)
        err = float(np.abs(temporal_ref.smooth_emul32(z, low, radius, sigma_r).astype(np.float64) - _want(n, radius, sigma_r)).max())
        print(f"emulation n {n} radius {radius} sigma_r {sigma_r}: max |fp32 - float64| = {err:.3e}")
        worst = max(worst, err)
    assert worst <= EMUL_ERR and EMUL_ERR <= 1.25 * worst          # the constant is the measurement, rounded up
    assert TOL < 0.25 / 255


@pytest.mark.gpu
@pytest.mark.parametrize("n, radius, sigma_r", [(12, r, s) for r, s in SETTINGS] + [(n, 8, 16.0) for n in SHORT])
def test_against_float64(n, radius, sigma_r):
    z, low = _case(n)
    out = _smooth(z, low, radius, sigma_r)
    assert out.shape == (n, 64, 64) and out.dtype == np.float32
    assert not np.isnan(out).any() and out.min() >= 0.0 and out.max() <= 1.0
    err = float(np.abs(out.astype(np.float64) - _want(n, radius, sigma_r)).max())
    print(f"temporal.smooth n {n} radius {radius} sigma_r {sigma_r}: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL
    if n > 1:
        assert np.abs(out - z).max() > 100 * TOL                       # the filter did something


@pytest.mark.gpu
def test_exact_cases():
    z, low = _case(12)
    ones = _smooth(np.ones_like(z), low, 3)
    assert (ones == np.float32(1.0)).all()
    zeros = _smooth(np.zeros_like(z), low, 3)
    assert (zeros == 0.0).all()
    rs = np.random.RandomState(3)
    ends = rs.randint(0, 2, z.shape).astype(np.float32)                 # only 0.0 and 1.0: the bounds are reached and not passed
    out = _smooth(ends, low, 8, 64.0)
    assert out.min() >= 0.0 and out.max() <= 1.0 and 0.0 < out.mean() < 1.0


@pytest.mark.gpu
def test_scene_cut_passes_unchanged():
    """d2 / (2 sigma_r^2) = 69400 / 512 = 135.5 nats between the two scenes, past fp32's smallest subnormal (103 nats): the weights
    across the cut are +0 exactly, and inside a scene every tap has the value of the centre: the output is the input bit for bit."""
    low = np.empty((10, 64, 64, 3), dtype=np.uint8)
    low[:5], low[5:] = A, B
    z = np.concatenate((np.ones((5, 64, 64), dtype=np.float32), np.zeros((5, 64, 64), dtype=np.float32)))
    for radius in (1, 3, 8):
        np.testing.assert_array_equal(_smooth(z, low, radius, 16.0), z)
    # the same cut with a wide range sigma does mix the scenes: the cut is what stopped it
    mixed = _smooth(z, low, 3, 1000.0)
    assert mixed[4].max() < 1.0 and mixed[5].min() > 0.0


@pytest.mark.gpu
def test_flicker_is_damped():
    n = 12
    low = np.full((n, 64, 64, 3), 117, dtype=np.uint8)
    z = np.empty((n, 64, 64), dtype=np.float32)
    z[0::2], z[1::2] = 0.2, 0.8
    out = _smooth(z, low, 3)
    want = temporal_ref.smooth_ref(z, low, 3, 16.0)
    err = float(np.abs(out.astype(np.float64) - want).max())
    print(f"temporal.smooth flicker: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL
    v_in, v_out = float(z[:, 30, 30].var()), float(out[:, 30, 30].var())
    print(f"variance along time at (30, 30): {v_in:.4f} in, {v_out:.6f} out")
    assert v_out < 0.25 * v_in


@pytest.mark.gpu
def test_sub_range_and_chunks_equal_the_full_call():
    z, low = drifting(13, seed=5)
    zd, ld = _dev(z), _dev(low)
    full = temporal.smooth(zd, ld, 3)
    assert torch.equal(temporal.smooth(zd, ld, 3, f0=4, f1=9), full[4:9])
    assert torch.equal(temporal.smooth(zd, ld, 3, f0=12), full[12:])
    parts = []
    for lo in range(0, 13, 5):                                          # windows of 5 frames with 3-frame halos
        a, b = max(0, lo - 3), min(13, lo + 5 + 3)
        parts.append(temporal.smooth(zd[a:b], ld[a:b], 3, f0=lo - a, f1=min(13, lo + 5) - a))
    assert torch.equal(torch.cat(parts), full)
    # a halo one frame short is seen: the test can fail
    short = temporal.smooth(zd[3:13], ld[3:13], 3, f0=2, f1=7)          # frame 5 with frames 3 and 4 before it, not 2
    assert not torch.equal(short[0], full[5]) and torch.equal(short[1:], full[6:10])


@pytest.mark.gpu
def test_border_cells_and_missing_frames_are_skipped():
    """One bright cell at a corner of frame 0 on a constant colour: clamping would count the corner cell (and frame 0) several times."""
    n = 4
    low = np.full((n, 64, 64, 3), 90, dtype=np.uint8)
    z = np.zeros((n, 64, 64), dtype=np.float32)
    z[0, 0, 0] = 1.0
    for radius in (1, 2):
        out = _smooth(z, low, radius).astype(np.float64)
        want = temporal_ref.smooth_ref(z, low, radius, 16.0)
        err = float(np.abs(out - want).max())
        print(f"temporal.smooth corner cell radius {radius}: max |out - float64| = {err:.3e} (bound {TOL:.3e})")
        assert err <= TOL
    # by hand, radius 1 (sigma_t = 0.5): frame 0 keeps its own corner (weight 1) and sees 4 cells of frame 1, all 0
    wt, ws = np.exp(-1 / (2 * 0.25)), np.exp(-0.5)
    out = _smooth(z, low, 1).astype(np.float64)
    assert abs(out[0, 0, 0] - 1.0 / (1.0 + wt * (1 + 2 * ws + ws * ws))) < 1e-6
    # frame 1, cell (1, 1): the corner cell of frame 0 is its diagonal neighbour; frames 0 and 2 both count nine cells
    assert abs(out[1, 1, 1] - wt * ws * ws / (1.0 + 2 * wt * (1 + 4 * ws + 4 * ws * ws))) < 1e-6
    assert (out[2:] == 0.0).all()


@pytest.mark.gpu
def test_entry_argument_checks():
    """The C entry refuses bad arguments before anything is launched."""
    lib = _lib.load()
    z = torch.zeros((4, 64, 64), dtype=torch.float32, device=DEV)
    low = torch.zeros((4, 64, 64, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((4, 64, 64), 7.0, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(z_=z.data_ptr(), low_=low.data_ptr(), n=4, f0=0, f1=4, radius=2, sr=16.0, out_=out.data_ptr()):
        return lib.cgs_temporal_smooth(z_, low_, n, f0, f1, radius, sr, out_, st)
    bad = _lib.ERR_BADARG
    assert call(z_=None) == bad and call(low_=None) == bad and call(out_=None) == bad
    assert call(radius=0) == bad and call(radius=-1) == bad and call(radius=9) == _lib.ERR_UNSUPPORTED
    assert call(f0=2, f1=2) == bad and call(f0=3, f1=2) == bad and call(f1=5) == bad and call(f0=-1) == bad and call(n=0, f1=0) == bad
    assert call(sr=0.0) == bad and call(sr=-1.0) == bad and call(sr=float("nan")) == bad and call(sr=float("inf")) == bad
    assert call(z_=z.data_ptr() + 2) == bad and call(out_=out.data_ptr() + 1) == bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                     # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    # the module's own checks
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 0)
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 9)
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, f0=2, f1=2)
    with pytest.raises(ValueError):
        temporal.smooth(z, low[:3], 2)
    with pytest.raises(ValueError):
        temporal.smooth(z, low, 2, sigma_r=0.0)
