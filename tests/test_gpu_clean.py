"""Mask clean-up on the GPU (cgs_mask_clean, cgs_amd.clean) against the per-pixel loops and flood fills of tests/clean_ref.py.
Everything is integer or selection: exact equality everywhere, `gated` compared bit for bit."""
import os
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
from cgs_amd import clean  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERNS = objects_ref.patterns()
FULL = dict(strong=0.8, open=1, close=2, fill=16, shape="cross", connectivity=4)
SINGLE = ([dict(open=r, shape=s) for s in ("square", "cross") for r in (1, 2, 3, 4)]
          + [dict(close=r, shape=s) for s in ("square", "cross") for r in (1, 2, 3, 4)]
          + [dict(fill=a, connectivity=c) for c in (4, 8) for a in (1, 4, 4096)]
          + [dict(open=0, close=0, fill=0)])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _gpu(src, **kw):
    """clean.clean, everything back on the host."""
    t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    res = clean.clean(t, **kw)
    torch.cuda.synchronize()
    n, h, w = (t[None] if t.dim() == 2 else t).shape
    assert res.mask.dtype == torch.bool and res.mask.shape == (n, h, w) and res.mask.device.type == "cuda"
    assert res.counts.dtype == torch.int32 and res.counts.shape == (n, 8) and res.counts.device.type == "cuda"
    if kw.get("want_gated"):
        assert res.gated.dtype == torch.float32 and res.gated.shape == (n, h, w) and res.gated.device.type == "cuda"
    else:
        assert res.gated is None
    return clean_ref.Cleaned(res.mask.cpu().numpy(), res.gated.cpu().numpy() if res.gated is not None else None, res.counts.cpu().numpy())


def _check(src, ref_src=None, **kw):
    """src: [n,h,w] array; the kernel's answer must be the checker's (of ref_src when the GPU is given another form of the stack)."""
    want = clean_ref.clean(src if ref_src is None else ref_src, **kw)
    got = _gpu(src, **kw)
    np.testing.assert_array_equal(got.mask, want.mask, err_msg=f"mask {kw}")
    np.testing.assert_array_equal(got.counts, want.counts, err_msg=f"counts {kw}")
    if kw.get("want_gated"):
        np.testing.assert_array_equal(_bits(got.gated), _bits(want.gated), err_msg=f"gated {kw}")
        thr = np.float32(kw["thresh"])
        np.testing.assert_array_equal(np.nan_to_num(got.gated, nan=-1.0) >= thr, got.mask)       # (gated holds no NaN: the assert says so)
    return want


def _soft(on, seed):
    """A float32 frame whose on pixels (>= 0.5) are `on`: 0.6 on, 0.1 off, and about one on pixel in 50 strong (0.9)."""
    rs = np.random.RandomState(seed)
    v = np.where(on, np.float32(0.6), np.float32(0.1)).astype(np.float32)
    v[on & (rs.rand(*on.shape) < 0.02)] = 0.9
    return v


# ---------------------------------------------------------------- single operations and a full spec
@pytest.mark.parametrize("name", list(PATTERNS))
def test_patterns(name):
    on = PATTERNS[name][None]
    for kw in SINGLE:
        _check(on, **kw)
    soft = _soft(PATTERNS[name], len(name))[None]
    for conn in (4, 8):
        _check(soft, thresh=0.5, inclusive=True, strong=0.8, connectivity=conn)
    _check(soft, thresh=0.5, inclusive=True, want_gated=True, **FULL)


def test_structured_stack():
    stack = np.stack([_structured(64, 64, seed)[1] for seed in range(6)])
    assert stack.dtype == np.float32 and 0.2 < (stack >= 0.5).mean() < 0.8
    want = _check(stack, thresh=0.5, inclusive=True, want_gated=True, **FULL)
    c = want.counts.sum(axis=0)
    assert c[5] > 0 and c[1] < c[0] and c[2] < c[1] and c[3] > c[2]              # hysteresis, opening and closing all do something here
    for kw in (dict(strong=0.9, connectivity=4), dict(strong=0.9, connectivity=8), dict(open=1), dict(open=2, shape="cross"),
               dict(close=1), dict(close=3, shape="cross"), dict(fill=1), dict(fill=4, connectivity=4), dict(fill=4096)):
        want = _check(stack, thresh=0.5, inclusive=True, want_gated=True, **kw)
        assert "fill" not in kw or 0 < want.counts[:, 7].sum() <= want.counts[:, 6].sum()          # and so does the filling
        _check(stack, thresh=0.5, inclusive=False, **kw)


# ---------------------------------------------------------------- a winding hole
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["serpentine", "spiral"])
def test_winding_hole(name, conn):
    """The inverted 62 x 62 pattern inside a one-pixel ring of on pixels: the off region is one long corridor that does not reach the
    edge -- the smallest input on which a flood with a bounded number of sweeps goes wrong."""
    corridor = objects_ref.serpentine(62, 62) if name == "serpentine" else objects_ref.spiral(62)
    on = np.ones((64, 64), dtype=bool)
    on[1:63, 1:63] = ~corridor
    found = clean_ref.holes(on, conn)
    area = int(corridor.sum())
    assert len(found) == 1 and len(found[0]) == area and area > 1800
    filled = _check(on[None], fill=area, connectivity=conn)
    assert filled.mask.all() and filled.counts[0].tolist()[4:] == [4096, 0, 1, 1]
    kept = _check(on[None], fill=area - 1, connectivity=conn)
    np.testing.assert_array_equal(kept.mask[0], on)
    assert kept.counts[0].tolist()[4:] == [4096 - area, 0, 1, 0]


# ---------------------------------------------------------------- holes and the edge
def test_holes_and_the_edge():
    full = np.ones((9, 11), dtype=bool)
    corner = full.copy()                               # an off region that reaches the frame's corner pixel through a diagonal step
    corner[0, 0] = corner[1, 1] = False
    diag = full.copy()                                 # a pocket joined to an off pixel of the last column by a diagonal step only
    diag[4, 8] = diag[3, 9] = diag[2, 10] = False
    last = full.copy()                                 # holes beside the edge, not on it; an off pixel in each edge row and column
    last[1, 1] = last[7, 9] = last[1, 9] = last[7, 1] = False
    last[0, 5] = last[8, 5] = last[4, 0] = last[4, 10] = False
    stack = np.stack([corner, diag, last])
    for conn in (4, 8):
        want = _check(stack, fill=4096, connectivity=conn)
        # conn 8: holes are 4-connected, so the diagonal steps cut them off from the edge and they fill; conn 4: they leak out
        assert bool(want.mask[0, 1, 1]) == (conn == 8) and not want.mask[0, 0, 0]
        assert bool(want.mask[1, 4, 8]) == (conn == 8) and bool(want.mask[1, 3, 9]) == (conn == 8) and not want.mask[1, 2, 10]
        assert want.counts[:, 6].tolist() == ([1, 2, 4] if conn == 8 else [0, 0, 4])
        assert want.mask[2, 1:8, 1:10].all() and not want.mask[2, 0, 5] and not want.mask[2, 4, 10]


# ---------------------------------------------------------------- hysteresis
def test_hysteresis_cases():
    v = np.full((5, 12, 14), 0.1, dtype=np.float32)
    v[0, 1:4, 1:4] = 0.6                               # two components, the strong pixel in one
    v[0, 6:9, 8:12] = 0.6
    v[0, 7, 9] = 0.95
    v[1, 2:5, 2:9] = 0.6                               # a pixel exactly equal to strong: strong under >=, weak under >
    v[1, 3, 4] = 0.8
    v[2, 1:6, 1:6] = 0.6                               # NaN cells are off: the row of them splits the block, the lower half has no strong pixel
    v[2, 3, 1:6] = np.nan
    v[2, 1, 1] = 0.9
    v[3, 2, 3:7] = 0.6                                 # the only strong pixel is the component's last in raster order
    v[3, 3:9, 3] = 0.6
    v[3, 8, 3:11] = 0.6
    v[3, 8, 10] = 0.9
    v[4, 4, 4], v[4, 5, 5] = 0.6, 0.9                  # joined by a diagonal step only
    for inclusive in (False, True):
        for conn in (4, 8):
            want = _check(v, thresh=0.5, inclusive=inclusive, strong=0.8, connectivity=conn, want_gated=True)
            assert want.counts[0].tolist()[:2] + [int(want.counts[0, 5])] == [21, 12, 1] and not want.mask[0, 1:4, 1:4].any()
            assert bool(want.mask[1].any()) == inclusive and want.counts[1, 5] == (0 if inclusive else 1)
            assert want.mask[2, 1:3, 1:6].all() and not want.mask[2, 3:].any() and want.counts[2, 5] == 1
            assert want.mask[3].sum() == 17 and want.counts[3, 5] == 0
            assert bool(want.mask[4, 4, 4]) == (conn == 8) and want.mask[4, 5, 5]


# ---------------------------------------------------------------- shapes and frame counts
@pytest.mark.parametrize("h,w,n", [(1, 1, 3), (1, 64, 3), (64, 1, 3), (63, 64, 3), (64, 63, 3), (17, 33, 1), (17, 33, 130)])
def test_shapes(h, w, n):
    rs = np.random.RandomState(1000 * h + 10 * w + n)
    v = rs.rand(n, h, w).astype(np.float32)
    v[rs.rand(n, h, w) < 0.01] = np.nan
    v[0] = 0.9                                         # a full frame first, an empty one last when there is room: neighbours must not leak
    if n > 1:
        v[-1] = 0.0
    _check(v, thresh=0.35, inclusive=True, want_gated=True, **FULL)
    _check(v, thresh=0.35, inclusive=False, open=2, fill=4, strong=0.6)
    if n <= 3:
        _check(v, thresh=0.35, inclusive=True, close=4)
        _check(v, thresh=0.35, inclusive=True, open=4, shape="cross", fill=4096, connectivity=4)


def test_source_kinds_and_views():
    rs = np.random.RandomState(7)
    v = rs.rand(4, 20, 31).astype(np.float32)
    v[rs.rand(*v.shape) < 0.1] = 0.5                   # cells exactly at the threshold: on under >=, off under >
    kw = dict(open=1, close=1, fill=2)
    gt = _check(v, thresh=0.5, inclusive=False, **kw)
    ge = _check(v, thresh=0.5, inclusive=True, **kw)
    assert gt.counts[:, 0].sum() < ge.counts[:, 0].sum()
    on = v >= 0.5
    same = _check(on, **kw)
    np.testing.assert_array_equal(same.mask, ge.mask)
    u8 = (on * rs.randint(1, 256, on.shape)).astype(np.uint8)            # any non-zero byte is on
    np.testing.assert_array_equal(_check(u8, **kw).mask, ge.mask)
    np.testing.assert_array_equal(_gpu(v[0], thresh=0.5, inclusive=True, **kw).mask, ge.mask[:1])          # [h,w] is one frame
    t = torch.from_numpy(v).to(DEV)
    np.testing.assert_array_equal(_gpu(t[::2], thresh=0.5, inclusive=True, **kw).mask, ge.mask[::2])        # a view is made contiguous
    np.testing.assert_array_equal(_gpu(t.transpose(1, 2), thresh=0.5, inclusive=True, fill=2).mask,
                                  clean_ref.clean(v.transpose(0, 2, 1), thresh=0.5, inclusive=True, fill=2).mask)


# ---------------------------------------------------------------- gated
def test_gated_is_selection():
    stack = np.stack([_structured(64, 64, seed)[1] for seed in (3, 4)])
    stack[0, 5, 5:9] = np.nan
    thr = np.float32(0.45)
    for inclusive in (False, True):
        want = _check(stack, thresh=float(thr), inclusive=inclusive, want_gated=True, **FULL)
        got = _gpu(stack, thresh=float(thr), inclusive=inclusive, want_gated=True, **FULL)
        np.testing.assert_array_equal(got.gated >= thr, got.mask)
        with np.errstate(invalid="ignore"):
            passes = (stack >= thr) if inclusive else (stack > thr)
        survive = got.mask & passes
        assert survive.any() and (got.mask & ~passes).any() and (~got.mask & passes).any()        # kept, added and removed cells
        np.testing.assert_array_equal(_bits(got.gated)[survive], _bits(stack)[survive])           # the input's bits
        assert (got.gated[got.mask & ~passes] == thr).all() and (got.gated[~got.mask] == 0).all()


def test_identity_spec_is_the_plain_threshold():
    stack = np.stack([_structured(64, 64, seed)[1] for seed in (5, 6, 7)])
    for inclusive in (False, True):
        with np.errstate(invalid="ignore"):
            plain = (stack >= np.float32(0.5)) if inclusive else (stack > np.float32(0.5))
        got = _gpu(stack, thresh=0.5, inclusive=inclusive, strong=0.5 if inclusive else None, open=0, close=0, fill=0, want_gated=True)
        np.testing.assert_array_equal(got.mask, plain)
        np.testing.assert_array_equal(_bits(got.gated), _bits(np.where(plain, stack, np.float32(0))))
        on = plain.sum(axis=(1, 2))
        np.testing.assert_array_equal(got.counts, np.stack([on] * 5 + [np.zeros_like(on)] * 3, axis=1))


# ---------------------------------------------------------------- streams and graphs
def test_other_stream_and_graph_replay():
    stack = np.stack([_structured(64, 64, seed)[1] for seed in range(8, 12)])
    t = torch.from_numpy(stack).to(DEV)
    kw = dict(thresh=0.5, inclusive=True, want_gated=True, **FULL)
    base = _gpu(t, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = clean.clean(t, **kw)
    side.synchronize()
    for got, want in zip(res, base):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = clean.clean(t, **kw)
    for out in held:
        out.zero_()                                    # the capture ran nothing; what the replay leaves is the replay's
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(held, base):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    t.copy_(torch.from_numpy(stack[::-1].copy()).to(DEV))                # the graph reads the tensor where it is
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(held, base):
        np.testing.assert_array_equal(got.cpu().numpy(), want[::-1])
