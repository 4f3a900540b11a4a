"""cgs_graph_cut (csrc/graph_cut.hip) through graphcut.cut against tests/graph_cut_ref.py (scipy's Dinic on the whole graph, the cut by
a backward search in capacity - flow): the mask, the energy and every stats column are compared bit for bit.  The one column the
reference cannot give is `rounds` -- how many searches the kernel's schedule ran, which no schedule-free reference knows; it is held
by two conditions instead: no frame of any stack here reports NOT_CONVERGED, and every frame's rounds are at most a quarter of the
default max_rounds (and at least 1 where a cut ran).

The stacks are small on purpose (the reference costs about 0.2 s for a 64 x 64 frame): every shape at which an index can go wrong (one
cell, one row, one column, 2 x 3, a width below the full 64, the full frame), more workgroups than CUs, every kind of mask cell, and
frames that drive the n-links to both ends of their table.  About the serpentine: with the rule's beta = 1 / (2 <d2>) a corridor whose
walls make up half of the frame's pairs leaves the wall arcs at about exp(-1) of the full weight, so flow also crosses the walls; the
case is kept as the issue describes it (the longest corridor a frame holds, seeded at its two ends), and the longest residual paths
that only run along one line are the 1 x 64 and 64 x 1 frames and "deep-corridor", whose walls carry nothing (561 levels in one search)."""
import functools

import numpy as np
import pytest
import torch

import graph_cut_ref as ref
from cgs_amd import graphcut

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def textured(rs, n, h, w):
    """Frames of two textured regions split by a slanted edge, and masks that follow the split loosely: blob-like soft masks."""
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.empty((n, h, w, 3), dtype=np.uint8)
    masks = np.empty((n, h, w), dtype=np.float32)
    for i in range(n):
        cy, cx, r = rs.uniform(0.2, 0.8) * h, rs.uniform(0.2, 0.8) * w, rs.uniform(0.2, 0.5) * max(h, w, 2)
        inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        a, b = rs.randint(0, 256, 3), rs.randint(0, 256, 3)
        frames[i] = np.clip(np.where(inside[..., None], a, b) + rs.randint(-40, 41, (h, w, 3)), 0, 255)
        soft = np.where((yy - cy - 0.15 * r) ** 2 + (xx - cx + 0.1 * r) ** 2 <= (0.8 * r) ** 2, 0.8, 0.15)
        masks[i] = np.clip(soft + rs.normal(0, 0.2, (h, w)), 0, 1)
    return frames, masks


def serpentine():
    """A one-cell-wide corridor through a 64 x 64 frame -- the even rows, joined at alternating ends -- 2079 cells long, of one colour
    in a contrasting frame; its two end cells are hard foreground, every other cell is unknown and off."""
    frame = np.empty((64, 64, 3), dtype=np.uint8)
    frame[:] = (20, 20, 200)
    frame[0::2] = (200, 40, 40)
    for k, y in enumerate(range(1, 63, 2)):
        frame[y, 63 if k % 2 == 0 else 0] = (200, 40, 40)
    z = np.full((64, 64), 0.3, dtype=np.float32)
    z[0, 0] = z[62, 0] = 1.0                               # (row 62 is entered at x = 63 and ends at x = 0)
    return frame[None], z[None]


def deep_corridor():
    """A corridor the flow cannot leave: every eighth row, joined at alternating ends by columns, 561 cells of one colour between walls
    seven cells thick.  Only an eighth of the frame's pairs cross a wall, so their idx = 64 d2 / m is 512 and at lambda = 1 their
    capacity rint(16 exp(-4)) is 0, while a pair inside the corridor has 16.  The corridor is on and unknown, with hard foreground at
    one end and hard background at the other: no corridor cell but the last has a sink arc left (cost_bg > cost_fg), so the first
    search from the sink walks the whole corridor, 561 levels deep."""
    frame = np.empty((64, 64, 3), dtype=np.uint8)
    frame[:] = (20, 20, 200)
    z = np.full((64, 64), 0.3, dtype=np.float32)
    rows = list(range(0, 64, 8))
    for k, y in enumerate(rows):
        frame[y], z[y] = (200, 40, 40), 0.6
        if k + 1 < len(rows):
            x = 63 if k % 2 == 0 else 0
            frame[y:y + 8, x], z[y:y + 8, x] = (200, 40, 40), 0.6
    z[0, 0], z[56, 0] = 1.0, 0.0                          # (row 56 is entered at x = 63 and ends at x = 0)
    return frame[None], z[None]


def two_colour_shifted():
    """Left half one colour, right half another (a little noise); the mask's edge lies three cells to the right of the colour edge,
    so the first cut moves the labelling and the second returns it."""
    rs = np.random.RandomState(11)
    frame = np.empty((20, 24, 3), dtype=np.int64)
    frame[:, :12], frame[:, 12:] = (220, 60, 30), (30, 90, 220)
    frame = np.clip(frame + rs.randint(-6, 7, frame.shape), 0, 255).astype(np.uint8)
    z = np.full((20, 24), 0.35, dtype=np.float32)
    z[:, :15] = 0.65
    z[:, :4], z[:, 20:] = 0.95, 0.02
    return frame[None], z[None]


@functools.lru_cache(maxsize=None)
def case(name):
    """(frames uint8 [n,h,w,3], masks float32 [n,h,w], thresh, keywords of cut) of a named stack."""
    rs = np.random.RandomState(sum(map(ord, name)))
    kw = {}
    if name.startswith("shape-"):
        h, w = (int(v) for v in name[6:].split("x"))
        f, z = textured(rs, 1, h, w)
    elif name == "n3":
        f, z = textured(rs, 3, 17, 23)
    elif name == "n300":
        f, z = textured(rs, 300, 8, 8)
    elif name in ("all-fg", "all-bg", "no-seed", "all-unknown", "nan", "ties-gt", "ties-ge"):
        f, _ = textured(rs, 2, 16, 19)
        if name == "all-fg":
            z = np.ones((2, 16, 19), dtype=np.float32)
        elif name == "all-bg":
            z = np.zeros((2, 16, 19), dtype=np.float32)
        elif name == "no-seed":                              # unknown and off everywhere
            z = rs.uniform(0.3, 0.45, (2, 16, 19)).astype(np.float32)
        elif name == "all-unknown":
            z = rs.uniform(0.3, 0.7, (2, 16, 19)).astype(np.float32)
        elif name == "nan":
            z = rs.uniform(0, 1, (2, 16, 19)).astype(np.float32)
            z[rs.rand(2, 16, 19) < 0.2] = np.nan
            z[1, 0] = np.nan
        else:                                                # exactly lo, thresh and hi, and their float32 neighbours
            t, a, b = np.float32(0.5), np.float32(0.25), np.float32(0.75)
            vals = np.array([a, t, b, np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(1)), np.nextafter(t, np.float32(0)),
                             np.nextafter(t, np.float32(1)), np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1)), 0.0, 1.0],
                            dtype=np.float32)
            z = vals[rs.randint(0, len(vals), (2, 16, 19))]
            kw = dict(inclusive=name == "ties-ge", lo=0.25, hi=0.75)
    elif name == "flat":
        _, z = textured(rs, 1, 21, 30)
        f = np.full((1, 21, 30, 3), 97, dtype=np.uint8)
    elif name == "checkerboard":
        _, z = textured(rs, 1, 22, 27)
        yy, xx = np.mgrid[0:22, 0:27]
        f = np.where(((yy + xx) % 2 == 0)[None, ..., None], np.array([250, 250, 10]), np.array([10, 30, 240])).astype(np.uint8)
    elif name == "serpentine":
        f, z = serpentine()
        kw = dict(lo=0.25, hi=0.75, connectivity=4)
    elif name == "deep-corridor":
        f, z = deep_corridor()
        kw = dict(lo=0.25, hi=0.75, connectivity=4, lam=1)
    elif name in ("noise-l100", "noise-l0"):
        f = rs.randint(0, 256, (1, 64, 64, 3)).astype(np.uint8)
        z = rs.uniform(0, 1, (1, 64, 64)).astype(np.float32)
        kw = dict(lam=100 if name == "noise-l100" else 0)
    elif name.startswith("conn"):                           # conn4-bins8 ...
        f, z = textured(rs, 2, 24, 31)
        kw = dict(connectivity=int(name[4]), bins=int(name[-1]))
    elif name == "it1":
        f, z = textured(rs, 2, 24, 31)
        kw = dict(iters=1)
    elif name == "it8-early":
        f, z = two_colour_shifted()
        kw = dict(iters=8, lo=0.1, hi=0.9)
    else:
        raise KeyError(name)
    return f, z, 0.5, kw


@functools.lru_cache(maxsize=None)
def expected(name):
    f, z, thresh, kw = case(name)
    return ref.cut(f, z, thresh, **kw)


def run(name, **more):
    f, z, thresh, kw = case(name)
    res = graphcut.cut(torch.from_numpy(f).to(DEV), torch.from_numpy(z).to(DEV), thresh, **{**kw, **more})
    torch.cuda.synchronize()
    return res.mask.cpu().numpy(), res.stats.cpu().numpy().astype(np.int64)


CASES = ["shape-1x1", "shape-1x64", "shape-64x1", "shape-2x3", "shape-63x64", "shape-64x64", "n3", "n300", "all-fg", "all-bg", "no-seed",
         "all-unknown", "nan", "ties-gt", "ties-ge", "flat", "checkerboard", "serpentine", "deep-corridor", "noise-l100", "noise-l0", "conn4-bins4",
         "conn4-bins8", "conn8-bins4", "conn8-bins8", "it1", "it8-early"]
NOT_ROUNDS = [c for c in range(8) if c != ref.ROUNDS]


@pytest.mark.parametrize("name", CASES)
def test_matches_reference(name):
    want = expected(name)
    mask, stats = run(name)
    print(name, "rounds", stats[:, ref.ROUNDS].max(), "iterations", stats[:, ref.ITERATIONS].tolist()[:4], "status", sorted(set(stats[:, 0])))
    assert mask.dtype == np.bool_ and mask.shape == want.mask.shape
    np.testing.assert_array_equal(stats[:, NOT_ROUNDS], want.stats[:, NOT_ROUNDS])
    np.testing.assert_array_equal(mask, want.mask)
    # the two conditions on the schedule
    assert not (stats[:, ref.STATUS] & ref.NOT_CONVERGED).any()
    assert (stats[:, ref.ROUNDS] <= graphcut.MAX_ROUNDS // 4).all()
    assert ((stats[:, ref.ROUNDS] >= 1) == (stats[:, ref.ITERATIONS] >= 1)).all()


def test_cases_are_what_they_claim():
    """The reference's own view of the special stacks: the status bits and counts that make them the cases of the list above."""
    s = lambda name: expected(name).stats
    assert (s("all-fg")[:, ref.STATUS] == ref.EMPTY).all() and (s("all-fg")[:, ref.ON] == 16 * 19).all()
    assert (s("all-bg")[:, ref.STATUS] == ref.EMPTY).all() and (s("all-bg")[:, ref.ON] == 0).all()
    assert (s("no-seed")[:, ref.STATUS] == ref.EMPTY).all() and (s("no-seed")[:, ref.UNKNOWN] == 16 * 19).all()
    assert (s("all-unknown")[:, ref.UNKNOWN] == 16 * 19).all() and (s("all-unknown")[:, ref.ITERATIONS] >= 1).all()
    assert (s("it1")[:, ref.ITERATIONS] == 1).all()
    early = s("it8-early")[0]
    assert early[ref.STATUS] == ref.EARLY and early[ref.ITERATIONS] == 2 and early[ref.CHANGED] > 0
    ties_gt, ties_ge = expected("ties-gt"), expected("ties-ge")
    assert (ties_gt.stats[:, ref.SEED_ON] < ties_ge.stats[:, ref.SEED_ON]).all()       # cells at thresh exactly
    assert expected("serpentine").stats[0, ref.UNKNOWN] == 64 * 64 - 2
    f, z, thresh, kw = case("deep-corridor")
    WA, WD, _ = (t.astype(np.int64) for t in graphcut.tables(kw["lam"]))
    links, _m = ref.n_links(f[0], 4, WA, WD)
    inside = (f[0][..., 0] == 200).ravel()
    assert inside.sum() == 561 and {c for p, q, c in links if inside[p] != inside[q]} == {0}
    assert {c for p, q, c in links if inside[p] and inside[q]} == {16} and sum(1 for p, q, c in links if inside[p] and inside[q]) == 560


@pytest.mark.parametrize("sweeps", [16, 64])
def test_sweeps_do_not_change_the_result(sweeps):
    want = expected("conn8-bins8")
    mask, stats = run("conn8-bins8", sweeps=sweeps)
    np.testing.assert_array_equal(stats[:, NOT_ROUNDS], want.stats[:, NOT_ROUNDS])
    np.testing.assert_array_equal(mask, want.mask)


def test_round_cap_is_a_bounded_exit():
    """max_rounds=1 on the noise frame: the cut cannot finish in one search, so the kernel returns normally with NOT_CONVERGED, the
    seed labelling and no completed cut."""
    f, z, thresh, kw = case("noise-l100")
    mask, stats = run("noise-l100", max_rounds=1)
    seed = z > np.float32(thresh)
    assert stats[0, ref.STATUS] == ref.NOT_CONVERGED
    np.testing.assert_array_equal(mask, seed)
    assert stats[0, ref.ITERATIONS] == 0 and stats[0, ref.ROUNDS] == 1 and stats[0, ref.ENERGY] == 0
    assert stats[0, ref.SEED_ON] == seed.sum() == stats[0, ref.ON] and stats[0, ref.CHANGED] == 0
    assert stats[0, ref.UNKNOWN] == expected("noise-l100").stats[0, ref.UNKNOWN]


def test_refusals():
    f = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    z = torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV)
    for bad in (dict(lo=0.6), dict(hi=0.4), dict(lam=101), dict(iters=0), dict(iters=9), dict(bins=16), dict(connectivity=6),
                dict(max_rounds=0), dict(lo=float("nan"))):
        with pytest.raises(ValueError):
            graphcut.cut(f, z, 0.5, **bad)
    with pytest.raises(ValueError):
        graphcut.cut(f, z.double(), 0.5)
    with pytest.raises(ValueError):
        graphcut.cut(f[:, :4], z, 0.5)
    with pytest.raises(ValueError):
        graphcut.cut(torch.zeros((1, 65, 8, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 65, 8), device=DEV), 0.5)
