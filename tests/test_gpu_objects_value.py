"""The value of an object on the GPU (cgs_objects_ablate, cgs_objects_select; cgs_amd.objects.ablate / value / select) against
tests/objects_value_ref.py, bit for bit.  The critic of the value tests carries the weights of fixture G1; what is compared there is the
kernel's images against the reference's, through the same critic in the same batches."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_value_ref as ref  # noqa: E402
from cgs_amd import objects  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLOUR = (200, 17, 96)


def _blocks(skip=()):
    """An 8 x 8 grid of 6 x 6 blocks, the outer ones on the four borders; `skip`: grid positions left out."""
    m = np.zeros((64, 64), dtype=bool)
    for by in range(8):
        for bx in range(8):
            if (by, bx) in skip:
                continue
            y0, x0 = (8 * by if by < 7 else 58), (8 * bx if bx < 7 else 58)
            m[y0:y0 + 6, x0:x0 + 6] = True
    return m


def _masks():
    """Five frames: 2048 isolated pixels (4-connectivity), nothing, one L-shaped blob, 63 blocks, 64 blocks."""
    yy, xx = np.mgrid[0:64, 0:64]
    blob = np.zeros((64, 64), dtype=bool)
    blob[20:40, 30:34] = True
    blob[36:40, 30:50] = True
    return np.stack([(yy + xx) % 2 == 0, np.zeros((64, 64), dtype=bool), blob, _blocks(skip=[(3, 3)]), _blocks()])


@pytest.fixture(scope="module")
def stack():
    """(frames uint8 [5,64,64,3], labels int32 [5,64,64], kept [5], table [5,64,8]) as host arrays, and objects.label's result."""
    frames = np.random.default_rng(7).integers(0, 256, size=(5, 64, 64, 3), dtype=np.uint8)
    res = objects.label(torch.from_numpy(_masks()).to(DEV), connectivity=4, max_objects=64, want_labels=True, want_mask=True)
    kept = res.kept.cpu().numpy()
    assert kept.tolist() == [2048, 0, 1, 63, 64]
    return frames, res.labels.cpu().numpy(), kept, res.table.cpu().numpy(), res


def _fill(kind):
    if kind == "frame":
        return np.random.default_rng(11).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    return "mean" if kind == "mean" else COLOUR


def _gpu_ablate(frames, labels, kept, fill, grow, rng=None, pick=slice(None)):
    f = torch.from_numpy(fill).to(DEV) if isinstance(fill, np.ndarray) else fill
    ab = objects.ablate(torch.from_numpy(np.ascontiguousarray(frames[pick])).to(DEV), torch.from_numpy(np.ascontiguousarray(labels[pick])).to(DEV),
                        torch.from_numpy(np.ascontiguousarray(kept[pick])).to(DEV), fill=f, grow=grow, frames_range=rng)
    return [t.cpu().numpy() for t in ab]


def _same(got, want):
    for g, w, name in zip(got, want, ("images", "row_frame", "row_label", "offsets")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("grow", [0, 1, 4])
@pytest.mark.parametrize("kind", ["colour", "frame", "mean"])
def test_ablate_matches_the_reference(stack, kind, grow):
    frames, labels, kept, _, _ = stack
    fill = _fill(kind)
    want = ref.ablate(frames, labels, kept, fill, grow)
    got = _gpu_ablate(frames, labels, kept, fill, grow)
    assert want[0].shape[0] == 64 + 0 + 1 + 63 + 64 and got[3].tolist() == [0, 64, 64, 65, 128, 192]
    _same(got, want)
    if grow == 0 and kind == "colour":                         # the 2048-label frame: 64 rows, one cell replaced in each
        changed = (got[0][:64] != frames[0][None]).any(axis=-1).reshape(64, -1).sum(axis=1)
        assert (changed <= 1).all() and changed.sum() >= 60    # (a cell that already has the colour does not show)


def test_ablate_mean_without_background_and_n_1(stack):
    frames, labels, kept, _, _ = stack
    full = np.ones((1, 64, 64), dtype=np.int32)                # a full-frame object: the mean falls back to all 4096 cells
    one = np.array([1], dtype=np.int32)
    _same(_gpu_ablate(frames[:1], full, one, "mean", 0), ref.ablate(frames[:1], full, one, "mean", 0))
    half = np.zeros((1, 64, 64, 3), dtype=np.uint8)            # the rounding at exactly .5
    half[0, 0, :, 0], half[0, 1, :, 1] = 32, 31
    got = _gpu_ablate(half, full, one, "mean", 2)
    assert (got[0] == (1, 0, 0)).all()
    _same(got, ref.ablate(half, full, one, "mean", 2))
    for f in (2, 4):                                           # n = 1: the blob alone, the 64 blocks alone
        pick = slice(f, f + 1)
        for grow in (0, 3):
            _same(_gpu_ablate(frames, labels, kept, "mean", grow, pick=pick), ref.ablate(frames[pick], labels[pick], kept[pick], "mean", grow))


def test_ablate_without_objects_launches_nothing(stack):
    frames, labels, kept, _, _ = stack
    empty = np.zeros((2, 64, 64), dtype=np.int32)
    got = _gpu_ablate(frames[:2], empty, np.zeros(2, dtype=np.int32), COLOUR, 1)
    assert got[0].shape == (0, 64, 64, 3) and got[1].shape == (0,) and got[2].shape == (0,) and got[3].tolist() == [0, 0, 0]
    _same(got, ref.ablate(frames[:2], empty, [0, 0], COLOUR, 1))
    got = _gpu_ablate(frames, labels, kept, COLOUR, 1, rng=(1, 2))                # the one frame of the stack that has no object
    assert got[0].shape[0] == 0 and got[3].tolist() == [0, 64, 64, 65, 128, 192]
    # labels without a count: kept says 0, so there is no row whatever the labels hold
    got = _gpu_ablate(frames[:2], labels[3:5], np.zeros(2, dtype=np.int32), COLOUR, 0)
    assert got[0].shape[0] == 0


def test_ablate_frames_range_at_every_cut(stack):
    frames, labels, kept, _, _ = stack
    fill = _fill("frame")
    whole = _gpu_ablate(frames, labels, kept, fill, 2)
    _same(whole, ref.ablate(frames, labels, kept, fill, 2))
    for cut in range(6):
        a, b = _gpu_ablate(frames, labels, kept, fill, 2, rng=(0, cut)), _gpu_ablate(frames, labels, kept, fill, 2, rng=(cut, 5))
        _same(a, ref.ablate(frames, labels, kept, fill, 2, frames_range=(0, cut)))
        for k in range(3):
            np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), whole[k])
        np.testing.assert_array_equal(a[3], whole[3])
        np.testing.assert_array_equal(b[3], whole[3])
    # a kept count above the labels and a smaller max_objects: rows come from kept, labels above K match nothing
    ab = objects.ablate(*(torch.from_numpy(a).to(DEV) for a in (frames, labels, kept)), fill=COLOUR, grow=1, max_objects=5)
    _same([t.cpu().numpy() for t in ab], ref.ablate(frames, labels, kept, COLOUR, 1, K=5))


# ---------------------------------------------------------------------------------------------------------------- value
@pytest.fixture(scope="module")
def critic(g1):
    from cgs_amd import engine
    pc, pm = g1
    e = engine.HourglassEngine(8, dropout=0.0)
    e.load_state(pc, pm)
    return lambda X: e.infer(X, want_mask=False)[0]


@pytest.fixture(scope="module")
def scenes(golden, stack):
    """Five frames for the critic: four of fixture G6's and one of a single colour; the labels of `stack`, the 2048-pixel frame last but
    one and the 64 blocks on the uniform frame."""
    _, labels, kept, _, _ = stack
    g6 = golden("g6_process.npz")["frames"]
    frames = np.concatenate([g6[:4], np.broadcast_to(np.array(COLOUR, dtype=np.uint8), (1, 64, 64, 3))]).astype(np.uint8)
    order = [2, 3, 1, 0, 4]                                    # rows 1, 63, 0, 64, 64
    return np.ascontiguousarray(frames), np.ascontiguousarray(labels[order]), np.ascontiguousarray(kept[order])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _expected_value(infer, frames, labels, kept, fill, grow, chunk_rows):
    """objects.value from the reference's images: the same critic, the same batches in the same order, np.float32 subtraction."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    base = np.concatenate([infer(dev(frames[lo:lo + chunk_rows])).cpu().numpy() for lo in range(0, len(frames), chunk_rows)]).astype(np.float32)
    fill_frame = None
    if isinstance(fill, str) and fill == "low":
        fill_frame = int(np.argmin(base))
        fill = frames[fill_frame]
    images, row_frame, row_label, offsets = ref.ablate(frames, labels, kept, fill, grow)
    chunks = ref.chunks(ref.row_counts(kept), chunk_rows)
    drop = np.zeros((len(frames), 64), dtype=np.float32)
    for f0, f1, rows in chunks:
        lo, hi = int(offsets[f0]), int(offsets[f1])
        assert hi - lo == rows
        pred = infer(dev(images[lo:hi])).cpu().numpy().astype(np.float32)
        drop[row_frame[lo:hi], row_label[lo:hi] - 1] = base[row_frame[lo:hi]] - pred
    return base, drop, fill_frame, chunks


@pytest.mark.parametrize("chunk_rows", [64, 2048])
@pytest.mark.parametrize("kind", ["low", "mean", "colour", "frame"])
def test_value_matches_the_reference_images_through_the_same_critic(critic, scenes, kind, chunk_rows):
    frames, labels, kept = scenes
    fill = "low" if kind == "low" else _fill(kind)
    base, drop, fill_frame, chunks = _expected_value(critic, frames, labels, kept, fill, 1, chunk_rows)
    val = objects.value(critic, *(torch.from_numpy(a).to(DEV) for a in (frames, labels, kept)),
                        fill=torch.from_numpy(fill).to(DEV) if isinstance(fill, np.ndarray) else fill, grow=1, chunk_rows=chunk_rows)
    assert val.chunks == chunks and val.fill_frame == fill_frame and val.rows == 192
    assert val.chunks == ([(0, 3, 64), (3, 4, 64), (4, 5, 64)] if chunk_rows == 64 else [(0, 5, 192)])
    assert val.base.dtype == torch.float32 and val.drop.dtype == torch.float32 and tuple(val.drop.shape) == (5, 64)
    np.testing.assert_array_equal(_bits(val.base.cpu().numpy()), _bits(base))
    got = val.drop.cpu().numpy()
    print(f"{kind} chunk_rows={chunk_rows}: base {base.tolist()}, drop min {got.min():.6g} max {got.max():.6g}, "
          f"distinct {len(np.unique(got))}")
    np.testing.assert_array_equal(_bits(got), _bits(drop))
    assert not got[2].any() and not got[0, 1:].any()           # entries without a row are 0
    if kind == "colour":                                       # the uniform frame filled with its own colour: rebuilt unchanged
        assert (got[4] == 0.0).all()
    if kind == "low":                                          # the fill frame's own objects
        assert (got[fill_frame] == 0.0).all()
    assert len(np.unique(got)) > 2                             # the critic does tell some of these objects apart


# ---------------------------------------------------------------------------------------------------------------- select
def _keeps(kept):
    n = len(kept)
    every, none = np.ones((n, 64), dtype=bool), np.zeros((n, 64), dtype=bool)
    alternating = np.zeros((n, 64), dtype=bool)
    alternating[:, ::2] = True
    last = np.zeros((n, 64), dtype=bool)
    for f, c in enumerate(ref.row_counts(kept)):
        if c:
            last[f, c - 1] = True
    mixed = np.random.default_rng(3).integers(0, 2, size=(n, 64)).astype(bool)
    return {"all": every, "none": none, "alternating": alternating, "last": last, "mixed": mixed}


@pytest.mark.parametrize("which", ["all", "none", "alternating", "last", "mixed"])
def test_select_matches_the_reference_and_tracks_alike(stack, which):
    _, labels, kept, table, res = stack
    keep = _keeps(kept)[which]
    want = ref.select(labels, table, kept, keep)
    as_u8 = which == "mixed"                                    # keep as uint8 with values other than 0 / 1
    dev_keep = torch.from_numpy(keep.astype(np.uint8) * 7 if as_u8 else keep).to(DEV)
    sel, unscored = objects.select(res, dev_keep)
    got = (sel.labels, sel.table, sel.kept, sel.mask.view(torch.uint8), unscored)
    for g, w, name in zip(got, want, ("labels", "table", "kept", "mask", "unscored")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert sel.mask.dtype == torch.bool and sel.found is res.found
    assert unscored.tolist() == [2048 - 64, 0, 0, 0, 0]
    if which == "all":                                         # only the labels above K go
        np.testing.assert_array_equal(sel.labels.cpu().numpy(), np.where(labels <= 64, labels, 0))
        assert sel.kept.tolist() == [64, 0, 1, 63, 64]
    if which == "none":
        assert not sel.labels.any() and not sel.table.any() and sel.kept.tolist() == [0] * 5
    mine, theirs = objects.track(sel.labels, iou=0.3), objects.track(torch.from_numpy(want[0]).to(DEV), iou=0.3)
    for k in ("prev", "track", "n_tracks", "n_links", "n_objects", "longest", "table"):
        np.testing.assert_array_equal(getattr(mine, k).cpu().numpy(), getattr(theirs, k).cpu().numpy(), err_msg=k)


def test_select_takes_a_longer_table_and_smaller_frames(stack):
    _, labels, kept, _, _ = stack
    res = objects.label(torch.from_numpy(_masks()[:, :40, :33].copy()).to(DEV), connectivity=8, max_objects=256, want_labels=True)
    host = [t.cpu().numpy() for t in (res.labels, res.table, res.kept)]
    keep = np.random.default_rng(5).integers(0, 2, size=(5, 48)).astype(bool)
    want = ref.select(host[0], host[1], host[2], keep, K=48)
    sel, unscored = objects.select(res, torch.from_numpy(keep).to(DEV))
    for g, w in zip((sel.labels, sel.table, sel.kept, sel.mask.view(torch.uint8), unscored), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
