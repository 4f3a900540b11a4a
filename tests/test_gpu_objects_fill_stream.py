"""Filling a frame range of a window (cgs_objects_track_fill_window, objects.fill(frames=)) and filling a stack that comes in chunks
(objects.FillStream) on the GPU.  The expected value is objects.fill of the whole stack -- existing code, held once per stack against
tests/objects_track_fill_ref.py here -- and everything is integer: exact equality.  The stacks are tests/objects_fill_stream_ref.py's;
what a case needs of its input so that it cannot pass vacuously (new objects, a head in a later chunk, an old carried mask, a vanished
candidate) is asserted from the whole-stack result."""
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

import objects_fill_stream_ref as sref  # noqa: E402
import objects_track_fill_ref as ref  # noqa: E402
import temporal_motion_ref as tmref  # noqa: E402
from cgs_amd import objects, temporal  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K, IOU = 24, 64, 0.3
KEYS = ("labels", "track", "age", "table")
STACKS = {"17x23-s3": (17, 23, 3, None), "17x23-s5": (17, 23, 5, None), "64x64-s3": (64, 64, 3, None),
          "64x64-s3-flow": (64, 64, 3, "flow"), "64x64-s3-zero": (64, 64, 3, "zero")}
GAPS = (1, 2, 8)


def _splits(G):
    return ([N], [1] * N, [5, 19], [23, 1], [3] * 8, [G, N - G])


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(labels int32 [24,h,w] on the device, bwd int8 [23,8,8,2] on the device or None)."""
    h, w, seed, field = STACKS[name]
    labels = torch.from_numpy(np.array(sref.stack(N, h, w, seed))).to(DEV)
    bwd = None
    if field == "flow":                                                   # a pan of one cell a frame, every cell its own colour
        low = torch.from_numpy(tmref.pan(N, 0, 1, 11, texture=True)[1]).to(DEV)
        bwd = temporal.flow(low, 2)[1]
        assert bool((bwd != 0).any())
    elif field == "zero":
        bwd = torch.zeros((N - 1, 8, 8, 2), dtype=torch.int8, device=DEV)
    return labels, bwd


def _host(fl):
    out = {k: getattr(fl, k).cpu().numpy() for k in KEYS}
    out["totals"] = torch.stack([fl.n_objects, fl.n_cells, fl.n_dropped, fl.n_vanished]).cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _whole(name, G):
    """objects.fill of the whole stack on the host, its tracks' prev / gap / track, and the per-frame totals; held against the
    checker once.  Never written afterwards."""
    labels, bwd = _inputs(name)
    tr = objects.track(labels, iou=IOU, max_objects=K, max_tracks=1, max_gap=G, motion=bwd)
    want = _host(objects.fill(labels, tr, motion=bwd, max_objects=K))
    host = {k: getattr(tr, k).cpu().numpy() for k in ("prev", "gap", "track")}
    field = None if bwd is None else bwd.cpu().numpy()
    check = ref.fill(labels.cpu().numpy(), field, host["prev"], host["gap"], host["track"], K, G)
    for key in KEYS + ("totals",):
        np.testing.assert_array_equal(want[key], check[key], err_msg=f"objects.fill against the checker: {key}")
    per_frame = sref.frame_totals(labels.cpu().numpy(), field, host["prev"], host["gap"], host["track"], K, G)
    np.testing.assert_array_equal(per_frame.sum(axis=0), check["totals"])
    for v in list(want.values()) + list(host.values()) + [per_frame]:
        v.setflags(write=False)
    return want, host, per_frame, tr


# ---------------------------------------------------------------- the window entry
@pytest.mark.parametrize("G", GAPS)
@pytest.mark.parametrize("name", ["64x64-s3", "64x64-s3-flow", "17x23-s5"])
def test_frame_range_is_the_slice_of_the_whole_stack(name, G):
    labels, bwd = _inputs(name)
    want, _host_tracks, per_frame, tr = _whole(name, G)
    assert want["totals"][0] > 0
    for f0, f1 in ((0, N), (0, 0), (N, N), (5, 6), (G, N - G), (N - 1, N)):
        got = _host(objects.fill(labels, tr, motion=bwd, max_objects=K, frames=(f0, f1)))
        for key in KEYS:
            assert got[key].shape[0] == f1 - f0
            np.testing.assert_array_equal(got[key], want[key][f0:f1], err_msg=f"{key} of frames {f0}..{f1} at G={G}")
        np.testing.assert_array_equal(got["totals"], per_frame[f0:f1].sum(axis=0), err_msg=f"totals of frames {f0}..{f1} at G={G}")
    fl = objects.fill(labels, tr, motion=bwd, max_objects=K, frames=(3, 20), want_table=False, want_rgb=True)
    assert fl.table is None and tuple(fl.rgb.shape) == (17,) + tuple(labels.shape[1:]) + (3,)
    np.testing.assert_array_equal(fl.rgb.cpu().numpy(), ref.paint(want["labels"][3:20], want["track"][3:20], K)[1])


# ---------------------------------------------------------------- the stream
def _run(name, G, sizes):
    labels, bwd = _inputs(name)
    fs = objects.FillStream(IOU, max_objects=K, max_gap=G, motion=bwd is not None)
    field = None if bwd is None else torch.cat((torch.zeros_like(bwd[:1]), bwd))         # row i: from frame i to the frame before it
    parts, counts, at = [], [], 0
    for m in sizes:
        out = fs.push(labels[at:at + m], *(() if field is None else (field[at:at + m],)))
        at += m
        assert out.labels.shape[0] == max(at - G, 0) - sum(counts)        # all frames pushed but the last G, less those returned
        parts.append(out)
        counts.append(int(out.labels.shape[0]))
    parts.append(fs.flush())
    assert sum(counts) + parts[-1].labels.shape[0] == N and parts[-1].labels.shape[0] == min(G, N)
    got = {k: np.concatenate([getattr(p, k).cpu().numpy() for p in parts]) for k in KEYS}
    got["totals"] = np.sum([torch.stack([p.n_objects, p.n_cells, p.n_dropped, p.n_vanished]).cpu().numpy() for p in parts], axis=0)
    return got, fs


@pytest.mark.parametrize("G", GAPS)
@pytest.mark.parametrize("name", list(STACKS))
def test_every_split_gives_the_whole_stack(name, G):
    want, host, _per_frame, tr = _whole(name, G)
    totals = want["totals"]
    print(f"{name} G={G}: totals {totals.tolist()}, max age {int(want['age'].max())}")
    assert totals[0] > 0                                                  # new objects at every G
    if G == 8 and name.startswith("64x64"):
        assert want["age"].max() >= 4
    if G == 8 and name == "17x23-s5":
        assert totals[3] > 0                                              # a carried mask that found the bar in its place
    for sizes in _splits(G):
        if sizes in ([1] * N, [3] * 8):                                   # a filled frame whose link ends in a chunk not yet pushed
            assert sref.heads_in_later_chunks(want["age"], host["gap"], want["track"], sizes) > 0
        got, fs = _run(name, G, sizes)
        for key in KEYS + ("totals",):
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} for the split {sizes} at G={G}")
        np.testing.assert_array_equal(fs.totals.cpu().numpy(), want["totals"])
        assert int(fs.n_tracks) == int(tr.n_tracks)
        with pytest.raises(ValueError, match="flushed"):
            fs.flush()
        with pytest.raises(ValueError, match="flushed"):
            fs.push(_inputs(name)[0][:1])


def test_streams_shorter_than_the_gap():
    """Fewer frames than G + 1, pushed one by one: push returns nothing, flush everything."""
    labels, _ = _inputs("17x23-s3")
    for n, G in ((1, 1), (2, 8), (8, 8), (9, 8)):
        stack = labels[:n]
        tr = objects.track(stack, iou=IOU, max_objects=K, max_tracks=1, max_gap=G)
        want = _host(objects.fill(stack, tr, max_objects=K))
        fs = objects.FillStream(IOU, max_objects=K, max_gap=G)
        parts = [fs.push(stack[i:i + 1]) for i in range(n)] + [fs.flush()]
        assert [int(p.labels.shape[0]) for p in parts] == [0] * min(n, G) + [1] * (n - min(n, G)) + [min(n, G)]
        for key in KEYS:
            np.testing.assert_array_equal(np.concatenate([getattr(p, key).cpu().numpy() for p in parts]), want[key], err_msg=f"{key} n={n} G={G}")
        np.testing.assert_array_equal(fs.totals.cpu().numpy(), want["totals"])
