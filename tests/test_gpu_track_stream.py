"""objects.TrackStream on the GPU: for every split of a label stack into chunks the concatenated results of push are
objects.track(stack).track bit for bit, and n_tracks is the whole stack's.  The stacks are blobs that drift along lanes, appear,
vanish and change their label from frame to frame; the test checks on the whole-stack result that a track crosses a chunk boundary, that
one starts after a boundary and that a frame without objects lies at one, so that it cannot pass without having carried anything."""
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

from cgs_amd import _lib, objects  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (n, h, w, the frame without objects) and the splits of n
STACKS = {"64x64": ((37, 64, 64, 18), ([37], [1] * 37, [5, 32], [36, 1], [18, 1, 18])),
          "17x23": ((12, 17, 23, 6), ([12], [1] * 12, [5, 7], [11, 1], [6, 1, 5]))}


@functools.lru_cache(maxsize=None)
def _stack(n, h, w, empty):
    """int32 [n,h,w]: one blob per lane of rows, drifting by 0..5 cells a frame (wrapping), there or not from frame to frame; a frame's
    blobs are numbered 1.. from the top, so a blob's label changes when one above it comes or goes.  Lane 0 holds a slow blob up to the
    empty frame, lane 1 one from the frame after it to the end, and lane 2 a blob that is new in the last frame."""
    rs = np.random.RandomState(n * h + w)
    lanes = 6 if h >= 60 else 5
    lh, bw = h // lanes, max(w // 4, 2)
    s = np.zeros((n, h, w), dtype=np.int32)
    there = np.zeros((n, lanes), dtype=bool)
    x = np.zeros((n, lanes), dtype=np.int64)
    for lane in range(lanes):
        on, pos, v = rs.rand() < 0.5, rs.randint(w), int(rs.choice([0, 1, 2, 5]))
        for f in range(n):
            if rs.rand() < 0.15:
                on = not on
                if on:
                    pos, v = rs.randint(w), int(rs.choice([0, 1, 2, 5]))
            there[f, lane], x[f, lane] = on, pos
            pos += v
    there[:, 0], x[:, 0] = np.arange(n) < empty, np.arange(n)
    there[:, 1], x[:, 1] = np.arange(n) > empty, 3 + np.arange(n)
    there[n - 2, 2], there[n - 1, 2] = False, True
    there[empty] = False
    for f in range(n):
        for k, lane in enumerate(np.flatnonzero(there[f])):
            cols = (x[f, lane] + np.arange(bw)) % w
            s[f, lane * lh:(lane + 1) * lh, cols] = k + 1
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _whole(name, milli):
    dims, _ = STACKS[name]
    tr = objects.track(torch.from_numpy(_stack(*dims).copy()).to(DEV), iou=milli / 1000)
    return tr.track.cpu().numpy(), tr.prev.cpu().numpy(), int(tr.n_tracks)


@pytest.mark.parametrize("milli", [300, 600])
@pytest.mark.parametrize("name", sorted(STACKS))
def test_every_split_gives_the_whole_stacks_numbers(name, milli):
    dims, splits = STACKS[name]
    stack = _stack(*dims)
    want, prev, n_tracks = _whole(name, milli)
    assert n_tracks > 3 and want.max() == n_tracks
    for split in splits:
        assert sum(split) == dims[0]
        starts = np.cumsum(split)[:-1]                                    # the first frame of every chunk but the first
        if len(starts):                                                   # conditions on the input, read off the whole-stack result
            objs = want[starts] > 0
            if len(split) != 3:                                           # (both boundaries of the three-chunk splits lie at the empty frame)
                assert (objs & (prev[starts] > 0)).any(), f"{split}: no track crosses a boundary"
            assert any((want[b:] > 0)[prev[b:] == 0].any() for b in starts), f"{split}: no track starts after a boundary"
        if len(split) > 2:
            assert any(not stack[b].any() or not stack[b - 1].any() for b in starts), f"{split}: no empty frame at a boundary"
        ts = objects.TrackStream(milli / 1000)
        assert int(ts.n_tracks) == 0
        parts, lo = [], 0
        for m in split:
            ids = ts.push(torch.from_numpy(stack[lo:lo + m].copy()).to(DEV))
            assert ids.dtype == torch.int32 and tuple(ids.shape) == (m, 64) and ids.is_cuda
            parts.append(ids.cpu().numpy())
            lo += m
        np.testing.assert_array_equal(np.concatenate(parts), want, err_msg=f"{name} iou {milli} split {split}")
        assert int(ts.n_tracks) == n_tracks


def test_fewer_objects_than_the_cap_and_a_cap_that_cuts():
    """max_objects below the number of blobs: the objects above it are no objects, in the stream as in the whole stack."""
    dims, _ = STACKS["64x64"]
    stack = torch.from_numpy(_stack(*dims).copy()).to(DEV)
    assert int(stack.max()) > 2
    want = objects.track(stack, iou=0.3, max_objects=2)
    ts = objects.TrackStream(0.3, max_objects=2)
    got = torch.cat([ts.push(stack[lo:lo + 4]) for lo in range(0, dims[0], 4)])
    assert tuple(got.shape) == (dims[0], 2)
    np.testing.assert_array_equal(got.cpu().numpy(), want.track.cpu().numpy())
    assert int(ts.n_tracks) == int(want.n_tracks)


def test_refusals():
    ts = objects.TrackStream(0.5)
    a = torch.zeros((2, 17, 23), dtype=torch.int32, device=DEV)
    ts.push(a)
    for bad in (a[:, :16], a[:, :, :20], a.cpu(), a.long(), a[0], a[:0], "labels"):
        with pytest.raises(ValueError):
            ts.push(bad)
    with pytest.raises(ValueError, match="frames"):
        ts.push(torch.zeros((objects.TRACK_MAX_FRAMES, 1, 1), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="frames"):
        objects.TrackStream(0.5).push(torch.zeros((objects.TRACK_MAX_FRAMES, 1, 1), dtype=torch.int32, device=DEV))
    ts.push(a)                                                            # the refusals left the stream as it was
    assert int(ts.n_tracks) == 0
    for iou in (0, 1.5, 0.3333, "0.5"):
        with pytest.raises(ValueError):
            objects.TrackStream(iou)
    with pytest.raises(ValueError):
        objects.TrackStream(0.5, max_objects=65)
    with pytest.raises(_lib.CgsError):
        objects.TrackStream(0.5).push(a.cpu())                            # the first push is objects.track's: no CPU path
