"""Motion-compensated tracking on the GPU (cgs_objects_track_mc, cgs_amd.objects.track(motion=), TrackStream(motion=True),
--track-motion, --overlay-motion) against the frame-pair walk of tests/objects_track_mc_ref.py.  Everything is integer: exact equality
everywhere.  The hand-made cases state their expected arrays; the checker must agree with them before the kernels are asked
(tests/test_objects_track_mc_host.py runs them with the checker in the kernels' place)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_track_gap_ref as gap_ref  # noqa: E402
import objects_track_mc_ref as ref  # noqa: E402
import objects_track_ref as base  # noqa: E402
import temporal_motion_ref as flow_ref  # noqa: E402
from cgs_amd import _lib, cli, fit, handler, objects, process, temporal  # noqa: E402
from test_gpu_objects_track_gap import JUNK, KEYS, _files, _run, _same, videodir, workdir  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIDE = 64


def _up(a, dtype=np.int32):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _field(n, vector=(0, 0)):
    """A constant backward field for n frames."""
    f = np.zeros((max(n - 1, 0), 8, 8, 2), dtype=np.int8)
    f[...] = vector
    return f


def _gpu(labels, bwd, milli, K=64, G=0, max_tracks=None, paint=True):
    """objects.track(motion=bwd) on a stack, back on the host in the checker's form; bwd None: no motion (then G = 0 has no gap keys)."""
    motion = None if bwd is None else _up(bwd, np.int8)
    res = objects.track(_up(labels), iou=milli / 1000, max_objects=K, max_tracks=max_tracks, want_labels=paint, want_rgb=paint, max_gap=G,
                        motion=motion)
    torch.cuda.synchronize()
    n = res.prev.shape[0]
    rows = n * K if max_tracks is None else max_tracks
    assert res.prev.shape == res.track.shape == (n, K) and res.table.shape == (rows, 8)
    out = {"prev": res.prev, "track": res.track, "table": res.table, "totals": torch.stack(res[2:6])}
    if motion is not None or G:
        assert res.gap.shape == (n, K) and res.extra.shape == (rows, 2) and res.gap_links.shape == (G + 1,)
        out.update(gap=res.gap, gap_links=res.gap_links, extra=res.extra)
    if paint:
        out["track_labels"], out["rgb"] = res.track_labels, res.rgb
    assert all(t.dtype == (torch.uint8 if k == "rgb" else torch.int32) and t.is_cuda for k, t in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(labels, bwd, milli, K=64, G=0, max_tracks=None):
    labels = np.asarray(labels)
    want = ref.track(labels, bwd, milli, K, G, max_tracks, want_paint=True)
    _same(_gpu(labels, bwd, milli, K, G, max_tracks), want, f"milli={milli} K={K} G={G}")
    return want


def _raw(labels, bwd, milli, K, G, max_tracks=None, tracks=True, extra=True, painted=True, rgb=True):
    """cgs_objects_track_mc itself on outputs full of junk; what was not asked for stays junk."""
    labels, bwd = _up(labels), _up(bwd, np.int8)
    n, h, w = (int(s) for s in labels.shape)
    max_tracks = n * K if max_tracks is None else max_tracks
    need = int(_lib.load().cgs_objects_track_mc_scratch_bytes(n, K, G))
    full = lambda *shape, dtype=torch.int32: torch.full(shape, JUNK, dtype=dtype, device=DEV)
    o = {"prev": full(n, K), "gap": full(n, K), "track": full(n, K), "totals": full(4), "gap_links": full(G + 1), "table": full(max_tracks, 8),
         "extra": full(max_tracks, 2), "track_labels": full(n, h, w), "rgb": full(n, h, w, 3, dtype=torch.uint8)}
    scratch = torch.full((need // 8 + 1,), -1, dtype=torch.int64, device=DEV)
    ptr = lambda key, on=True: o[key].data_ptr() if on else None
    _lib.call("cgs_objects_track_mc", labels.data_ptr(), bwd.data_ptr() if n > 1 else None, n, h, w, K, milli, G, max_tracks, ptr("prev"),
              ptr("gap"), ptr("track"), ptr("totals"), ptr("gap_links"), ptr("table", tracks), ptr("extra", extra),
              ptr("track_labels", painted), ptr("rgb", rgb), scratch.data_ptr(), scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---------------------------------------------------------------- the stacks
@functools.lru_cache(maxsize=None)
def _blobs(n, seed=0, junk=True):
    """n frames of 64 x 64: one 8 x 8 blob per cell of an 8 x 8 grid, shifted by -1..1 cells (so block borders cut it) and absent from a
    third of the frames; the labels are permuted in one frame of four; frame 1 holds all 64 objects, frame 4 none; a few cells carry
    labels that are no objects: negative, above every cap, 0x7fffffff."""
    rs = np.random.RandomState(1000 * seed + n)
    s = np.zeros((n, SIDE + 2, SIDE + 2), dtype=np.int32)
    for f in range(n):
        perm = rs.permutation(64) if f % 4 == 3 else np.arange(64)
        for i in range(64):
            gone = rs.rand() < 1 / 3
            dy, dx = rs.randint(-1, 2), rs.randint(-1, 2)
            if (gone and f != 1) or f == 4:
                continue
            y, x = 1 + (i // 8) * 8 + dy, 1 + (i % 8) * 8 + dx
            s[f, y:y + 8, x:x + 8] = perm[i] + 1
    s = s[:, 1:-1, 1:-1].copy()
    if junk:
        r = rs.rand(n, SIDE, SIDE)
        s[r < 0.02] = 70
        s[(r >= 0.02) & (r < 0.03)] = -3
        s[(r >= 0.03) & (r < 0.04)] = 0x7FFFFFFF
    s.setflags(write=False)
    return s


def _random_field(n, seed, full):
    rs = np.random.RandomState(seed)
    return (rs.randint(-128, 128, (n - 1, 8, 8, 2)) if full else rs.randint(-4, 5, (n - 1, 8, 8, 2))).astype(np.int8)


def _square(n, y, x, step, side=5, present=None):
    """An object of side x side cells that moves `step` cells a frame along x; present: the frames that show it."""
    s = np.zeros((n, SIDE, SIDE), dtype=np.int32)
    for f in range(n):
        if present is None or f in present:
            s[f, y:y + side, x + f * step:x + f * step + side] = 1
    return s


# ---------------------------------------------------------------- 1. a zero field is the old tracker
@pytest.mark.parametrize("K", [64, 5])
@pytest.mark.parametrize("G", [0, 1, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 18])
def test_zero_field_is_the_old_tracker_bit_for_bit(n, G, K):
    s = _blobs(n)
    new = _raw(s, _field(n), 300, K, G)
    old = objects.track(_up(s), iou=0.3, max_objects=K, want_labels=True, want_rgb=True, max_gap=G)
    torch.cuda.synchronize()
    for key, t in (("prev", old.prev), ("track", old.track), ("table", old.table), ("track_labels", old.track_labels), ("rgb", old.rgb),
                   ("totals", torch.stack(old[2:6]))):
        np.testing.assert_array_equal(new[key], t.cpu().numpy(), err_msg=key)
    if G:
        for key, t in (("gap", old.gap), ("gap_links", old.gap_links), ("extra", old.extra)):
            np.testing.assert_array_equal(new[key], t.cpu().numpy(), err_msg=key)
    else:                                                                   # cgs_objects_track plus gap = prev > 0
        assert old.gap is None
        np.testing.assert_array_equal(new["gap"], (new["prev"] > 0).astype(np.int32))
        assert new["gap_links"].tolist() == [int(new["totals"][1])] and not new["extra"].any()
    if n == 18:
        assert new["totals"][1] > 0 and (K == 5 or new["totals"][2] > 600)
        _same({k: new[k] for k in KEYS}, gap_ref.track(s, 300, K, G))


# ---------------------------------------------------------------- 2. a pan that breaks the old tracker
PAN_N = 12


def test_a_pan_that_breaks_the_old_tracker():
    n = PAN_N
    s = _square(n, 20, 6, 3)                                                # 5 x 5, 3 cells a frame: 10 / 40 between neighbours
    assert base.links(s[0], s[1], 250, 64) == {1: (1, 10, 40)}
    still = _gpu(s, None, 300)
    assert still["totals"].tolist() == [n, 0, n, 1] and not still["prev"].any() and still["track"][:, 0].tolist() == list(range(1, n + 1))
    want = _check(s, _field(n, (0, -3)), 300)
    prev = np.zeros((n, 64), dtype=np.int32)
    prev[1:, 0] = 1
    track = np.zeros((n, 64), dtype=np.int32)
    track[:, 0] = 1
    np.testing.assert_array_equal(want["prev"], prev)
    np.testing.assert_array_equal(want["gap"], prev)
    np.testing.assert_array_equal(want["track"], track)
    assert want["totals"].tolist() == [1, n - 1, n, n] and want["gap_links"].tolist() == [n - 1] and not want["extra"].any()
    assert want["table"][0].tolist() == [0, 1, n, 25 * n, 25, 25, 25 * (n - 1), 25 * (n - 1)] and not want["table"][1:].any()
    np.testing.assert_array_equal(want["track_labels"], s)
    assert objects.track_rows(want["table"], 1)[0]["link_iou"] == 1.0
    assert _check(s, _field(n, (0, -2)), 300)["totals"].tolist() == [1, n - 1, n, n]       # a cell short: 20 / 30
    assert _check(s, _field(n, (0, -2)), 667)["totals"].tolist() == [n, 0, n, 1]
    assert _check(s, _field(n, (0, 3)), 300)["totals"].tolist() == [n, 0, n, 1]            # the wrong way


# ---------------------------------------------------------------- 3. end to end with the real vectors
def _glued(n=8, step=3, seed=5):
    """(low uint8 [n,64,64,3], labels int32 [n,64,64]): a random texture that pans `step` cells a frame along x and a 5 x 5 object glued
    to it, in interior blocks and cut by a block border."""
    rs = np.random.RandomState(seed)
    canvas = rs.randint(0, 256, (SIDE, SIDE + step * n, 3)).astype(np.uint8)
    marks = np.zeros((SIDE, SIDE + step * n), dtype=np.int32)
    off = step * (n - 1)
    marks[21:26, off + 16:off + 21] = 1                                     # frame 0: rows 21..25, columns 16..20
    low = np.stack([canvas[:, off - step * g:off - step * g + SIDE] for g in range(n)])
    labels = np.stack([marks[:, off - step * g:off - step * g + SIDE] for g in range(n)])
    return low, labels


def test_end_to_end_with_the_real_vectors():
    low, labels = _glued()
    n = len(low)
    np.testing.assert_array_equal(labels, _square(n, 21, 16, 3))
    fwd, bwd = temporal.flow(_up(low, np.uint8), 4)
    torch.cuda.synchronize()
    got = bwd.cpu().numpy()
    assert (got[:, :, 1:] == np.array([0, -3], dtype=np.int8)).all()       # the premise: every block that can look 3 cells left
    np.testing.assert_array_equal(got, flow_ref.flow_ref(low, 4)[1])
    assert _gpu(labels, None, 300)["totals"].tolist() == [n, 0, n, 1]
    want = _check(labels, got, 300)
    assert want["totals"].tolist() == [1, n - 1, n, n] and want["table"][0].tolist() == [0, 1, n, 25 * n, 25, 25, 25 * (n - 1), 25 * (n - 1)]
    pair = objects.track(_up(labels), iou=0.3, motion=(fwd, bwd))           # the pair as temporal.flow returns it
    assert int(pair.n_tracks) == 1 and int(pair.longest) == n


# ---------------------------------------------------------------- 4. the carried area decides
def test_carried_area_decides():
    s = np.zeros((2, SIDE, SIDE), dtype=np.int32)
    s[0, 10:14, 0:4] = 1                                                    # 4 x 4 at the left edge
    s[1, 10:14, 0:2] = 1                                                    # two cells further left: half of it is still seen
    bwd = _field(2)
    bwd[0, :, 0] = (0, 2)
    assert int(ref.carried(s[0], bwd, 0, 1, 64).sum()) == 8
    want = _check(s, bwd, 600)
    assert want["prev"][1, 0] == 1 and want["totals"].tolist() == [1, 1, 2, 2]
    assert want["table"][0].tolist() == [0, 1, 2, 24, 8, 16, 8, 8]         # the areas are the objects' own: 16 and 8
    assert _check(s, bwd, 1000)["totals"][0] == 1
    still = _gpu(s, None, 600)
    assert still["totals"].tolist() == [2, 0, 2, 1]                        # 8 / 16 without motion
    assert _gpu(s, None, 500)["table"][0].tolist() == [0, 1, 2, 24, 8, 16, 8, 16]


# ---------------------------------------------------------------- 5. gap and pan together
def test_gap_and_pan_together():
    s = _square(4, 16, 8, 2, present=(0, 3))                               # columns 8..12 in frame 0, 14..18 in frame 3, rows 16..20
    bwd = _field(4)
    bwd[2, 2, 1:3] = bwd[1, 2, 1:3] = bwd[0, 2, 1] = (0, -2)               # the chain 14..18 -> 12..16 -> 10..14 -> 8..12 crosses a block border
    assert ref.offset(bwd, 0, 3, 16, 18) == (0, -6) and ref.offset(bwd, 0, 3, 16, 20) == (0, -4) and ref.offset(bwd, 0, 3, 40, 18) == (0, 0)
    np.testing.assert_array_equal(ref.carried(s[0], bwd, 0, 3, 64), s[3])
    want = _check(s, bwd, 500, G=2)
    prev = np.zeros((4, 64), dtype=np.int32)
    prev[3, 0] = 1
    track = np.zeros((4, 64), dtype=np.int32)
    track[[0, 3], 0] = 1
    np.testing.assert_array_equal(want["prev"], prev)
    np.testing.assert_array_equal(want["gap"], 3 * prev)
    np.testing.assert_array_equal(want["track"], track)
    assert want["totals"].tolist() == [1, 1, 2, 4] and want["gap_links"].tolist() == [0, 0, 1]
    assert want["extra"][0].tolist() == [1, 2] and not want["extra"][1:].any()
    assert want["table"][0].tolist() == [0, 1, 2, 50, 25, 25, 25, 25]
    assert _check(s, bwd, 500, G=1)["totals"].tolist() == [2, 0, 2, 1]     # three frames back is beyond G = 1
    flat = _gpu(s, None, 500, G=2)
    assert flat["totals"].tolist() == [2, 0, 2, 1] and flat["gap_links"].tolist() == [0, 0, 0]


# ---------------------------------------------------------------- 6. random fields against the checker
@pytest.mark.parametrize("full", [False, True], ids=["within4", "int8"])
@pytest.mark.parametrize("milli", [1, 300, 500, 1000])
@pytest.mark.parametrize("G", [0, 1, 3, 8])
def test_random_fields(G, milli, full):
    linked = 0
    for n in sorted({2, 3, G + 2, 12}):
        s, bwd = _blobs(n, seed=1), _random_field(n, 31 * n + G, full)
        want = _check(s, bwd, milli, G=G)
        linked += int(want["totals"][1])
        if n == 12:
            assert s.max() == 0x7FFFFFFF and s.min() == -3 and len(np.unique(s[1])) >= 65 and not ((s[4] >= 1) & (s[4] <= 64)).any()
            _check(s, bwd, milli, K=5, G=G)
            if not full and milli == 1:
                assert want["gap_links"][:min(G, 3) + 1].all()              # links of every short gap
    assert linked > 0 or milli == 1000


# ---------------------------------------------------------------- 7. output options and argument errors
def test_output_options():
    n, K, G = 12, 64, 3
    s, bwd = _blobs(n, seed=1), _random_field(n, 7, False)
    want = ref.track(s, bwd, 300, K, G, want_paint=True)
    count = int(want["totals"][0])
    assert count > 100 and want["extra"][:100].any()
    cut = _check(s, bwd, 300, K=K, G=G, max_tracks=100)                     # max_tracks below the track count
    assert cut["totals"][0] == count and cut["track"].max() == count and cut["table"].shape == (100, 8)
    np.testing.assert_array_equal(cut["table"], want["table"][:100])
    np.testing.assert_array_equal(cut["extra"], want["extra"][:100])
    for off in ("tracks", "extra", "painted", "rgb"):
        got = _raw(s, bwd, 300, K, G, **{off: False})
        junk = {"tracks": "table", "extra": "extra", "painted": "track_labels", "rgb": "rgb"}[off]
        assert (got.pop(junk) == JUNK).all(), off
        _same({k: v for k, v in got.items() if k in KEYS}, want, f"without {off}")
        if "track_labels" in got:
            np.testing.assert_array_equal(got["track_labels"], want["track_labels"])
        if "rgb" in got:
            np.testing.assert_array_equal(got["rgb"], base.colours(want["track_labels"]))


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    for n, K, G in ((1, 1, 0), (5, 64, 8), (7, 3, 2)):
        assert lib.cgs_objects_track_mc_scratch_bytes(n, K, G) == lib.cgs_objects_track_gap_scratch_bytes(n, K, G) > 0
    assert lib.cgs_objects_track_mc_scratch_bytes(5, 4, 9) == 0 and lib.cgs_objects_track_mc_scratch_bytes(0, 4, 1) == 0
    n, K = 5, 4
    stack = _square(n, 20, 6, 3)
    labels, field = _up(stack), _up(_field(n, (0, -3)), np.int8)
    full = lambda *shape, dtype=torch.int32: torch.full(shape, JUNK, dtype=dtype, device=DEV)
    outs = {"prev": full(n, K), "gap": full(n, K), "track": full(n, K), "totals": full(4), "gap_links": full(9 + 1), "tracks": full(n * K, 8),
            "extra": full(n * K, 2), "painted": full(n, SIDE, SIDE), "rgb": full(n, SIDE, SIDE, 3, dtype=torch.uint8)}
    need = int(lib.cgs_objects_track_mc_scratch_bytes(n, K, 8))
    scratch = torch.full((need // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(G=2, bytes_=need, shift=None, h=SIDE, w=SIDE, frames=n, **over):
        p = {k: v.data_ptr() for k, v in outs.items()}
        p.update(labels=labels.data_ptr(), bwd=field.data_ptr(), scratch=scratch.data_ptr())
        if shift:
            p[shift] += 2 if shift != "scratch" else 4
        p.update(over)
        return lib.cgs_objects_track_mc(p["labels"], p["bwd"], frames, h, w, K, 500, G, n * K, p["prev"], p["gap"], p["track"], p["totals"],
                                        p["gap_links"], p["tracks"], p["extra"], p["painted"], p["rgb"], p["scratch"], bytes_, stream)

    bad, unsupported = _lib.ERR_BADARG, _lib.ERR_UNSUPPORTED
    assert call(G=-1) == bad and call(G=9) == bad and call(bwd=None) == bad
    assert call(bytes_=int(lib.cgs_objects_track_mc_scratch_bytes(n, K, 2)) - 1) == bad
    assert call(h=32) == unsupported and call(w=32) == unsupported and call(h=63, w=63) == unsupported and call(h=0) == bad
    for name in ("labels", "prev", "gap", "track", "totals", "gap_links", "tracks", "extra", "painted", "scratch"):
        assert call(shift=name) == bad, name
    for name in ("labels", "prev", "gap", "track", "totals", "gap_links", "scratch"):
        assert call(**{name: None}) == bad, name
    torch.cuda.synchronize()
    assert all((v == JUNK).all() for v in outs.values()) and (scratch == -1).all()
    assert call(frames=1, bwd=None) == 0                                    # one frame reads no vector
    torch.cuda.synchronize()
    assert outs["track"][0].tolist() == [1, 0, 0, 0] and (outs["track"][1:] == JUNK).all()
    assert call() == 0                                                      # and the call with nothing wrong runs
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs["track"].cpu().numpy(), ref.track(stack, _field(n, (0, -3)), 500, K, 2)["track"])
    assert outs["track"][:, 0].tolist() == [1] * n
    a = _up(np.zeros((3, 32, 32)))
    with pytest.raises(ValueError, match="64 x 64"):
        objects.track(a, motion=field[:2])
    for wrong in (field[:3], field[:4].to(torch.int32), field[:4].cpu(), (field[:4],)):
        with pytest.raises(ValueError, match="motion"):
            objects.track(labels, motion=wrong)


# ---------------------------------------------------------------- 8. TrackStream(motion=True)
SPLITS = ([10], [1] * 10, [3, 3, 3, 1], [1, 9], [9, 1], [4, 6], [2, 5, 3], [3, 1, 1, 5])


@pytest.mark.parametrize("G", [0, 2])
def test_track_stream_with_motion(G):
    n = 10
    s, bwd = _blobs(n, seed=2), _random_field(n, 11, False)
    whole = _check(s, bwd, 300, G=G)
    n_tracks = int(whole["totals"][0])
    assert whole["totals"][1] > 20 and n_tracks > 64 and (G == 0 or whole["gap_links"][1:].sum() > 2)
    assert not np.array_equal(whole["track"], gap_ref.track(s, 300, 64, G)["track"])       # the field matters
    dev = _up(s)
    rows = _up(np.concatenate([np.full((1, 8, 8, 2), 99), bwd]), np.int8)   # row i: from frame i to frame i - 1; row 0 is never read
    got = []
    for split in SPLITS:
        assert sum(split) == n
        ts = objects.TrackStream(0.3, max_gap=G, motion=True)
        parts, lo = [], 0
        for m in split:
            ids = ts.push(dev[lo:lo + m], rows[lo:lo + m])
            assert ids.dtype == torch.int32 and tuple(ids.shape) == (m, 64) and ids.is_cuda
            parts.append(ids)
            lo += m
        got.append((split, torch.cat(parts), ts.n_tracks))
    for split, ids, count in got:                                           # (read back after the last push: the stream never waits)
        np.testing.assert_array_equal(ids.cpu().numpy(), whole["track"], err_msg=f"G={G} split {split}")
        assert int(count) == n_tracks
    ts = objects.TrackStream(0.3, motion=True)
    with pytest.raises(ValueError, match="bwd"):
        ts.push(dev[:2])
    with pytest.raises(ValueError, match="bwd"):
        ts.push(dev[:2], rows[:3])
    with pytest.raises(ValueError, match="bwd"):
        objects.TrackStream(0.3).push(dev[:2], rows[:2])


# ---------------------------------------------------------------- 9. end to end
def _report_side(t, kept, G):
    more = {"max_gap": G, "gap_links": t["gap_links"], "missed": int(t["extra"][:, 1].sum())} if G else {}
    return objects.track_report(t["totals"], t["table"][:, 2], int(t["table"][:, 6].astype(np.int64).sum()),
                                int(t["table"][:, 7].astype(np.int64).sum()), int(np.maximum(kept - 64, 0).sum()), **more)


def test_cli_process_track_motion(workdir, capsys, monkeypatch):
    """-process -objects --track-iou 0.3 --track-motion 4 on a folder of panning PNGs.  The network's masks are replaced by the object
    glued to the texture (the masks of the golden weights follow no pan): the flag, the file bytes in natural order of the names, the
    vectors, the tracker and tracks.json are the code under test."""
    from PIL import Image
    low, labels = _glued()
    n = len(low)
    os.makedirs("S")
    stems = [f"f{k}" for k in (1, 2, 3, 10, 11, 12, 20, 100)]
    for stem, frame in zip(stems, low):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    index = {frame.tobytes(): i for i, frame in enumerate(low)}

    def masks(self, X, to_device, progress, **kw):
        order = [index[np.round(np.asarray(x) * 255).astype(np.uint8).tobytes()] for x in X]
        return np.zeros(len(X), dtype=np.float32), (labels[order] > 0).astype(np.float32)[:, None], None
    monkeypatch.setattr(handler.Handler, "_sweep_masks", masks)
    common = ["-process", "--source-imgs", "S", "-objects", "--track-iou", "0.3"]
    _run(common + ["--mask-output-imgs", "R0"], capsys)
    _run(common + ["--mask-output-imgs", "RZ", "--track-motion", "0"], capsys)
    _run(common + ["--mask-output-imgs", "R4", "--track-motion", "4"], capsys)
    r0, rz, r4 = _files("R0"), _files("RZ"), _files("R4")
    assert r0 == rz and set(r4) == set(r0) and all(r4[f] == r0[f] for f in r0 if "tracks" not in f)
    flat, moved = json.loads(r0["tracks.json"]), json.loads(r4["tracks.json"])
    assert flat["summary"]["tracks"] == n and "track_motion" not in flat and "motion" not in str(flat)
    bwd = temporal.flow(_up(low, np.uint8), 4)[1].cpu().numpy()
    want = ref.track(labels, bwd, 300)
    assert want["totals"].tolist() == [1, n - 1, n, n]
    assert moved["summary"] == _report_side(want, np.ones(n, dtype=np.int64), 0) and moved["summary"]["tracks"] == 1
    assert moved["track_motion"] == objects.motion_report(bwd, 4) and moved["track_motion"]["search"] == 4 and moved["track_motion"]["block"] == 8
    assert abs(moved["track_motion"]["mean_cells_per_frame"] - 3.0) < 0.5 and moved["order"] == stems
    assert [k for k in moved if k not in flat] == ["track_motion"] and list(moved["summary"]) == list(flat["summary"])
    assert moved["frames"] == {s: [{"label": 1, "track": 1, "prev": int(j > 0)}] for j, s in enumerate(stems)}
    assert moved["tracks"] == [{"track": 1, "first": "f1", "last": "f100", "length": n, "area_sum": 25 * n, "area_min": 25, "area_max": 25,
                                "link_iou": 1.0}]
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R4", f"{s}-tracks-mask.png"))), base.colours(labels[j]))


def test_cli_process_fit_track_motion(workdir, capsys, monkeypatch):
    """The same under -fit on frames of 128 x 128: the vectors come from the shrunk frames (fit.down of a frame doubled in both
    directions is the frame), in natural order of the names.  The network's masks are replaced as above."""
    from PIL import Image
    low, labels = _glued()
    n = len(low)
    os.makedirs("S")
    stems = [f"f{k}" for k in (1, 2, 3, 10, 11, 12, 20, 100)]
    for stem, frame in zip(stems, low):
        Image.fromarray(np.repeat(np.repeat(frame, 2, axis=0), 2, axis=1)).save(os.path.join("S", stem + ".png"))
    index = {frame.tobytes(): i for i, frame in enumerate(low)}

    def masks(eng, shrunk, unit, fp16, train_mode):
        order = [index[x.tobytes()] for x in shrunk.cpu().numpy()]
        return torch.from_numpy((labels[order] > 0).astype(np.float32)).to(shrunk.device)
    monkeypatch.setattr(process, "fit_infer", masks)
    common = ["-process", "-fit", "--source-imgs", "S", "-objects", "--track-iou", "0.3"]
    _run(common + ["--mask-output-imgs", "R0"], capsys)
    _run(common + ["--mask-output-imgs", "R4", "--track-motion", "4"], capsys)
    r0, r4 = _files("R0"), _files("R4")
    assert set(r4) == set(r0) and all(r4[f] == r0[f] for f in r0 if "tracks" not in f)
    flat, moved = json.loads(r0["tracks.json"]), json.loads(r4["tracks.json"])
    bwd = temporal.flow(_up(low, np.uint8), 4)[1].cpu().numpy()
    assert flat["summary"]["tracks"] == n and "track_motion" not in flat and moved["summary"]["tracks"] == 1 and moved["order"] == stems
    assert moved["track_motion"] == objects.motion_report(bwd, 4) and moved["summary"]["link_iou"] == 1.0


def test_cli_eval_track_motion(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    read = lambda: open(os.path.join(root, "m", "eval_tracks.json"), "rb").read()
    line = lambda text: [ln for ln in text.split("\n") if ln.startswith("TRACKS")]
    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4", "--match-iou", "0.5", "--track-iou", "0.3"]
    _, plain = _run(common, capsys)
    plain_json = read()
    _, zero = _run(common + ["--track-motion", "0"], capsys)
    assert read() == plain_json and line(zero) == line(plain) and b"motion" not in plain_json and "motion" not in line(plain)[0]

    bwd = temporal.flow(_up(frames, np.uint8), 2)[1]
    sides = {}
    for G in (0, 1):
        for name, src, kw in (("truth", _up(truth, bool), dict(min_area=1)), ("pred", _up(M[:, 0], np.float32), dict(thresh=thr, min_area=4))):
            res = objects.label(src, connectivity=8, max_objects=64, **kw)
            tr = objects.track(res.labels, iou=0.3, max_gap=G, motion=bwd)
            t = {"totals": torch.stack(tr[2:6]).cpu().numpy(), "table": tr.table.cpu().numpy(), "gap_links": tr.gap_links.cpu().numpy(),
                 "extra": tr.extra.cpu().numpy()}
            sides[G, name] = {**_report_side(t, res.kept.cpu().numpy().astype(np.int64), G), "track_motion": objects.motion_report(bwd, 2)}
    H1, out = _run(common + ["--track-motion", "2"], capsys)
    rep = json.loads(read())
    p, t = sides[0, "pred"], sides[0, "truth"]
    assert rep == H1.tracks and rep["truth"] == t and rep["mask"]["pred"] == p and list(p)[-1] == "track_motion"
    assert sorted(p["track_motion"]) == ["block", "mean_cells_per_frame", "saturated", "search"] and p["track_motion"]["search"] == 2
    assert [k for k in rep] == [k for k in json.loads(plain_json)] and "fragments" not in rep["mask"]["switches"][0]
    assert line(out) == [f"TRACKS conn=8 min_area=4 iou>=0.3 motion<=2: {p['tracks']} tracks over {p['objects']} objects, mean length "
                         f"{p['mean_length']:.6f}, longest {p['max_length']}; truth {t['tracks']} tracks over {t['objects']} objects"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]
    H2, out = _run(common + ["--track-motion", "2", "--track-gap", "1"], capsys)
    rep = json.loads(read())
    assert rep["truth"] == sides[1, "truth"] and rep["mask"]["pred"] == sides[1, "pred"] and "fragments" in rep["mask"]["switches"][0]
    assert " gap<=1 motion<=2: " in line(out)[0]


def _video(argv, results):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-video", "in.raw", "--overlay-video", "out.mp4",
                                        "--mask-output-imgs", results, "--overlay-tracks", "0.3"] + argv))
    assert H.load_models()
    return H.segment(folder=H.args.source_imgs)


def test_video_overlay_motion(videodir, monkeypatch, golden):
    n, calls = videodir
    sent = lambda i: np.fromfile(os.path.join(calls, f"{i}.stdin"), dtype=np.uint8)
    M = _video([], "R0")
    _video(["--overlay-motion", "0"], "RZ")
    assert _files("R0") == _files("RZ")                                    # without the flag, and at 0: today's files and frames
    np.testing.assert_array_equal(sent(0), sent(1))
    M1 = _video(["--overlay-motion", "2", "--overlay-gap", "1"], "R1")
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    M3 = _video(["--overlay-motion", "2", "--overlay-gap", "1"], "R3")
    assert n > 3
    np.testing.assert_array_equal(M1, M)
    np.testing.assert_array_equal(M3, M)
    np.testing.assert_array_equal(sent(2), sent(3))                        # one chunk and chunks of 3: the same numbers drawn
    r1, r3 = _files("R1"), _files("R3")
    assert r1 == r3 and set(r1) == {"out.json", "out-objects.json", "out-tracks.json"} and r1["out-objects.json"] == _files("R0")["out-objects.json"]
    g = golden("g6_process.npz")
    order = objects.natural_order([str(s) for s in g["names"]])
    big = np.repeat(np.repeat(g["frames"], 2, axis=1), 2, axis=2)[order]
    bwd = temporal.flow(fit.down(_up(big, np.uint8)), 2)[1]
    res = objects.label(_up(M[:, 0], np.float32), thresh=0.5, inclusive=True, connectivity=8, min_area=1, max_objects=64)
    tr = objects.track(res.labels, iou=0.3, max_gap=1, motion=bwd)
    track, gap = tr.track.cpu().numpy(), tr.gap.cpu().numpy()
    _same({"track": track, "gap": gap}, ref.track(res.labels.cpu().numpy(), bwd.cpu().numpy(), 300, 64, 1))
    rep = json.loads(r1["out-tracks.json"])
    assert rep["track_motion"] == objects.motion_report(bwd, 2) and rep["track_gap"] == 1 and rep["summary"]["tracks"] == int(tr.n_tracks)
    for i in range(n):
        assert {r["label"]: (r["track"], r["gap"]) for r in rep["frames"][f"{i:06d}"]} == {
            int(l) + 1: (int(track[i, l]), int(gap[i, l])) for l in np.flatnonzero(track[i])}
    info = json.loads(r1["out.json"])["tracks"]
    assert info["motion"] == 2 and info["gap"] == 1 and info["n_tracks"] == int(tr.n_tracks)
    assert "motion" not in json.loads(_files("R0")["out.json"])["tracks"] and "track_motion" not in json.loads(_files("R0")["out-tracks.json"])
