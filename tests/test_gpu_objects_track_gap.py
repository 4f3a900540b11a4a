"""Tracking across gaps on the GPU (cgs_objects_track_gap, cgs_amd.objects.track(max_gap=G), TrackStream(max_gap=G), fragments,
--track-gap, --overlay-gap) against the level-order walk of tests/objects_track_gap_ref.py.  Everything is integer: exact equality
everywhere.  The hand-made cases state their expected arrays; the checker must agree with them before the kernels are asked."""
import functools
import itertools
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

import objects_ref  # noqa: E402
import objects_track_gap_ref as ref  # noqa: E402
import objects_track_ref as base  # noqa: E402
from cgs_amd import _lib, cli, handler, objects  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402
from test_gpu_process_video_tracks import FFMPEG, FFPROBE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 77


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.int32)).to(DEV)


def _gpu(labels, milli, K=64, G=1, max_tracks=None, paint=True):
    """objects.track(max_gap=G) on a stack, back on the host in the checker's form."""
    res = objects.track(_up(labels), iou=milli / 1000, max_objects=K, max_tracks=max_tracks, want_labels=paint, want_rgb=paint, max_gap=G)
    torch.cuda.synchronize()
    n = res.prev.shape[0]
    rows = n * K if max_tracks is None else max_tracks
    assert res.prev.shape == res.gap.shape == res.track.shape == (n, K) and res.table.shape == (rows, 8)
    assert res.extra.shape == (rows, 2) and res.gap_links.shape == (G + 1,)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in res[:7] + (res.gap, res.gap_links, res.extra))
    out = {"prev": res.prev, "gap": res.gap, "track": res.track, "table": res.table, "extra": res.extra, "gap_links": res.gap_links,
           "totals": torch.stack(res[2:6])}
    if paint:
        out["track_labels"], out["rgb"] = res.track_labels, res.rgb
    return {k: v.cpu().numpy() for k, v in out.items()}


KEYS = ("prev", "gap", "track", "totals", "gap_links", "table", "extra")


def _same(got, want, what=""):
    for key in KEYS:
        if key in got:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")
    if "track_labels" in got and "track_labels" in want:
        np.testing.assert_array_equal(got["track_labels"], want["track_labels"], err_msg=f"track_labels {what}")
        np.testing.assert_array_equal(got["rgb"], base.colours(want["track_labels"]), err_msg=f"rgb {what}")


def _check(labels, milli, K=64, G=1, max_tracks=None):
    labels = np.asarray(labels)
    want = ref.track(labels, milli, K, G, max_tracks, want_paint=True)
    _same(_gpu(labels, milli, K, G, max_tracks), want, f"milli={milli} K={K} G={G}")
    return want


def _raw(labels, milli, K, G, max_tracks=None, tracks=True, extra=True, painted=True, rgb=True, entry="cgs_objects_track_gap"):
    """The C entry itself on outputs full of junk; what was not asked for stays junk."""
    labels = _up(labels)
    n, h, w = (int(s) for s in labels.shape)
    max_tracks = n * K if max_tracks is None else max_tracks
    lib = _lib.load()
    gapped = entry == "cgs_objects_track_gap"
    need = int(lib.cgs_objects_track_gap_scratch_bytes(n, K, G)) if gapped else int(lib.cgs_objects_track_scratch_bytes(n, K))
    full = lambda *shape, dtype=torch.int32: torch.full(shape, JUNK, dtype=dtype, device=DEV)
    o = {"prev": full(n, K), "gap": full(n, K), "track": full(n, K), "totals": full(4), "gap_links": full(G + 1), "table": full(max_tracks, 8),
         "extra": full(max_tracks, 2), "track_labels": full(n, h, w), "rgb": full(n, h, w, 3, dtype=torch.uint8)}
    scratch = torch.full((need // 8 + 1,), -1, dtype=torch.int64, device=DEV)
    ptr = lambda key, on=True: o[key].data_ptr() if on else None
    tail = (ptr("track_labels", painted), ptr("rgb", rgb), scratch.data_ptr(), scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
    if gapped:
        _lib.call(entry, labels.data_ptr(), n, h, w, K, milli, G, max_tracks, ptr("prev"), ptr("gap"), ptr("track"), ptr("totals"),
                  ptr("gap_links"), ptr("table", tracks), ptr("extra", extra), *tail)
    else:
        _lib.call(entry, labels.data_ptr(), n, h, w, K, milli, max_tracks, ptr("prev"), ptr("track"), ptr("totals"), ptr("table", tracks), *tail)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---------------------------------------------------------------- the blinking stack of cases 1, 2 and 8
RUNS = (1, 9, 2, 8, 3, 7, 4, 6, 5)                                         # object 2's absences, one frame of presence between them


def _present(n):
    """Frames in which object 1 (absent on every third frame) and object 2 (absent for runs of 1..9 frames) exist."""
    two, f = [], 0
    for r in RUNS:
        two.append(f)
        f += 1 + r
    return [f for f in range(n) if f % 3 != 2], [f for f in two if f < n]


def _blink(n):
    s = np.zeros((n, 4, 4), dtype=np.int32)
    one, two = _present(n)
    s[one, 0] = 1
    s[two, 2, 1:] = 2
    return s


def _by_hand(n, G):
    """The blinking stack's figures from the frame lists alone: the objects never touch each other and never move, so an object links
    to its last appearance exactly when that is at most G + 1 frames back."""
    links, missed, spans, tracks = np.zeros(G + 1, dtype=np.int64), 0, [], 0
    for frames in _present(n):
        first = None
        for a, b in zip([None] + frames[:-1], frames):
            if a is not None and b - a <= G + 1:
                links[b - a - 1] += 1
                missed += b - a - 1
            else:
                tracks += 1
                first = b
            spans.append(b - first + 1)
    return tracks, links, missed, max(spans, default=0)


# ---------------------------------------------------------------- 1. max_gap = 0 is cgs_objects_track
@pytest.mark.parametrize("n", [1, 2, 3, 18])
def test_gap_zero_is_the_adjacent_tracker_bit_for_bit(n):
    s = _blink(n)
    old = _raw(s, 500, 3, 0, entry="cgs_objects_track")
    new = _raw(s, 500, 3, 0)
    for key in ("prev", "track", "totals", "table", "track_labels", "rgb"):
        np.testing.assert_array_equal(new[key], old[key], err_msg=key)
    _same({k: old[k] for k in ("prev", "track", "totals", "table")}, base.track(s, 500, 3))
    np.testing.assert_array_equal(new["gap"], (old["prev"] > 0).astype(np.int32))
    assert new["gap_links"].tolist() == [int(old["totals"][1])] and not new["extra"].any()
    assert (old["gap"] == JUNK).all() and (old["extra"] == JUNK).all()     # the old entry knows nothing of them


# ---------------------------------------------------------------- 2. a blinking object
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 10, 11, 17, 18, 33, 34])
def test_blinking_objects(n, G):
    want = _check(_blink(n), 500, K=3, G=G)
    tracks, links, missed, span = _by_hand(n, G)
    assert want["totals"].tolist() == [tracks, links.sum(), sum(len(p) for p in _present(n)), span]
    assert want["gap_links"].tolist() == links.tolist() and want["extra"][:, 1].sum() == missed
    assert want["extra"][:, 0].sum() == links[1:].sum() and max(want["spans"], default=0) == span
    if n >= 5:
        assert links[1] > 0 and missed > 0                                  # object 1 is bridged over every third frame
    if n == 34:
        # object 2 is in frames 0, 2, 12, 15, 24, 28: steps of 2, 10, 3, 9, 4; G bridges steps up to G + 1, the step of 10 never
        assert tracks == 1 + {1: 5, 2: 4, 8: 2}[G] and links.tolist() == {1: [11, 12], 2: [11, 12, 1], 8: [11, 12, 1, 1, 0, 0, 0, 0, 1]}[G]
    _check(_blink(n), 500, K=1, G=G)                                        # object 2 above the cap


# ---------------------------------------------------------------- 3. level order
def _strip(n, spans):
    """n frames of 4 x 4; spans: per frame {label: (first, last)} over the 16 pixels in raster order."""
    s = np.zeros((n, 16), dtype=np.int32)
    for f, frame in enumerate(spans):
        for l, (a, b) in frame.items():
            s[f, a:b + 1] = l
    return s.reshape(n, 4, 4)


def _literal(stack, milli, G, prev, gap, track, K=2):
    want = _check(stack, milli, K=K, G=G)
    assert want["prev"].tolist() == prev and want["gap"].tolist() == gap and want["track"].tolist() == track
    return want


def test_level_order():
    # A (0..3) is gone in frame 1, where the newcomer N (0..11) is too large for it (4 / 12); X (0..5) of frame 2 fits both N (6 / 12,
    # adjacent) and A (4 / 6, two back): the adjacent link wins and A's track ends
    s = _strip(3, [{1: (0, 3)}, {1: (0, 11)}, {1: (0, 5)}])
    _literal(s, 500, 1, prev=[[0, 0], [0, 0], [1, 0]], gap=[[0, 0], [0, 0], [1, 0]], track=[[1, 0], [2, 0], [2, 0]])
    assert base.links(s[0], s[2], 500, 2) == {1: (1, 4, 6)}                # (the bridge was there to be made)
    # a head (1..8) over the open tails two back (4..11, 5 / 11) and three back (0..7, 7 / 9): gap 2 wins against the larger IoU
    s = _strip(4, [{1: (0, 7)}, {2: (4, 11)}, {}, {1: (1, 8)}])
    want = _literal(s, 400, 2, prev=[[0, 0], [0, 0], [0, 0], [2, 0]], gap=[[0, 0], [0, 0], [0, 0], [2, 0]],
                    track=[[1, 0], [0, 2], [0, 0], [2, 0]])
    assert want["gap_links"].tolist() == [0, 1, 0] and want["extra"][:2].tolist() == [[0, 0], [1, 1]] and want["totals"][3] == 3
    assert base.links(s[0], s[3], 400, 2) == {1: (1, 7, 9)}
    # two heads for one tail at exactly 4 / 8 each: the tail's best partner is the smaller number, whichever side of it that lies on
    for first in ({1: (0, 3), 2: (4, 7)}, {2: (0, 3), 1: (4, 7)}):
        s = _strip(3, [{1: (0, 7)}, {}, first])
        _literal(s, 500, 1, prev=[[0, 0], [0, 0], [1, 0]], gap=[[0, 0], [0, 0], [2, 0]], track=[[1, 0], [0, 0], [1, 2]])


# ---------------------------------------------------------------- 4. masking before matching
def test_an_object_that_is_taken_does_not_block_a_bridge():
    # P (0..7) of frame 0 overlaps nothing in frame 1, where R is (8..15).  In frame 2, Q1 = label 1 (2..15) is P's best partner over all
    # objects (6 / 16 against 2 / 8) but continues R (8 / 14); Q2 = label 2 (0..1) is open and P bridges to it
    s = _strip(3, [{1: (0, 7)}, {1: (8, 15)}, {1: (2, 15), 2: (0, 1)}])
    table, area_a, area_b = base.pair_counts(s[0], s[2], 2)
    assert base.best_partner(table[1, :], area_a[1], area_b, 2) == (1, 6)  # unmasked, P would pick Q1 and find it taken
    want = _literal(s, 200, 1, prev=[[0, 0], [0, 0], [1, 1]], gap=[[0, 0], [0, 0], [1, 2]], track=[[1, 0], [2, 0], [2, 1]])
    assert want["table"][0].tolist() == [0, 1, 2, 10, 2, 8, 2, 8] and want["table"][1].tolist() == [1, 1, 2, 22, 8, 14, 8, 14]


# ---------------------------------------------------------------- 5. thresholds at the edge
def test_thresholds_at_the_edge():
    s = np.zeros((3, 64, 64), dtype=np.int32)
    s[0, 10:26, 5:21] = 1
    s[2, 10:26, 6:22] = 1                                                   # 240 / 272 = 15 / 17 = 0.88235... across the empty frame
    for milli, linked in ((1, True), (882, True), (883, False), (1000, False)):
        want = _check(s, milli, G=1)
        assert want["gap_links"].tolist() == [0, int(linked)] and want["totals"].tolist() == [2 - linked, int(linked), 2, 3 if linked else 1]
        if linked:
            assert want["table"][0].tolist() == [0, 1, 2, 512, 256, 256, 240, 272] and want["extra"][0].tolist() == [1, 1]
    s[2] = s[0]
    assert _check(s, 1000, G=1)["gap_links"].tolist() == [0, 1]             # IoU 1 reaches 1000
    assert _check(s, 1000, G=8)["gap_links"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------- 6. random flickering stacks
SHAPES = {"16x16": (64, 16, 16, 4, 64), "64x64": (8, 64, 64, 8, 64), "64x64-K3": (8, 64, 64, 8, 3), "1x1": (12, 1, 1, 1, 64),
          "64x1": (12, 64, 1, 4, 64)}


@functools.lru_cache(maxsize=None)
def _flicker(name):
    """n frames: one object per cell of a grid, shifted by -1..1 pixels (cells of one pixel stay) and absent from a third of the
    frames; the labels of a frame are permuted in one frame of four, and a few pixels carry a label above every cap."""
    n, h, w, cell, _ = SHAPES[name]
    rs = np.random.RandomState(n * h + w + cell)
    rows, cols = -(-h // cell), -(-w // cell)
    s = np.zeros((n, h + 2, w + 2), dtype=np.int32)
    for f in range(n):
        perm = rs.permutation(rows * cols) if f % 4 == 3 else np.arange(rows * cols)
        for i in range(rows * cols):
            if rs.rand() < 1 / 3:
                continue
            dy, dx = (rs.randint(-1, 2), rs.randint(-1, 2)) if cell > 1 else (0, 0)
            y, x = 1 + (i // cols) * cell + dy, 1 + (i % cols) * cell + dx
            s[f, y:y + cell, x:x + cell] = perm[i] + 1
    s = s[:, 1:-1, 1:-1].copy()
    s[rs.rand(n, h, w) < 0.02] = 70
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("milli", [1, 300, 500, 1000])
@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_flickering_stacks(name, G, milli):
    s, K = _flicker(name), SHAPES[name][4]
    want = _check(s, milli, K=K, G=G)
    if name == "16x16" and milli == 300:                                    # the stack shows what it is for
        assert all(want["gap_links"][:G + 1] > 0) and want["totals"][3] > want["table"][:, 2].max()
    if name == "64x64":
        assert s.max() == 70 and len(np.unique(s)) == 66
    if name == "64x64-K3":
        assert not want["track_labels"][s > 3].any()


# ---------------------------------------------------------------- 7. output options and argument errors
def test_output_options():
    s, K, G = _flicker("16x16")[:20], 16, 3
    want = ref.track(s, 300, K, G, want_paint=True)
    count = int(want["totals"][0])
    assert count > 12
    cut = _check(s, 300, K=K, G=G, max_tracks=10)                           # max_tracks below the track count
    assert cut["totals"][0] == count and cut["track"].max() == count and cut["table"].shape == (10, 8)
    np.testing.assert_array_equal(cut["table"], want["table"][:10])
    np.testing.assert_array_equal(cut["extra"], want["extra"][:10])
    assert want["extra"][:10].any()
    for off in ("tracks", "extra", "painted", "rgb"):
        got = _raw(s, 300, K, G, **{off: False})
        junk = {"tracks": "table", "extra": "extra", "painted": "track_labels", "rgb": "rgb"}[off]
        assert (got.pop(junk) == JUNK).all(), off
        _same({k: v for k, v in got.items() if k in KEYS}, want, f"without {off}")
        if "track_labels" in got:
            np.testing.assert_array_equal(got["track_labels"], want["track_labels"])
        if "rgb" in got:
            np.testing.assert_array_equal(got["rgb"], base.colours(want["track_labels"]))


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    assert lib.cgs_objects_track_gap_scratch_bytes(5, 4, -1) == 0 and lib.cgs_objects_track_gap_scratch_bytes(5, 4, 9) == 0
    assert lib.cgs_objects_track_gap_scratch_bytes(0, 4, 1) == 0 and lib.cgs_objects_track_gap_scratch_bytes(5, 0, 1) == 0
    assert lib.cgs_objects_track_gap_scratch_bytes(5, 4, 0) > lib.cgs_objects_track_scratch_bytes(5, 4)
    n, h, w, K = 5, 4, 4, 4
    labels = _up(_blink(n))
    full = lambda *shape, dtype=torch.int32: torch.full(shape, JUNK, dtype=dtype, device=DEV)
    outs = {"prev": full(n, K), "gap": full(n, K), "track": full(n, K), "totals": full(4), "gap_links": full(9 + 1), "tracks": full(n * K, 8),
            "extra": full(n * K, 2), "painted": full(n, h, w), "rgb": full(n, h, w, 3, dtype=torch.uint8)}
    need = int(lib.cgs_objects_track_gap_scratch_bytes(n, K, 8))
    scratch = torch.full((need // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(G=2, bytes_=need, shift=None, **over):
        p = {k: v.data_ptr() for k, v in outs.items()}
        p.update(labels=labels.data_ptr(), scratch=scratch.data_ptr())
        if shift:
            p[shift] += 2 if shift != "scratch" else 4
        p.update(over)
        return lib.cgs_objects_track_gap(p["labels"], n, h, w, K, 500, G, n * K, p["prev"], p["gap"], p["track"], p["totals"], p["gap_links"],
                                         p["tracks"], p["extra"], p["painted"], p["rgb"], p["scratch"], bytes_, stream)

    bad = _lib.ERR_BADARG
    assert call(G=-1) == bad and call(G=9) == bad
    assert call(bytes_=int(lib.cgs_objects_track_gap_scratch_bytes(n, K, 2)) - 1) == bad
    for name in ("labels", "prev", "gap", "track", "totals", "gap_links", "tracks", "extra", "painted", "scratch"):
        assert call(shift=name) == bad, name
    for name in ("labels", "prev", "gap", "track", "totals", "gap_links", "scratch"):
        assert call(**{name: None}) == bad, name
    torch.cuda.synchronize()
    assert all((v == JUNK).all() for v in outs.values()) and (scratch == -1).all()
    assert call() == 0                                                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs["track"].cpu().numpy(), ref.track(_blink(n), 500, K, 2)["track"])


# ---------------------------------------------------------------- 8. TrackStream
def _every_split(n):
    """All 2^(n - 1) ways to cut n frames into chunks."""
    for cuts in itertools.product((False, True), repeat=n - 1):
        edges = [0] + [i + 1 for i, c in enumerate(cuts) if c] + [n]
        yield [b - a for a, b in zip(edges, edges[1:])]


def _splits(n):
    """The subset the CPU test walks with the checker as the tracker: every split of n frames into at most three chunks, single frames
    throughout, and even chunks of 2, 3, 4 and 5."""
    out = [[n], [1] * n]
    out += [[a, n - a] for a in range(1, n)]
    out += [[a, b - a, n - b] for a, b in itertools.combinations(range(1, n), 2)]
    out += [[c] * (n // c) + ([n % c] if n % c else []) for c in (2, 3, 4, 5)]
    return out


@pytest.mark.parametrize("G", [1, 3])
def test_track_stream_every_split(G):
    s = np.concatenate([_flicker("16x16")[:8], np.zeros((1, 16, 16), dtype=np.int32), _flicker("16x16")[9:12]])
    whole = _check(s, 300, K=16, G=G)
    n_tracks = int(whole["totals"][0])
    assert whole["gap_links"][1:].sum() > 2 and n_tracks > 16              # bridges, and tracks that start later
    dev, got = _up(s), []
    splits = list(_every_split(12))
    assert len(splits) == 2048 and [1] * 12 in splits and [12] in splits and all(s in splits for s in _splits(12))
    for split in splits:
        assert sum(split) == 12
        ts = objects.TrackStream(0.3, max_objects=16, max_gap=G)
        parts, lo = [], 0
        for m in split:
            ids = ts.push(dev[lo:lo + m])
            assert ids.dtype == torch.int32 and tuple(ids.shape) == (m, 16) and ids.is_cuda
            parts.append(ids)
            lo += m
        got.append((split, torch.cat(parts), ts.n_tracks))
    for split, ids, count in got:                                           # (read back after the last push: the stream never waits)
        np.testing.assert_array_equal(ids.cpu().numpy(), whole["track"], err_msg=f"G={G} split {split}")
        assert int(count) == n_tracks
    with pytest.raises(ValueError):
        objects.TrackStream(0.3, max_gap=9)


# ---------------------------------------------------------------- 9. switches and fragments
def _scores(pred, truth, track_milli, match_milli, K, G):
    pred, truth, iou = _up(pred), _up(truth), [m / 1000 for m in match_milli]
    pt, tt = (objects.track(s, iou=track_milli / 1000, max_objects=K, max_gap=G) for s in (pred, truth))
    best = objects.match(pred, truth, iou=iou, max_objects=K).best
    truth_prev = torch.where(tt.gap == 1, tt.prev, 0) if G else tt.prev
    frag = objects.fragments(tt.track, pt.track, best, iou)
    assert frag.dtype == torch.int64 and frag.shape == (len(match_milli),) and frag.is_cuda
    return objects.switches(truth_prev, pt.track, best, iou).cpu().numpy(), frag.cpu().numpy()


def _dropped(stack, seed, p=0.25):
    """The stack with every object of every frame removed with probability p."""
    rs, out = np.random.RandomState(seed), np.array(stack)
    for f in range(len(out)):
        for l in np.unique(out[f]):
            if l > 0 and rs.rand() < p:
                out[f][out[f] == l] = 0
    return out


def test_switches_and_fragments():
    truth = np.zeros((9, 8, 8), dtype=np.int32)                             # two objects that stay; the prediction drops each now and then
    truth[:, 1:4, 1:7], truth[:, 5:7, 2:6] = 1, 2
    pred = truth.copy()
    pred[2][truth[2] == 1] = 0
    pred[5][truth[5] == 1] = 0
    pred[4][truth[4] == 2] = 0
    pred[:, 1, 1] = 0                                                       # and is a pixel short of object 1: 17 / 18
    want = {G: (ref.switches(pred, truth, 300, [500, 950], 4, G), ref.fragments(pred, truth, 300, [500, 950], 4, G)) for G in (0, 1)}
    assert want[0][1].tolist() == [3, 1] and want[1][1].tolist() == [0, 0]  # three breaks; at 0.95 only object 2 is covered
    assert want[0][0].tolist() == want[1][0].tolist() == [[15, 10, 0], [8, 6, 0]]          # no adjacent link changes its predicted track
    for G in (0, 1):
        got = _scores(pred, truth, 300, [500, 950], 4, G)
        np.testing.assert_array_equal(got[0], want[G][0])
        np.testing.assert_array_equal(got[1], want[G][1])
    t = _flicker("16x16")[:24]
    s = _dropped(t, 7)                                                      # the prediction misses a quarter of the truth's objects
    for G in (0, 2):
        got = _scores(s, t, 300, [500, 650, 800], 16, G)
        np.testing.assert_array_equal(got[0], ref.switches(s, t, 300, [500, 650, 800], 16, G))
        np.testing.assert_array_equal(got[1], ref.fragments(s, t, 300, [500, 650, 800], 16, G))
        assert got[0][0, 1] > 0 and got[1][0] > 0


# ---------------------------------------------------------------- 10. end to end
def _run(argv, capsys):
    capsys.readouterr()
    H = cli.main(argv + ["--model", "m"])
    return H, capsys.readouterr().out


def _files(folder):
    out = {}
    for f in sorted(os.listdir(folder)):
        with open(os.path.join(folder, f), "rb") as fp:
            out[f] = fp.read()
    return out


def _side(labels, kept, milli, G):
    t = ref.track(labels, milli, 64, G)
    return t, objects.track_report(t["totals"], t["table"][:, 2], int(t["table"][:, 6].astype(np.int64).sum()),
                                   int(t["table"][:, 7].astype(np.int64).sum()), int(np.maximum(kept - 64, 0).sum()), max_gap=G,
                                   gap_links=t["gap_links"], missed=int(t["extra"][:, 1].sum()))


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """test_gpu_objects_track.py's folder: the synthetic red-trees/ and the G1 checkpoints, every frame rolled by half its index."""
    root = str(tmp_path)
    for name, state in zip([str(s) for s in golden("g6_process.npz")["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    Xe = np.stack([np.roll(_structured(64, 64, 200 + k // 80)[0], k // 2, axis=1) for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    monkeypatch.chdir(root)
    return root, Xe[slice(100, 5000, 2)]


def test_cli_process_track_gap(workdir, capsys):
    from PIL import Image
    root, frames = workdir
    os.makedirs("S")
    stems = [f"f{k}" for k in (1, 2, 3, 10, 11, 12, 20, 21, 100, 101)]
    for stem, frame in zip(stems, frames[:len(stems)]):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S")]
    thr = float(np.median(M))
    labels, _, kept, _, _ = objects_ref.label(objects_ref.on_pixels(M[:, 0], thr, inclusive=True), 8, 2, 64)
    order = [listed.index(s) for s in stems]
    t, side = _side(labels[order], kept[order], 300, 2)
    assert side["track_gap"] == 2 and set(side["links_by_gap"]) == {"1", "2", "3"} and side["max_span"] == int(t["totals"][3])

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2", "--track-iou", "0.3"]
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    _run(common + ["--mask-output-imgs", "R2", "--track-gap", "0"], capsys)
    _run(common + ["--mask-output-imgs", "R3", "--track-gap", "2"], capsys)
    r1, r2, r3 = _files("R1"), _files("R2"), _files("R3")
    assert r1 == r2 and set(r3) == set(r1)                                 # without the flag, and at 0: cgs_objects_track's files
    assert all(r3[f] == r1[f] for f in r1 if "tracks" not in f)
    flat = json.loads(r1["tracks.json"])
    assert "track_gap" not in flat and set(flat["summary"]) == set(_side(labels[order], kept[order], 300, 0)[1]) and "gap" not in str(flat)
    report = json.loads(r3["tracks.json"])
    rows = objects.track_rows(t["table"], side["tracks"], t["extra"])
    assert report == {"source": "thresholded-mask", "threshold": thr, "connectivity": 8, "min_area": 2, "max_objects": 64, "track_iou": 0.3,
                      "track_gap": 2, "summary": side, "order": stems,
                      "frames": {s: [{"label": l + 1, "track": int(t["track"][j, l]), "prev": int(t["prev"][j, l]), "gap": int(t["gap"][j, l])}
                                     for l in np.flatnonzero(t["track"][j])] for j, s in enumerate(stems)},
                      "tracks": [{"track": r["track"], "first": stems[r["first_frame"]], "last": stems[r["last_frame"]], "length": r["length"],
                                  "area_sum": r["area_sum"], "area_min": r["area_min"], "area_max": r["area_max"], "link_iou": r["link_iou"],
                                  "bridges": r["bridges"], "missed": r["missed"]} for r in rows]}
    painted = ref.track(labels[order], 300, 64, 2, want_paint=True)["track_labels"]
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R3", f"{s}-tracks-mask.png"))), base.colours(painted[j]))


def test_cli_eval_track_gap(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    pred_labels, _, pred_kept, _, _ = objects_ref.label(objects_ref.on_pixels(M[:, 0], thr), 8, 4, 64)
    truth_labels, _, truth_kept, _, _ = objects_ref.label(truth, 8, 1, 64)
    (pt, pred_side), (tt, truth_side) = _side(pred_labels, pred_kept, 300, 1), _side(truth_labels, truth_kept, 300, 1)
    tracks_file = os.path.join(root, "m", "eval_tracks.json")
    read = lambda: open(tracks_file, "rb").read()
    line = lambda text: [ln for ln in text.split("\n") if ln.startswith("TRACKS")]

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4", "--match-iou", "0.5", "--track-iou", "0.3"]
    _, plain = _run(common, capsys)
    plain_json = read()
    _, zero = _run(common + ["--track-gap", "0"], capsys)
    assert read() == plain_json and line(zero) == line(plain) and "fragments" not in plain_json.decode() and "bridged" not in plain
    H1, out = _run(common + ["--track-gap", "1"], capsys)
    assert line(out) == [f"TRACKS conn=8 min_area=4 iou>=0.3 gap<=1: {pred_side['tracks']} tracks over {pred_side['objects']} objects "
                         f"({pred_side['bridged_links']} of {pred_side['links']} links bridged), mean length {pred_side['mean_length']:.6f}, "
                         f"longest {pred_side['max_length']}; truth {truth_side['tracks']} tracks over {truth_side['objects']} objects"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]
    c = ref.switches(pred_labels, truth_labels, 300, [500], 64, 1)[0]
    rows = [{"iou": 0.5, "covered": int(c[0]), "continued": int(c[1]), "switches": int(c[2]), "switch_rate": int(c[2]) / int(c[1]) if c[1] else None,
             "fragments": int(ref.fragments(pred_labels, truth_labels, 300, [500], 64, 1)[0])}]
    assert json.loads(read()) == H1.tracks == {"connectivity": 8, "min_area": 4, "threshold": thr, "max_objects": 64, "track_iou": 0.3,
                                               "truth": truth_side, "mask": {"pred": pred_side, "switches": rows}}
    assert pred_side["track_gap"] == 1 and rows[0]["covered"] > 0


@pytest.fixture()
def videodir(tmp_path, golden, g1, monkeypatch):
    """test_gpu_process_video_tracks.py's folder: the G6 frames as in.raw (128 x 128) and its stub ffprobe / ffmpeg first on PATH."""
    root = str(tmp_path)
    g = golden("g6_process.npz")
    for name, state in zip([str(s) for s in g["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    frames, names = g["frames"], [str(s) for s in g["names"]]
    big = np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)
    order = objects.natural_order(names)
    with open(os.path.join(root, "in.raw"), "wb") as fp:
        fp.write(np.ascontiguousarray(big[order]).tobytes())
    bindir, calls = os.path.join(root, "bin"), os.path.join(root, "ffmpeg_calls")
    os.makedirs(bindir)
    os.makedirs(calls)
    with open(os.path.join(root, "probe.txt"), "w") as fp:
        fp.write("128,128,10/1\n")
    for exe, text in (("ffmpeg", FFMPEG.format(python=sys.executable, out=calls)),
                      ("ffprobe", FFPROBE.format(python=sys.executable, answer=os.path.join(root, "probe.txt")))):
        with open(os.path.join(bindir, exe), "w") as fp:
            fp.write(text)
        os.chmod(os.path.join(bindir, exe), 0o755)
    monkeypatch.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
    monkeypatch.chdir(root)
    return len(names), calls


def _video(argv, results):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-video", "in.raw", "--overlay-video", "out.mp4",
                                        "--mask-output-imgs", results, "--overlay-tracks", "0.3"] + argv))
    assert H.load_models()
    return H.segment(folder=H.args.source_imgs)


def test_video_overlay_gap(videodir, monkeypatch):
    n, calls = videodir
    sent = lambda i: np.fromfile(os.path.join(calls, f"{i}.stdin"), dtype=np.uint8)
    M = _video([], "R0")
    _video(["--overlay-gap", "0"], "RZ")
    assert _files("R0") == _files("RZ")                                    # without the flag, and at 0: today's files and frames
    np.testing.assert_array_equal(sent(0), sent(1))
    M1 = _video(["--overlay-gap", "1"], "R1")
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    M3 = _video(["--overlay-gap", "1"], "R3")
    assert n > 3
    np.testing.assert_array_equal(M1, M)
    np.testing.assert_array_equal(M3, M)
    np.testing.assert_array_equal(sent(2), sent(3))                        # one chunk and chunks of 3: the same numbers drawn
    r1, r3 = _files("R1"), _files("R3")
    assert r1 == r3 and set(r1) == {"out.json", "out-objects.json", "out-tracks.json"} and r1["out-objects.json"] == _files("R0")["out-objects.json"]
    res = objects.label(torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV), thresh=0.5, inclusive=True, connectivity=8, min_area=1,
                        max_objects=64)
    want = ref.track(res.labels.cpu().numpy(), 300, 64, 1)
    rep = json.loads(r1["out-tracks.json"])
    assert rep["track_gap"] == 1 and rep["summary"]["track_gap"] == 1 and rep["summary"]["tracks"] == int(want["totals"][0])
    for i in range(n):
        assert {r["label"]: (r["track"], r["gap"]) for r in rep["frames"][f"{i:06d}"]} == {
            int(l) + 1: (int(want["track"][i, l]), int(want["gap"][i, l])) for l in np.flatnonzero(want["track"][i])}
    info = json.loads(r1["out.json"])["tracks"]
    assert info["gap"] == 1 and info["n_tracks"] == int(want["totals"][0]) and "gap" not in json.loads(_files("R0")["out.json"])["tracks"]
