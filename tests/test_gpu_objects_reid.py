"""Re-identifying tracks by colour on the GPU (cgs_objects_appearance, cgs_objects_reid; cgs_amd.objects.appearance / reid) against the
rule as tests/objects_reid_ref.py writes it, on tracks made by objects.track of the same labels.  Everything is integer: exact equality
everywhere.  The by-hand cases, the generated stack and its conditions are those of tests/test_objects_reid_host.py, where the checker
has to give them first."""
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

import objects_reid_ref as ref  # noqa: E402
from cgs_amd import _lib, objects  # noqa: E402
from test_objects_reid_host import CASES, GENERATED, TRACK_MILLI, check_case, generated, generated_conditions  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 77
OUTS = ("prev", "next", "sim", "identity")


def _up(a, dtype=np.int32):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _gpu(frames, labels, K, G, milli, W, min_area, motion=False):
    """objects.track, appearance and reid on the GPU; everything on the host."""
    n = len(labels)
    field = torch.zeros((n - 1, 8, 8, 2), dtype=torch.int8, device=DEV) if motion else None
    tr = objects.track(_up(labels), iou=TRACK_MILLI / 1000, max_objects=K, max_gap=G, motion=field)
    ap = objects.appearance(_up(frames, np.uint8), _up(labels), tr, max_objects=K, want_objects=True)
    rd = objects.reid(tr, ap, n, sim=milli / 1000, window=W, min_area=min_area)
    torch.cuda.synchronize()
    scalars = (rd.n_identities, rd.n_links, rd.n_eligible, rd.longest)
    assert all(t.is_cuda and t.dtype == torch.int32 and t.dim() == 0 for t in scalars) and rd.signature.dtype == torch.int16
    assert all(getattr(rd, k).dtype == torch.int32 and getattr(rd, k).is_cuda for k in ("prev", "next", "sim", "identity"))
    host = lambda t: None if t is None else t.cpu().numpy()
    return {"track": host(tr.track), "table": host(tr.table), "extra": host(tr.extra), "n_tracks": int(tr.n_tracks), "S": host(ap.track_hist),
            "H": host(ap.object_hist), "prev": host(rd.prev), "next": host(rd.next), "sim": host(rd.sim), "identity": host(rd.identity),
            "Q": host(rd.signature), "totals": [int(v) for v in scalars], "tracks": tr, "appearance": ap, "reid": rd}


def _check(frames, labels, K, G=0, milli=800, W=64, min_area=64, motion=False, what=""):
    """The kernels against the checker on the GPU tracker's tracks; returns (the checker's result, the GPU's)."""
    frames, labels = np.asarray(frames), np.asarray(labels)
    got = _gpu(frames, labels, K, G, milli, W, min_area, motion)
    rows = got["table"].shape[0]
    assert rows == len(labels) * K and got["S"].shape == got["Q"].shape == (rows, 64) and got["H"].shape == (len(labels), K, 64)
    S, H = ref.appearance(frames, labels, got["track"], K)
    np.testing.assert_array_equal(got["H"], H, err_msg=f"H {what}")
    np.testing.assert_array_equal(got["S"], S, err_msg=f"S {what}")
    want = ref.reid(got["table"], got["extra"], S, got["n_tracks"], milli, W, min_area)
    print(f"{what} n={len(labels)} {labels.shape[1]}x{labels.shape[2]} K={K} G={G} milli={milli} W={W} area>={min_area}: "
          f"{got['n_tracks']} tracks, totals {want['totals']}, {len(want['admissible'])} admissible pairs")
    for key in OUTS + ("Q",):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")
    assert got["totals"] == want["totals"]
    return want, got


# ---------------------------------------------------------------- 1. the by-hand cases
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_by_hand(case):
    c = case()
    want, got = _check(c["frames"], c["labels"], c["K"], c["G"], c["milli"], c["W"], c["min_area"], what=case.__name__)
    assert got["n_tracks"] == len(c["want"]["identity"])
    check_case(c, got, got["table"].shape[0])


# ---------------------------------------------------------------- 2. the C ABI itself
def _inputs(seed=3):
    """A small stack with links, tracked on the GPU: what the raw entries take."""
    frames, labels = generated(n=24, seed=seed)
    tr = objects.track(_up(labels), iou=TRACK_MILLI / 1000, max_objects=16, max_gap=1)
    return _up(frames, np.uint8), _up(labels), tr


def _raw_appearance(frames, labels, track, K, rows, S=True, H=True, shape=None):
    n, h, w = shape or tuple(int(s) for s in labels.shape)
    full = lambda *s: torch.full(s, JUNK, dtype=torch.int32, device=DEV)
    o = {"S": full(max(rows, 1), 64), "H": full(len(labels), K, 64)}
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t
    code = _lib.load().cgs_objects_appearance(ptr(frames), ptr(labels), ptr(track), n, h, w, K, rows, ptr(o["S"]) if S is True else S,
                                              ptr(o["H"]) if H is True else H, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in o.items()}


def _raw_reid(S, table, extra, n_tracks, n, rows, milli=800, W=64, min_area=64, scratch_bytes=None, **swap):
    full = lambda *s: torch.full(s, JUNK, dtype=torch.int32, device=DEV)
    o = {"prev": full(rows), "next": full(rows), "sim": full(rows), "identity": full(rows), "totals": full(4),
         "Q": torch.full((rows, 64), JUNK, dtype=torch.int16, device=DEV)}
    need = int(_lib.load().cgs_objects_reid_scratch_bytes(min(n, objects.REID_MAX_FRAMES + 1) if n > 0 else 1, max(rows, 1)))
    scratch = torch.full(((need + 7) // 8 + 1,), JUNK, dtype=torch.int64, device=DEV)
    a = {"S": S, "table": table, "extra": extra, "n_tracks": n_tracks, "scratch": scratch, **o}
    a.update(swap)
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t
    code = _lib.load().cgs_objects_reid(ptr(a["S"]), ptr(a["table"]), ptr(a["extra"]), ptr(a["n_tracks"]), n, rows, milli, W, min_area,
                                        ptr(a["prev"]), ptr(a["next"]), ptr(a["sim"]), ptr(a["identity"]), ptr(a["totals"]), ptr(a["Q"]),
                                        ptr(a["scratch"]), need if scratch_bytes is None else scratch_bytes,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in o.items()}


def test_raw_entries_on_junk_filled_outputs():
    frames, labels, tr = _inputs()
    n, K, rows = int(labels.shape[0]), 16, int(tr.table.shape[0])
    N = int(tr.n_tracks)
    f, l, t = frames.cpu().numpy(), labels.cpu().numpy(), tr.track.cpu().numpy()
    S, H = ref.appearance(f, l, t, K)
    code, o = _raw_appearance(frames, labels, tr.track, K, rows)
    assert code == _lib.OK
    np.testing.assert_array_equal(o["S"], S)
    np.testing.assert_array_equal(o["H"], H)
    assert 0 < N < rows and not o["S"][N:].any() and o["S"][:N].any()
    code, o = _raw_appearance(frames, labels, tr.track, K, rows, H=None)     # what was not asked for stays junk
    assert code == _lib.OK and (o["H"] == JUNK).all()
    np.testing.assert_array_equal(o["S"], S)
    code, o = _raw_appearance(frames, labels, None, K, 0, S=None)
    assert code == _lib.OK and (o["S"] == JUNK).all()
    np.testing.assert_array_equal(o["H"], H)
    code, o = _raw_appearance(frames, labels, tr.track, K, 5)               # a short table: tracks beyond it count nowhere
    assert code == _lib.OK
    np.testing.assert_array_equal(o["S"], S[:5])

    Sd, count = _up(S), tr.n_tracks.reshape(1).clone()
    want = ref.reid(tr.table.cpu().numpy(), tr.extra.cpu().numpy(), S, N, 800, 20, 64)
    assert want["totals"][1] > 0
    code, o = _raw_reid(Sd, tr.table, tr.extra, count, n, rows, W=20)
    assert code == _lib.OK and o["totals"].tolist() == want["totals"]
    for key in OUTS + ("Q",):
        np.testing.assert_array_equal(o[key], want[key], err_msg=key)
        assert not o[key][N:].any()                                       # rows from n_tracks on are zero
    without = ref.reid(tr.table.cpu().numpy(), None, S, N, 800, 20, 64)
    code, o = _raw_reid(Sd, tr.table, None, count, n, rows, W=20)
    assert code == _lib.OK and o["totals"].tolist() == without["totals"]
    np.testing.assert_array_equal(o["identity"], without["identity"])
    code, o = _raw_reid(Sd, tr.table, tr.extra, _up([rows + 9]), n, rows, W=20)     # more than the table holds: clamped; the zero rows break the
    assert code == _lib.OK and 0 <= o["identity"].min() and o["identity"].max() <= rows      # first column's order, so only the ranges are checked
    for fewer in (0, 3, -5):                                                # n_tracks is read on the device
        m = max(0, min(fewer, rows))
        want = ref.reid(tr.table.cpu().numpy(), tr.extra.cpu().numpy(), S, m, 800, 20, 64)
        code, o = _raw_reid(Sd, tr.table, tr.extra, _up([fewer]), n, rows, W=20)
        assert code == _lib.OK and o["totals"].tolist() == want["totals"], fewer
        for key in OUTS + ("Q",):
            np.testing.assert_array_equal(o[key], want[key], err_msg=f"{key} n_tracks={fewer}")
    small = 7                                                               # a truncated table re-identifies the tracks it holds
    want = ref.reid(tr.table.cpu().numpy()[:small], tr.extra.cpu().numpy()[:small], S[:small], N, 800, 20, 64)
    code, o = _raw_reid(_up(S[:small]), tr.table[:small].contiguous(), tr.extra[:small].contiguous(), count, n, small, W=20)
    assert code == _lib.OK and o["totals"].tolist() == want["totals"]
    np.testing.assert_array_equal(o["identity"], want["identity"])


def test_argument_errors_launch_nothing():
    frames, labels, tr = _inputs()
    n, K, rows = int(labels.shape[0]), 16, int(tr.table.shape[0])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    full = lambda *s: torch.full(s, JUNK, dtype=torch.int32, device=DEV)
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t
    odd = lambda t: t.data_ptr() + 2

    S, H = full(rows, 64), full(n, K, 64)
    base = dict(frames=frames, labels=labels, track=tr.track, n=n, h=64, w=64, K=K, rows=rows, S=S, H=H)
    bad = [dict(n=0), dict(h=0), dict(w=0), dict(K=0), dict(frames=None), dict(labels=None), dict(track=None), dict(S=None),
           dict(track=None, S=None, H=None), dict(rows=0), dict(labels=odd(labels)), dict(track=odd(tr.track)), dict(S=odd(S)), dict(H=odd(H)),
           dict(K=0, h=65)]                                                 # (a bad argument comes before an unsupported one)
    unsupported = [dict(h=65), dict(w=65), dict(K=65), dict(n=objects.REID_MAX_FRAMES + 1)]
    for kw, want in [(k, _lib.ERR_BADARG) for k in bad] + [(k, _lib.ERR_UNSUPPORTED) for k in unsupported]:
        a = {**base, **kw}
        code = lib.cgs_objects_appearance(*(ptr(a[k]) for k in ("frames", "labels", "track", "n", "h", "w", "K", "rows", "S", "H")), stream)
        torch.cuda.synchronize()
        assert code == want and bool((S == JUNK).all()) and bool((H == JUNK).all()), kw

    Sz = torch.zeros((rows, 64), dtype=torch.int32, device=DEV)
    outs = {k: full(rows) for k in OUTS}
    outs.update(totals=full(4), Q=torch.full((rows, 64), JUNK, dtype=torch.int16, device=DEV))
    need = int(lib.cgs_objects_reid_scratch_bytes(objects.REID_MAX_FRAMES + 1, rows))
    scratch = torch.full((need // 8 + 1,), JUNK, dtype=torch.int64, device=DEV)
    base = dict(S=Sz, table=tr.table, extra=tr.extra, n_tracks=tr.n_tracks.reshape(1).clone(), n=n, rows=rows, milli=800, W=64, area=64,
                **outs, scratch=scratch, bytes=need)
    order = ("S", "table", "extra", "n_tracks", "n", "rows", "milli", "W", "area", "prev", "next", "sim", "identity", "totals", "Q",
             "scratch", "bytes")
    bad = [dict(milli=0), dict(milli=1001), dict(W=0), dict(W=objects.REID_MAX_WINDOW + 1), dict(area=0), dict(n=0), dict(rows=0),
           dict(S=None), dict(table=None), dict(n_tracks=None), dict(prev=None), dict(next=None), dict(sim=None), dict(identity=None),
           dict(totals=None), dict(Q=None), dict(scratch=None), dict(bytes=int(lib.cgs_objects_reid_scratch_bytes(n, rows)) - 1),
           dict(S=odd(Sz)), dict(table=odd(tr.table)), dict(extra=odd(tr.extra)), dict(n_tracks=odd(Sz)), dict(prev=odd(outs["prev"])),
           dict(Q=outs["Q"].data_ptr() + 8), dict(scratch=scratch.data_ptr() + 4), dict(n=objects.REID_MAX_FRAMES + 1, milli=0)]
    for kw, want in [(k, _lib.ERR_BADARG) for k in bad] + [(dict(n=objects.REID_MAX_FRAMES + 1), _lib.ERR_UNSUPPORTED)]:
        a = {**base, **kw}
        code = lib.cgs_objects_reid(*(ptr(a[k]) for k in order), stream)
        torch.cuda.synchronize()
        assert code == want and all(bool((v == JUNK).all()) for v in outs.values()) and bool((scratch == JUNK).all()), kw
    assert lib.cgs_objects_reid_scratch_bytes(0, 5) == 0 and lib.cgs_objects_reid_scratch_bytes(5, 0) == 0
    assert lib.cgs_objects_reid_scratch_bytes(3, 6) % 8 == 0
    code = lib.cgs_objects_reid(*(ptr(base[k]) for k in order), stream)     # the same arguments, untouched, run
    torch.cuda.synchronize()
    assert code == _lib.OK and not bool((outs["totals"] == JUNK).any())


# ---------------------------------------------------------------- 3. the small shapes
def _noisy(n, h, w, K, seed, junk=False):
    """Random label maps (values 0..K, hand-made: no components) over random palette pixels, an empty frame now and then."""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, K + 1, (n, h, w)).astype(np.int32)
    labels[rs.rand(n) < 0.3] = 0
    palette = np.array([(200, 30, 30), (30, 200, 30), (63, 64, 191), (64, 127, 192), (255, 255, 255), (0, 0, 0)], dtype=np.uint8)
    frames = palette[rs.randint(0, len(palette), (n, h, w))]
    if junk:
        r = rs.rand(n, h, w)
        labels[r < 0.05] = -3
        labels[(r >= 0.05) & (r < 0.1)] = 70
        labels[(r >= 0.1) & (r < 0.15)] = 0x7FFFFFFF
        assert (labels == 70).any() and (labels < 0).any() and (labels == 0x7FFFFFFF).any()
    return frames, labels


@pytest.mark.parametrize("n, h, w, K", [(1, 1, 1, 1), (2, 1, 1, 1), (1, 5, 7, 3), (2, 5, 7, 64), (9, 64, 63, 5), (9, 64, 64, 64), (7, 64, 64, 1),
                                        (12, 5, 7, 1)])
def test_small_shapes(n, h, w, K):
    frames, labels = _noisy(n, h, w, K, seed=n + h + K, junk=h * w >= 35)
    for G, milli, W, area in ((0, 1, 1, 1), (0, 1000, max(n, 1), 1), (1, 500, 1024, 2), (0, 1, 1024, 3)):
        _check(frames, labels, K, G, milli, W, area, what="small")


def test_blinking_object_every_window_and_threshold():
    """One object that blinks with a colour that drifts: the links depend on W and on the threshold."""
    n = 14
    frames, labels = np.zeros((n, 5, 7, 3), dtype=np.uint8), np.zeros((n, 5, 7), dtype=np.int32)
    for f in (0, 1, 3, 6, 7, 12, 13):
        labels[f, 1:4, 1:6] = 1
        frames[f, 1:4, 1:6] = (200, 30, 30)
        frames[f, 1:4, 1:1 + f % 5] = (30, 200, 30)
    seen = set()
    for W in (1, 2, 4, n, 1024):
        for milli in (1, 600, 1000):
            want, _ = _check(frames, labels, 2, 0, milli, W, 1, what="blink")
            seen.add(want["totals"][1])
    assert len(seen) > 2


def test_no_eligible_track():
    frames, labels = _noisy(6, 5, 7, 4, seed=1)
    want, got = _check(frames, labels, 4, 0, 800, 64, 5 * 7 * 6 + 1, what="nothing eligible")
    assert want["totals"][1:3] == [0, 0] and want["totals"][0] == got["n_tracks"] > 0 and not got["Q"].any()
    empty = np.zeros_like(labels)
    want, got = _check(frames, empty, 4, 0, 800, 64, 1, what="no object")
    assert want["totals"] == [0, 0, 0, 0] and got["n_tracks"] == 0


def test_full_frame_objects():
    rs = np.random.RandomState(2)
    frames = np.where(rs.rand(4, 64, 64, 1) < 0.37, np.uint8(200), np.uint8(40)) * np.ones(3, dtype=np.uint8)
    labels = np.ones((4, 64, 64), dtype=np.int32)
    labels[1] = 0                                                           # A = 4096 in frame 0, then 2 x 4096
    want, got = _check(frames.astype(np.uint8), labels, 1, 0, 900, 4, 4096, what="full frame")
    assert got["S"][0].sum() == 4096 and got["S"][1].sum() == 8192 and want["totals"][1] == 1
    # one object over the whole frame for 600 frames: S is about 2.4 M, S * 4096 needs 64 bits
    n = 606
    frames = np.where(rs.rand(n, 64, 64, 1) < 0.6, np.uint8(200), np.uint8(40)) * np.ones(3, dtype=np.uint8)
    labels = np.ones((n, 64, 64), dtype=np.int32)
    labels[600:603] = 0
    want, got = _check(frames.astype(np.uint8), labels, 1, 0, 950, 8, 64, what="600 frames")
    assert got["table"][0, 2] == 600 and got["S"][0].sum() == 600 * 4096 and int(got["S"][0].max()) * 4096 > 2 ** 32
    assert want["totals"] == [1, 1, 2, 2]


# ---------------------------------------------------------------- 4. the generated stack
@functools.lru_cache(maxsize=None)
def _generated():
    frames, labels = generated()
    frames.setflags(write=False), labels.setflags(write=False)
    return frames, labels


@pytest.mark.parametrize("G, motion", [(0, False), (2, False), (0, True), (2, True)])
def test_generated_stack(G, motion):
    frames, labels = _generated()
    want, got = _check(frames, labels, 64, G, motion=motion, what=f"generated motion={motion}", **GENERATED)
    generated_conditions(want, f"G={G} motion={motion}")
    assert got["n_tracks"] > 4 * 2                                          # more than one workgroup of the pair pass


def test_reproducible_and_consistent():
    frames, labels = _generated()
    a = _gpu(frames, labels, 64, 2, **GENERATED)
    b = _gpu(frames, labels, 64, 2, **GENERATED)
    for key in OUTS + ("Q", "S", "H"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["totals"] == b["totals"]
    tr, ap = a["tracks"], a["appearance"]
    sums = torch.zeros_like(ap.track_hist, dtype=torch.int64)              # track_hist is the per-track sum of object_hist
    t = tr.track.reshape(-1).to(torch.int64)
    sums.index_add_(0, (t[t > 0] - 1), ap.object_hist.reshape(-1, 64)[t > 0].to(torch.int64))
    assert torch.equal(sums, ap.track_hist.to(torch.int64))
    alone = objects.appearance(_up(frames, np.uint8), _up(labels), None, max_objects=64)
    assert alone.track_hist is None and torch.equal(alone.object_hist, ap.object_hist)
    only = objects.appearance(_up(frames, np.uint8), _up(labels), tr, max_objects=64)
    assert only.object_hist is None and torch.equal(only.track_hist, ap.track_hist)
    per_object = objects.identities(tr.track, a["reid"].identity)
    np.testing.assert_array_equal(per_object.cpu().numpy(), ref.object_identities(a["track"], a["identity"]))
    with pytest.raises(ValueError, match="truncated table"):
        short = objects.track(_up(labels), iou=0.5, max_objects=64, max_tracks=10)
        objects.reid(short, objects.appearance(_up(frames, np.uint8), _up(labels), short, max_objects=64), len(labels))
