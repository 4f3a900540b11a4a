"""Filling the frames a bridged track misses on the GPU (cgs_objects_track_fill, cgs_amd.objects.fill) against the per-cell rule of
tests/objects_track_fill_ref.py, on tracks made by objects.track of the same inputs.  Everything is integer: exact equality
everywhere.  The by-hand cases and their expected arrays are those of tests/test_objects_track_fill_host.py, where the checker has to
give them first."""
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

import objects_track_fill_ref as ref  # noqa: E402
from cgs_amd import _lib, objects  # noqa: E402
from test_objects_track_fill_host import CASES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 77
KEYS = ("labels", "track", "age", "table", "totals")


def _up(a, dtype=np.int32):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _tracks(labels, bwd, milli, K, G):
    """objects.track of the stack on the GPU: (Tracks, its prev / gap / track on the host)."""
    tr = objects.track(_up(labels), iou=milli / 1000, max_objects=K, max_tracks=1, max_gap=G, motion=None if bwd is None else _up(bwd, np.int8))
    return tr, {k: getattr(tr, k).cpu().numpy() for k in ("prev", "gap", "track")}


def _host(fl):
    torch.cuda.synchronize()
    out = {"labels": fl.labels, "track": fl.track, "age": fl.age, "totals": torch.stack([fl.n_objects, fl.n_cells, fl.n_dropped, fl.n_vanished])}
    if fl.table is not None:
        out["table"] = fl.table
    if fl.rgb is not None:
        out["rgb"] = fl.rgb
    assert all(t.is_cuda and t.dtype == (torch.uint8 if k == "rgb" else torch.int32) for k, t in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, K, what=""):
    for key in KEYS:
        if key in got:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")
    if "rgb" in got:
        np.testing.assert_array_equal(got["rgb"], ref.paint(want["labels"], want["track"], K)[1], err_msg=f"rgb {what}")


def _check(labels, bwd, milli, K, G):
    """The kernel against the checker on the GPU tracker's tracks; returns the checker's result."""
    labels = np.asarray(labels)
    tr, host = _tracks(labels, bwd, milli, K, G)
    got = _host(objects.fill(_up(labels), tr, motion=None if bwd is None else _up(bwd, np.int8), max_objects=K, want_rgb=True))
    want = ref.fill(labels, bwd, host["prev"], host["gap"], host["track"], K, G)
    print(f"n={len(labels)} K={K} G={G} milli={milli}: totals {want['totals'].tolist()}")
    _same(got, want, K, f"K={K} G={G} milli={milli}")
    n, h, w = labels.shape
    assert got["labels"].shape == (n, h, w) and got["track"].shape == got["age"].shape == (n, K) and got["table"].shape == (n, K, 8)
    return want


def _raw(labels, bwd, K, G, prev, gap, track, table=True):
    """cgs_objects_track_fill itself on outputs full of junk; what was not asked for stays junk."""
    labels = _up(labels)
    n, h, w = (int(s) for s in labels.shape)
    full = lambda *shape: torch.full(shape, JUNK, dtype=torch.int32, device=DEV)
    o = {"labels": full(n, h, w), "track": full(n, K), "age": full(n, K), "table": full(n, K, 8), "totals": full(4)}
    ins = [_up(prev), _up(gap), _up(track)]
    field = None if bwd is None else _up(bwd, np.int8)
    _lib.call("cgs_objects_track_fill", labels.data_ptr(), field.data_ptr() if field is not None else None, n, h, w, K, G,
              *(t.data_ptr() for t in ins), o["labels"].data_ptr(), o["track"].data_ptr(), o["age"].data_ptr(),
              o["table"].data_ptr() if table else None, o["totals"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---------------------------------------------------------------- the stacks
@functools.lru_cache(maxsize=None)
def _stack(n, seed=0, cell=8, junk=False):
    """n frames of 64 x 64: one blob per cell of a grid, shifted by -1..1 cells and absent from a third of the frames, numbered per
    frame in raster order of the blobs that are there, as objects.label numbers them.  junk: a few cells hold values that are no
    objects -- negative ones in every frame, 70 and 0x7fffffff in every fourth."""
    rs = np.random.RandomState(1000 * seed + n + cell)
    per = 64 // cell
    s = np.zeros((n, 66, 66), dtype=np.int32)
    for f in range(n):
        k = 0
        for i in range(per * per):
            gone = rs.rand() < 1 / 3
            dy, dx = rs.randint(-1, 2), rs.randint(-1, 2)
            if gone:
                continue
            k += 1
            y, x = 1 + (i // per) * cell + dy, 1 + (i % per) * cell + dx
            s[f, y:y + cell - 1, x:x + cell - 1] = k
    s = s[:, 1:-1, 1:-1].copy()
    if junk:
        r = rs.rand(n, 64, 64)
        s[r < 0.02] = -3
        s[3::4][(r[3::4] >= 0.02) & (r[3::4] < 0.03)] = 70
        s[1::4][(r[1::4] >= 0.03) & (r[1::4] < 0.04)] = 0x7FFFFFFF
    s.setflags(write=False)
    return s


def _field(n, seed, reach):
    """reach 4: vectors of -4..4; reach 128: a quarter of the blocks over the full int8 range, the others -1..1."""
    rs = np.random.RandomState(seed)
    small = rs.randint(-min(reach, 1 if reach > 4 else 4), min(reach, 1 if reach > 4 else 4) + 1, (n - 1, 8, 8, 2))
    if reach <= 4:
        return small.astype(np.int8)
    wild = rs.randint(-128, 128, (n - 1, 8, 8, 2))
    return np.where(rs.rand(n - 1, 8, 8, 1) < 0.25, wild, small).astype(np.int8)


# ---------------------------------------------------------------- 1. the by-hand cases and the smallest shapes
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_by_hand(case):
    labels, bwd, milli, K, G, want = case()
    tr, host = _tracks(labels, bwd, milli, K, G)
    assert (host["gap"] > 1).any()
    got = _host(objects.fill(_up(labels), tr, motion=None if bwd is None else _up(bwd, np.int8), max_objects=K, want_rgb=True))
    _same(got, {k: np.asarray(v, dtype=np.int32) for k, v in want.items()}, K, case.__name__)


def test_one_frame():
    for h, w, K in ((1, 1, 1), (5, 7, 2), (64, 64, 64)):
        s = np.arange(h * w, dtype=np.int32).reshape(1, h, w) % 4 - 1           # -1, 0, 1, 2
        want = _check(s, None, 500, K, 8)
        np.testing.assert_array_equal(want["labels"], s)
        assert not want["totals"].any() and not want["age"].any()
    s = _stack(1)
    got = _raw(s, np.zeros((0, 8, 8, 2), dtype=np.int8), 64, 3, *np.zeros((3, 1, 64), dtype=np.int32))
    np.testing.assert_array_equal(got["labels"], s)


def test_three_small_frames():
    s = np.zeros((3, 5, 7), dtype=np.int32)
    s[0, 1:4, 0:3] = s[2, 1:4, 0:3] = 1
    s[0, 0:2, 5:7] = s[2, 0:2, 5:7] = 2
    s[1, 4, 6] = -5
    want = _check(s, None, 500, 2, 1)
    assert want["totals"].tolist() == [2, 13, 0, 0] and want["age"][1].tolist() == [1, 1]
    s[1, 4, 3] = 1                                                          # one label left: the second candidate is dropped
    assert _check(s, None, 500, 2, 1)["totals"].tolist() == [1, 9, 1, 0]


def _every_gap(n=12):
    """Row r holds an object that is seen twice, r + 2 frames apart: from frame 0 on the even rows, up to frame n - 1 on the odd."""
    s = np.zeros((n, 8, 5), dtype=np.int32)
    for r in range(8):
        a = 0 if r % 2 == 0 else n - 1 - (r + 2)
        s[a, r, 1:4] = s[a + r + 2, r, 1:4] = r + 1
    return s


def test_every_gap_at_the_ends_of_the_stack():
    s = _every_gap()
    _, host = _tracks(s, None, 500, 64, 8)
    assert sorted(host["gap"][host["gap"] > 0].tolist()) == list(range(2, 10))
    want = _check(s, None, 500, 64, 8)
    assert want["totals"].tolist() == [sum(range(1, 9)), 3 * sum(range(1, 9)), 0, 0]
    assert want["age"].max() == 8 and (want["age"][1] > 0).sum() == 4          # m < j: frame 1 is filled from frame 0 alone
    assert (want["labels"][:, 0, 1:4] > 0).all(axis=1).tolist() == [True] * 3 + [False] * 9
    for G in (1, 4):                                                        # shorter tracks of the same stack
        assert _check(s, None, 500, 64, G)["totals"].tolist() == [sum(range(1, G + 1)), 3 * sum(range(1, G + 1)), 0, 0]


# ---------------------------------------------------------------- 2. 64 x 64, K = 64
@pytest.mark.parametrize("G", [1, 3, 8])
def test_flickering_blobs(G):
    want = _check(_stack(24), None, 300, 64, G)
    assert want["totals"][0] > 200 and want["totals"][1] > 200 * 30 and want["age"].max() >= min(G, 4)


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("reach", [4, 128])
def test_fields(reach, G):
    n = 18
    want = _check(_stack(n, seed=1, cell=16), _field(n, 40 + reach, reach), 100, 64, G)
    assert want["totals"][0] > 20 and want["age"].max() == min(G, 3)


def test_labels_above_K_and_below_zero():
    s = _stack(16, seed=2, cell=16, junk=True)
    assert (s == 70).any() and (s < 0).any() and (s == 0x7FFFFFFF).any()
    want = _check(s, None, 300, 64, 3)
    filled = want["labels"] != s
    assert want["totals"][0] > 0 and want["totals"][2] > 0                   # a frame that holds a 70 has no label left
    assert (s[filled] <= 0).all() and (s[filled] < 0).any() and not filled[(s == 70).any(axis=(1, 2))].any()
    want = _check(s, _field(16, 7, 4), 100, 64, 3)
    assert want["totals"][0] > 0


def test_fewer_labels_than_objects():
    s = _stack(16, seed=3, cell=16)
    assert s.max() > 5
    for K in (5, 12):
        want = _check(s, None, 300, K, 3)
        assert want["totals"][2] > 0 and (want["labels"] <= np.maximum(K, s)).all()
    assert _check(s, _field(16, 9, 4), 100, 12, 8)["totals"][2] > 0


# ---------------------------------------------------------------- 3. what the entry promises
def test_a_zero_field_is_no_field():
    s = _stack(16, seed=4, cell=16)
    _, host = _tracks(s, None, 300, 64, 3)
    a = _raw(s, None, 64, 3, host["prev"], host["gap"], host["track"])
    b = _raw(s, np.zeros((15, 8, 8, 2), dtype=np.int8), 64, 3, host["prev"], host["gap"], host["track"])
    assert a["totals"][0] > 0
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_inputs_stay_and_two_calls_agree():
    s, bwd = _stack(16, seed=5, cell=16), _field(16, 11, 4)
    labels, field = _up(s), _up(bwd, np.int8)
    tr = objects.track(labels, iou=0.1, max_objects=64, max_gap=8, motion=field)
    keep = [t.clone() for t in (labels, field, tr.prev, tr.gap, tr.track)]
    first = _host(objects.fill(labels, tr, motion=field, want_rgb=True))
    second = _host(objects.fill(labels, tr, motion=(field, field), want_rgb=True))
    assert first["totals"][0] > 0
    for key in first:
        np.testing.assert_array_equal(first[key], second[key], err_msg=key)
    for was, now in zip(keep, (labels, field, tr.prev, tr.gap, tr.track)):
        assert torch.equal(was, now)


def test_without_a_table():
    s = _stack(16, seed=4, cell=16)
    tr, host = _tracks(s, None, 300, 64, 3)
    want = ref.fill(s, None, host["prev"], host["gap"], host["track"], 64, 3)
    got = _raw(s, None, 64, 3, host["prev"], host["gap"], host["track"], table=False)
    assert (got.pop("table") == JUNK).all() and want["table"].any()
    _same(got, want, 64)
    fl = objects.fill(_up(s), tr, want_table=False)
    assert fl.table is None and fl.rgb is None
    _same(_host(fl), want, 64)


@pytest.mark.parametrize("seed", [0, 1])
def test_any_content_of_prev_gap_and_track(seed):
    """Whatever the three tables hold, the entry reads and writes inside its arrays and gives what the rule says: half of the entries
    are small numbers around the ranges, half any int32."""
    n, K, G = 12, 64, 8
    s, bwd = _stack(n, seed=6 + seed, cell=16, junk=True), _field(n, 20 + seed, 128)
    rs = np.random.RandomState(seed)
    def table(lo, hi):
        small, wild = rs.randint(lo, hi, (n, K)), rs.randint(-2 ** 31, 2 ** 31, (n, K), dtype=np.int64)
        return np.where(rs.rand(n, K) < 0.5, small, wild).astype(np.int32)
    prev, gap, track = table(-2, 70), table(-1, 12), table(-5, 500)
    for field in (None, bwd):
        want = ref.fill(s, field, prev, gap, track, K, G)
        print(f"seed {seed} field {field is not None}: totals {want['totals'].tolist()}")
        assert want["totals"][0] > 0 and want["totals"][3] > 0
        _same(_raw(s, field, K, G, prev, gap, track), want, K, f"field {field is not None}")
    small = np.where(rs.rand(n, 9, 13) < 0.6, 0, rs.randint(-1, 6, (n, 9, 13))).astype(np.int32)      # an odd size
    prev, gap, track = rs.randint(-1, 9, (n, 7)), rs.randint(-1, 5, (n, 7)), table(-5, 500)[:, :7]
    want = ref.fill(small, None, prev, gap, track, 7, 2)
    assert want["totals"][0] > 0 and want["totals"][3] > 0
    _same(_raw(small, None, 7, 2, prev, gap, track), want, 7, "9 x 13")


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    n, K = 4, 8
    labels, bwd = _up(_stack(n)), _up(np.zeros((n - 1, 8, 8, 2)), np.int8)
    small = _up(np.zeros((n, 5, 7)))
    ins = {k: _up(np.zeros((n, K))) for k in ("prev", "gap", "track")}
    full = lambda *shape: torch.full(shape, JUNK, dtype=torch.int32, device=DEV)
    outs = {"out_labels": full(n, 64, 64), "out_track": full(n, K), "age": full(n, K), "table": full(n, K, 8), "totals": full(4)}
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=n, h=64, w=64, K=K, G=2, shift=None, **over):
        p = {k: v.data_ptr() for k, v in {**ins, **outs}.items()}
        p.update(labels=labels.data_ptr(), bwd=bwd.data_ptr())
        if shift:
            p[shift] += 2
        p.update(over)
        return lib.cgs_objects_track_fill(p["labels"], p["bwd"], n, h, w, K, G, p["prev"], p["gap"], p["track"], p["out_labels"], p["out_track"],
                                          p["age"], p["table"], p["totals"], stream)

    bad, unsupported = _lib.ERR_BADARG, _lib.ERR_UNSUPPORTED
    assert call(G=0) == bad and call(G=9) == bad and call(n=0) == bad and call(h=0) == bad and call(w=0) == bad and call(K=0) == bad
    for name in ("labels", "prev", "gap", "track", "out_labels", "out_track", "age", "table", "totals"):
        assert call(shift=name) == bad, name
    for name in ("labels", "prev", "gap", "track", "out_labels", "out_track", "age", "totals"):
        assert call(**{name: None}) == bad, name
    assert call(out_labels=labels.data_ptr()) == bad
    assert call(K=65) == unsupported and call(n=(1 << 17) + 1) == unsupported
    assert call(h=32) == unsupported and call(w=63) == unsupported              # a field needs 64 x 64
    assert call(h=65, bwd=None) == unsupported and call(w=65, bwd=None) == unsupported
    torch.cuda.synchronize()
    assert all((v == JUNK).all() for v in outs.values())
    assert call() == 0 and call(bwd=None, labels=small.data_ptr(), h=5, w=7) == 0      # and calls with nothing wrong run
    torch.cuda.synchronize()
    assert not outs["totals"].any().item()
