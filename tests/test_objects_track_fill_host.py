"""CPU checks of --track-fill: the two forms of the checker in tests/objects_track_fill_ref.py against each other, the by-hand cases
with their expected arrays written out (tests/test_gpu_objects_track_fill.py runs the same cases on the kernel), every refusal of the
flag, the Python argument errors that come before the GPU, and the new symbol and source."""
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
from cgs_amd import _lib, build, cli, objects  # noqa: E402

KEYS = ("labels", "track", "age", "table", "totals")


def _flicker(seed, n=8, cell=16):
    """Small flicker stacks at 64 x 64: a grid of blobs, each shifted by -2..2 cells and absent from a third of the frames."""
    rs = np.random.RandomState(seed)
    per = 64 // cell
    s = np.zeros((n, 68, 68), dtype=np.int32)
    for f in range(n):
        for i in range(per * per):
            if rs.rand() < 1 / 3:
                continue
            y, x = 2 + (i // per) * cell + rs.randint(-2, 3), 2 + (i % per) * cell + rs.randint(-2, 3)
            s[f, y:y + cell - 3, x:x + cell - 3] = i + 1
    return s[:, 2:-2, 2:-2].copy()


def _both(labels, bwd, milli, K, G):
    """(tracks, fill) of the checker, the plain form held against the vectorised one."""
    t = ref.tracked(labels, bwd, milli, K, G)
    fast = ref.fill(labels, bwd, t["prev"], t["gap"], t["track"], K, G)
    slow = ref.fill_plain(labels, bwd, t["prev"], t["gap"], t["track"], K, G)
    for key in KEYS:
        np.testing.assert_array_equal(fast[key], slow[key], err_msg=key)
    return t, fast


def test_the_plain_and_the_vectorised_checker_agree():
    s = _flicker(3, n=6)[:, ::1, ::1]
    small = s[:, :24, :40].copy()
    _, a = _both(small, None, 300, 16, 2)
    assert a["totals"][0] > 0
    rs = np.random.RandomState(5)
    bwd = rs.randint(-4, 5, (len(s) - 1, 8, 8, 2)).astype(np.int8)
    t, b = _both(s[:5], bwd[:4], 200, 16, 3)
    assert t["gap_links"][1:].sum() > 0
    wild = rs.randint(-128, 128, (4, 8, 8, 2)).astype(np.int8)
    junk = {k: rs.randint(-3, 12, t[k].shape).astype(np.int32) for k in ("prev", "gap", "track")}
    fast = ref.fill(s[:5], wild, junk["prev"], junk["gap"], junk["track"], 16, 3)
    slow = ref.fill_plain(s[:5], wild, junk["prev"], junk["gap"], junk["track"], 16, 3)
    for key in KEYS:
        np.testing.assert_array_equal(fast[key], slow[key], err_msg=key)
    assert fast["totals"].sum() > 0


# ---------------------------------------------------------------- the by-hand cases: (labels, bwd, milli, K, G, expected)
def case_static_blob():
    s = np.zeros((3, 4, 5), dtype=np.int32)
    s[0, 1:3, 1:3] = s[2, 1:3, 1:3] = 1
    want = s.copy()
    want[1] = [[0, 0, 0, 0, 0], [0, 1, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
    track, age, table = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int32), np.zeros((3, 4, 8), np.int32)
    track[:, 0] = 1
    age[1, 0] = 1
    table[1, 0] = [4, 1, 1, 2, 2, 6, 6, 6]
    return s, None, 500, 4, 1, {"labels": want, "track": track, "age": age, "table": table, "totals": [1, 4, 0, 0]}


def case_shifted_blob():
    s = np.zeros((3, 64, 64), dtype=np.int32)
    s[0, 10:14, 10:14] = s[2, 10:14, 16:20] = 1
    bwd = np.zeros((2, 8, 8, 2), dtype=np.int8)
    bwd[...] = (0, -3)                                                      # the scene moves 3 cells right a frame
    want = s.copy()
    want[1, 10:14, 13:17] = 1
    track, age, table = np.zeros((3, 64), np.int32), np.zeros((3, 64), np.int32), np.zeros((3, 64, 8), np.int32)
    track[:, 0] = 1
    age[1, 0] = 1
    table[1, 0] = [16, 13, 10, 16, 13, 4 * (13 + 14 + 15 + 16), 4 * (10 + 11 + 12 + 13), 10 * 64 + 13]
    return s, bwd, 500, 64, 1, {"labels": want, "track": track, "age": age, "table": table, "totals": [1, 16, 0, 0]}


def case_real_object_keeps_its_cells():
    s = np.zeros((3, 4, 6), dtype=np.int32)
    s[0, 1:3, 1:3] = s[2, 1:3, 1:3] = 1
    s[1, :, 2:4] = 1                                                        # 8 cells, 2 of them the blob's: IoU 2 / 10 with it
    want = s.copy()
    want[1] = [[0, 0, 1, 1, 0, 0], [0, 2, 1, 1, 0, 0], [0, 2, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0]]
    track, age, table = np.zeros((3, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros((3, 3, 8), np.int32)
    track[0, 0] = track[2, 0] = 1
    track[1] = [2, 1, 0]
    age[1, 1] = 1
    table[1, 1] = [2, 1, 1, 1, 2, 2, 3, 7]
    return s, None, 500, 3, 1, {"labels": want, "track": track, "age": age, "table": table, "totals": [1, 2, 0, 0]}


def case_the_smaller_j_wins():
    s = np.zeros((4, 3, 6), dtype=np.int32)
    s[0, 1, 0:4] = 1                                                        # A
    s[1, 1:3, 3:6] = 1                                                      # B: shares (1, 3) with A, IoU 1 / 9
    s[3, 1, 0:3] = 1                                                        # A again, a cell short: 3 / 4
    s[3, 1:3, 3:6] = 2                                                      # B again
    want = s.copy()
    want[1] = [[0, 0, 0, 0, 0, 0], [2, 2, 2, 1, 1, 1], [0, 0, 0, 1, 1, 1]]   # A carried one frame, beside the real B
    want[2] = [[0, 0, 0, 0, 0, 0], [2, 2, 2, 1, 1, 1], [0, 0, 0, 1, 1, 1]]   # B from one frame back takes (1, 3), A from two the rest
    track, age, table = np.zeros((4, 3), np.int32), np.zeros((4, 3), np.int32), np.zeros((4, 3, 8), np.int32)
    track[0] = [1, 0, 0]
    track[1] = [2, 1, 0]
    track[2] = [2, 1, 0]
    track[3] = [1, 2, 0]
    age[1] = [0, 1, 0]
    age[2] = [1, 2, 0]
    table[1, 1] = [3, 0, 1, 2, 1, 3, 3, 6]
    table[2, 0] = [6, 3, 1, 5, 2, 24, 9, 9]
    table[2, 1] = [3, 0, 1, 2, 1, 3, 3, 6]
    return s, None, 500, 3, 2, {"labels": want, "track": track, "age": age, "table": table, "totals": [3, 12, 0, 0]}


def case_a_full_frame_drops_every_candidate():
    s = np.zeros((3, 4, 5), dtype=np.int32)
    s[0, 1:3, 1:3] = s[2, 1:3, 1:3] = 1
    s[1, 3, 4] = 2                                                          # base == K
    track = np.zeros((3, 2), np.int32)
    track[0, 0] = track[2, 0] = 1
    track[1, 1] = 2
    return s, None, 500, 2, 1, {"labels": s.copy(), "track": track, "age": np.zeros((3, 2), np.int32), "table": np.zeros((3, 2, 8), np.int32),
                                "totals": [0, 0, 1, 0]}


def case_one_label_left_for_two_candidates():
    s = np.zeros((3, 4, 7), dtype=np.int32)
    s[0, 0:2, 0:2] = s[2, 0:2, 0:2] = 1
    s[0, 2:4, 3:5] = s[2, 2:4, 3:5] = 2
    s[1, 0, 6] = 2                                                          # base == K - 1
    want = s.copy()
    want[1, 0:2, 0:2] = 3                                                   # (1, 1) comes before (1, 2)
    track, age, table = np.zeros((3, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros((3, 3, 8), np.int32)
    track[0] = track[2] = [1, 2, 0]
    track[1] = [0, 3, 1]
    age[1, 2] = 1
    table[1, 2] = [4, 0, 0, 1, 1, 2, 2, 0]
    return s, None, 500, 3, 1, {"labels": want, "track": track, "age": age, "table": table, "totals": [1, 4, 1, 0]}


def case_carried_out_of_the_grid():
    s = np.zeros((3, 64, 64), dtype=np.int32)
    s[0, 10:14, 2:6] = s[2, 10:14, 2:6] = 1
    bwd = np.zeros((2, 8, 8, 2), dtype=np.int8)
    bwd[1] = (0, 70)                                                        # two steps add up to nothing: the link holds,
    bwd[0] = (0, -70)                                                       # one step reads 70 cells to the left of every cell
    track = np.zeros((3, 64), np.int32)
    track[0, 0] = track[2, 0] = 1
    return s, bwd, 500, 64, 1, {"labels": s.copy(), "track": track, "age": np.zeros((3, 64), np.int32),
                                "table": np.zeros((3, 64, 8), np.int32), "totals": [0, 0, 0, 1]}


CASES = [case_static_blob, case_shifted_blob, case_real_object_keeps_its_cells, case_the_smaller_j_wins,
         case_a_full_frame_drops_every_candidate, case_one_label_left_for_two_candidates, case_carried_out_of_the_grid]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_by_hand(case):
    labels, bwd, milli, K, G, want = case()
    t = ref.tracked(labels, bwd, milli, K, G)
    assert t["gap_links"][1:].sum() > 0, "the case needs a bridged link"
    for form in (ref.fill, ref.fill_plain):
        got = form(labels, bwd, t["prev"], t["gap"], t["track"], K, G)
        for key in KEYS:
            np.testing.assert_array_equal(got[key], np.asarray(want[key], dtype=np.int32), err_msg=f"{form.__name__} {key}")


def test_a_zero_field_is_no_field_and_paint_is_the_trackers():
    s = _flicker(7, n=6)
    t = ref.tracked(s, None, 300, 16, 2)
    a = ref.fill(s, None, t["prev"], t["gap"], t["track"], 16, 2)
    b = ref.fill(s, np.zeros((5, 8, 8, 2), dtype=np.int8), t["prev"], t["gap"], t["track"], 16, 2)
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["totals"][0] > 0
    import objects_track_ref as base
    number, rgb = ref.paint(a["labels"], a["track"], 16)
    np.testing.assert_array_equal(rgb, base.colours(number))
    np.testing.assert_array_equal(objects.track_colours(torch.from_numpy(number)).numpy(), rgb)
    assert (number[s > 0] > 0).all() and (number > 0).sum() == (s > 0).sum() + a["totals"][1]


def test_the_flag_parses_and_is_refused():
    ok = ["-objects", "--track-iou", "0.3", "--track-gap", "2", "--track-fill"]
    assert cli.parse_args(["-process"] + ok).track_fill is True and cli.parse_args(["-eval"] + ok + ["--track-motion", "2"]).track_fill is True
    assert cli.parse_args(["-eval"]).track_fill is False
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3", "--track-gap", "2"]).track_fill is False
    video = ["-process", "--source-video", "a.mp4", "--overlay-video", "b.mp4"]
    for bad, word in ((["-eval", "-objects", "--track-fill"], "--track-iou"), (["-process", "--track-fill"], "--track-iou"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-fill"], "--track-gap"),
                      (["-process", "-objects", "--track-iou", "0.3", "--track-gap", "0", "--track-fill"], "--track-gap"),
                      (["-eval", "--track-iou", "0.3", "--track-gap", "2", "--track-fill"], "-objects"),
                      (video + ["-objects", "--track-iou", "0.3", "--track-gap", "2", "--track-fill"], "--track-fill with --source-video")):
        with pytest.raises((ValueError, SystemExit), match=word):
            cli.parse_args(bad)


def test_python_argument_errors_come_before_the_gpu():
    a = torch.zeros((3, 64, 64), dtype=torch.int32)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    def tracks(K=64, G=2, gap=True):
        return objects.Tracks(z(3, K), z(3, K), z(), z(), z(), z(), z(3 * K, 8), None, None,
                              *((z(3, K), z(G + 1), z(3 * K, 2)) if gap else ()))
    with pytest.raises(ValueError, match="without gap"):
        objects.fill(a, tracks(gap=False))
    with pytest.raises(ValueError, match="max_gap 0"):
        objects.fill(a, tracks(G=0))
    with pytest.raises(ValueError, match="objects.track"):
        objects.fill(a, (1, 2, 3))
    with pytest.raises(ValueError, match="int32"):
        objects.fill(a.float(), tracks())
    with pytest.raises(ValueError, match="tracks.prev"):
        objects.fill(a, tracks(K=32))
    with pytest.raises(ValueError, match="max_objects"):
        objects.fill(a, tracks(), max_objects=65)
    with pytest.raises(ValueError, match="64 x 64"):
        objects.fill(a[:, :32], tracks(), motion=torch.zeros((2, 8, 8, 2), dtype=torch.int8))
    with pytest.raises(ValueError, match="motion"):
        objects.fill(a, tracks(), motion=torch.zeros((3, 8, 8, 2), dtype=torch.int8))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CgsError, match="cgs_objects_track_fill"):
            objects.fill(a, tracks())


def test_the_entry_point_is_exported_and_checks_its_arguments():
    assert "objects_fill.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "objects_fill.hip"))
    assert len(_lib.SIGNATURES["cgs_objects_track_fill"][1]) == 16 and _lib.SIGNATURES["cgs_objects_track_fill"][0] is _lib.i32
    lib = _lib.load()
    assert lib.cgs_objects_track_fill(None, None, 2, 64, 64, 4, 1, *(None,) * 9) == _lib.ERR_BADARG       # NULL pointers: nothing is touched
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        header = fp.read()
    assert "int cgs_objects_track_fill(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects," in header
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        with open(os.path.join(REPO, doc)) as fp:
            text = fp.read()
        assert "cgs_objects_track_fill" in text and "--track-fill" in text, doc


def test_the_report_block():
    z = lambda v: torch.tensor(v, dtype=torch.int32)
    fl = objects.Filled(None, None, None, None, z(5), z(40), z(1), z(2), None)
    assert objects.fill_report(fl) == {"objects": 5, "cells": 40, "dropped": 1, "vanished": 2}
