"""CPU checks of --track-reid: the by-hand cases of the rule of cgs_objects_appearance / cgs_objects_reid with their expected arrays
written out (tests/test_gpu_objects_reid.py runs the same cases on the kernels), held against the checker tests/objects_reid_ref.py on
the reference tracker's tracks; the flag parsing and every refusal of the flag; the Python argument errors that come before the GPU;
the new symbols and source."""
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
import objects_track_gap_ref as track_ref  # noqa: E402
from cgs_amd import _lib, build, cli, objects  # noqa: E402

RED, GREEN, BLUE = (200, 30, 30), (30, 200, 30), (30, 30, 200)
TRACK_MILLI = 500


class Stack:
    """A hand-made stack: put(frame, label, rows, columns, colour) paints a block."""

    def __init__(self, n, h=4, w=4):
        self.frames = np.zeros((n, h, w, 3), dtype=np.uint8)
        self.labels = np.zeros((n, h, w), dtype=np.int32)

    def put(self, f, label, ys, xs, colour):
        self.labels[f, ys[0]:ys[1], xs[0]:xs[1]] = label
        self.frames[f, ys[0]:ys[1], xs[0]:xs[1]] = colour
        return self


TOP, BOTTOM, LEFT, RIGHT = (0, 2), (2, 4), (0, 2), (2, 4)


def _case(stack, want, K=2, G=0, milli=800, W=64, min_area=1, **more):
    return dict(frames=stack.frames, labels=stack.labels, K=K, G=G, milli=milli, W=W, min_area=min_area, want=want, **more)


def _two_tracks(second=RED, gap_frames=4, pixels=RIGHT):
    """Track 1 lives in frames 0..1, track 2 in the two frames `gap_frames` empty frames later, elsewhere in the frame."""
    s = Stack(4 + gap_frames)
    for f in (0, 1):
        s.put(f, 1, TOP, LEFT, RED)
    for f in (2 + gap_frames, 3 + gap_frames):
        s.put(f, 1, BOTTOM, pixels, second)
    return s


def case_one_colour_five_frames_apart():                                  # L_1 = 1, F_2 = 6
    return _case(_two_tracks(), dict(prev=[0, 1], next=[2, 0], sim=[0, 4096], identity=[1, 1], totals=[1, 1, 2, 2]))


def case_another_colour():
    return _case(_two_tracks(second=GREEN), dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]))


def case_overlap_in_time():                                               # track 1 in frames 0..3, track 2 in frames 2..5
    s = Stack(6)
    for f in range(4):
        s.put(f, 1, TOP, LEFT, RED)
    for f in range(2, 6):
        s.put(f, 2 if f < 4 else 1, BOTTOM, RIGHT, RED)
    return _case(s, dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]))


def case_window_reached():                                                # F_2 - L_1 = 5 = W
    return _case(_two_tracks(), dict(prev=[0, 1], next=[2, 0], sim=[0, 4096], identity=[1, 1], totals=[1, 1, 2, 2]), W=5)


def case_window_missed():                                                 # W + 1
    return _case(_two_tracks(), dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]), W=4)


def _half_and_half(reds):
    """Frame 0: one object over the whole 64 x 64 frame, its first `reds` pixels red and the rest green; frame 2: the same object all red."""
    s = Stack(3, 64, 64)
    s.put(0, 1, (0, 64), (0, 64), GREEN)
    s.frames[0].reshape(-1, 3)[:reds] = RED
    s.put(2, 1, (0, 64), (0, 64), RED)
    return s


def case_threshold_met_exactly():                                         # Q_1 = (2048, 2048), Q_2 = (4096): 1000 * 2048 == 500 * 4096
    return _case(_half_and_half(2048), dict(prev=[0, 1], next=[2, 0], sim=[0, 2048], identity=[1, 1], totals=[1, 1, 2, 2]), K=1, milli=500)


def case_threshold_missed_by_one():                                       # s = 2047
    return _case(_half_and_half(2047), dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]), K=1, milli=500)


def case_threshold_one_thousandth_higher():
    return _case(_half_and_half(2048), dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]), K=1, milli=501)


def case_tie_of_successors():                                             # tracks 2 and 3 both start in frame 2: succ[1] = 2
    s = Stack(3).put(0, 1, TOP, LEFT, RED).put(2, 1, TOP, RIGHT, RED).put(2, 2, BOTTOM, LEFT, RED)
    return _case(s, dict(prev=[0, 1, 0], next=[2, 0, 0], sim=[0, 4096, 0], identity=[1, 1, 2], totals=[2, 1, 3, 2]), ties=True)


def case_tie_of_predecessors():                                           # tracks 1 and 2 both end in frame 0: pred[3] = 1
    s = Stack(3).put(0, 1, TOP, RIGHT, RED).put(0, 2, BOTTOM, LEFT, RED).put(2, 1, TOP, LEFT, RED)
    return _case(s, dict(prev=[0, 0, 1], next=[3, 0, 0], sim=[0, 0, 4096], identity=[1, 2, 1], totals=[2, 1, 3, 2]), ties=True)


def case_not_mutual():
    """Track 1 (three red cells, one green) has track 3 as its best and only successor, but track 3's best predecessor is the all-red
    track 2: exactly one link, 2 -> 3."""
    s = Stack(3).put(0, 1, TOP, LEFT, RED).put(0, 2, BOTTOM, RIGHT, RED).put(2, 1, TOP, RIGHT, RED)
    s.frames[0, 0, 0] = GREEN
    return _case(s, dict(prev=[0, 0, 2], next=[0, 3, 0], sim=[0, 0, 4096], identity=[1, 2, 2], totals=[2, 1, 3, 2]), milli=500,
                 admissible=[(1, 3, 3072), (2, 3, 4096)])


def case_chain_of_three():                                                # frames 0, 2, 4; W = 2 leaves 1 -> 2 and 2 -> 3
    s = Stack(5).put(0, 1, TOP, LEFT, RED).put(2, 1, TOP, RIGHT, RED).put(4, 1, BOTTOM, LEFT, RED)
    return _case(s, dict(prev=[0, 1, 2], next=[2, 3, 0], sim=[0, 4096, 4096], identity=[1, 1, 1], totals=[1, 2, 3, 3]), W=2)


def case_small_track_is_left_out():                                       # track 2 has one pixel, min_area 2
    s = Stack(3).put(0, 1, TOP, LEFT, RED).put(2, 1, (3, 4), (3, 4), RED)
    return _case(s, dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 1, 1]), min_area=2)


def _bin_edge(channel, value):
    lo, hi = [0, 0, 0], [0, 0, 0]
    lo[channel], hi[channel] = value, value + 1
    s = Stack(3).put(0, 1, TOP, LEFT, tuple(lo)).put(2, 1, TOP, RIGHT, tuple(hi))
    shift = (4, 2, 0)[channel]
    return _case(s, dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]),
                 bins=[(value >> 6) << shift, ((value + 1) >> 6) << shift])


def case_bin_edge_63_64():
    return _bin_edge(0, 63)


def case_bin_edge_127_128():
    return _bin_edge(1, 127)


def case_bin_edge_191_192():
    return _bin_edge(2, 191)


def case_missed_frames_make_an_overlap():
    """Track 1 is seen in frames 0 and 2 (bridged at G = 1: length 2, missed 1, so L_1 = 2); track 2 starts in frame 2.  Without the
    missed frame L_1 would be 1 and 1 -> 2 a candidate."""
    s = Stack(4).put(0, 1, TOP, LEFT, RED).put(2, 1, TOP, LEFT, RED).put(2, 2, BOTTOM, RIGHT, RED).put(3, 1, BOTTOM, RIGHT, RED)
    return _case(s, dict(prev=[0, 0], next=[0, 0], sim=[0, 0], identity=[1, 2], totals=[2, 0, 2, 1]), G=1, without_extra_links=True)


CASES = [case_one_colour_five_frames_apart, case_another_colour, case_overlap_in_time, case_window_reached, case_window_missed,
         case_threshold_met_exactly, case_threshold_missed_by_one, case_threshold_one_thousandth_higher, case_tie_of_successors,
         case_tie_of_predecessors, case_not_mutual, case_chain_of_three, case_small_track_is_left_out, case_bin_edge_63_64,
         case_bin_edge_127_128, case_bin_edge_191_192, case_missed_frames_make_an_overlap]


def check_case(c, got, rows):
    """got: prev, next, sim, identity (arrays of `rows` entries) and totals, from the checker or the kernels, against the case's arrays."""
    want = c["want"]
    n = len(want["identity"])
    for key in ("prev", "next", "sim", "identity"):
        full = np.zeros(rows, dtype=np.int64)
        full[:n] = want[key]
        np.testing.assert_array_equal(np.asarray(got[key]).astype(np.int64), full, err_msg=key)
    assert [int(v) for v in got["totals"]] == want["totals"]


def checker(c):
    """(the reference tracker's tracks, S, H, the checker's result) of a case."""
    t = track_ref.track(c["labels"], TRACK_MILLI, c["K"], c["G"])
    S, H = ref.appearance(c["frames"], c["labels"], t["track"], c["K"])
    r = ref.reid(t["table"], t["extra"] if c["G"] else None, S, t["totals"][0], c["milli"], c["W"], c["min_area"])
    return t, S, H, r


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_by_hand(case):
    c = case()
    t, S, H, r = checker(c)
    assert t["totals"][0] == len(c["want"]["identity"])                    # the tracks are the ones the case speaks of
    check_case(c, r, t["table"].shape[0])
    if "bins" in c:
        assert [int(np.flatnonzero(r["Q"][k])[0]) for k in range(2)] == c["bins"] and c["bins"][0] != c["bins"][1]
    if "admissible" in c:
        assert r["admissible"] == c["admissible"]
    if c.get("ties"):
        assert r["ties"] > 0
    if c.get("without_extra_links"):
        assert t["extra"][0].tolist() == [1, 1]
        assert ref.reid(t["table"], None, S, t["totals"][0], c["milli"], c["W"], c["min_area"])["totals"][1] == 1
    eligible = r["totals"][2]
    D = r["Q"].sum(axis=1)
    assert np.count_nonzero(D) == eligible and all(4033 <= d <= 4096 for d in D[D > 0])
    np.testing.assert_array_equal(ref.appearance(c["frames"], c["labels"], None, c["K"])[1], H)


def test_signature_needs_64_bits_only_in_the_track_sum():
    S = np.zeros((2, 64), dtype=np.int64)
    S[0, 5], S[0, 9] = 600 * 4096 - 7, 7                                   # a full-frame object that lives 600 frames
    Q, D = ref.signatures(S, 2, 1)
    assert Q[0, 5] == 4095 and Q[0, 9] == 0 and D == [4095, 0] and int(S[0, 5]) * 4096 > 2 ** 32


def test_object_identities():
    got = ref.object_identities([[1, 0, 3], [2, 9, -1]], [5, 6, 7])
    assert got.tolist() == [[5, 0, 7], [6, 0, 0]]
    same = objects.identities(torch.tensor([[1, 0, 3], [2, 9, -1]], dtype=torch.int32), torch.tensor([5, 6, 7], dtype=torch.int32))
    assert same.dtype == torch.int32 and same.tolist() == got.tolist()


# ---------------------------------------------------------------- the flags
def test_parsers():
    assert objects.parse_track_reid("0.8") == 0.8 and objects.parse_track_reid(" 1 ") == 1.0 and objects.parse_track_reid("0.001") == 0.001
    for bad in ("", "x", "0", "-0.5", "1.001", "0.8005", "nan", "inf", "0.5-0.6"):
        with pytest.raises(ValueError, match="--track-reid"):
            objects.parse_track_reid(bad)
    assert objects.parse_track_reid_window("1") == 1 and objects.parse_track_reid_window("1024") == 1024
    for bad in ("", "0", "1025", "2.5", "-3", "w"):
        with pytest.raises(ValueError, match="--track-reid-window"):
            objects.parse_track_reid_window(bad)
    assert objects.parse_track_reid_area("1") == 1 and objects.parse_track_reid_area("4096") == 4096
    for bad in ("", "0", "-1", "1.5", "a", str(2 ** 31)):
        with pytest.raises(ValueError, match="--track-reid-area"):
            objects.parse_track_reid_area(bad)
    assert (objects.REID_SIM, objects.REID_WINDOW, objects.REID_MIN_AREA, objects.REID_BINS) == (0.8, 64, 64, 64)
    assert (objects.REID_MAX_WINDOW, objects.REID_MAX_FRAMES) == (1024, 1 << 14)


BASE = ["--model", "m", "-process", "-objects", "--track-iou", "0.5"]


def test_flags_accepted():
    a = cli.parse_args(BASE + ["--track-reid", "0.9"])
    assert (a.track_reid, a.track_reid_window, a.track_reid_area) == (0.9, 64, 64)
    a = cli.parse_args(BASE + ["--track-reid", "0.75", "--track-reid-window", "256", "--track-reid-area", "10", "--track-gap", "2",
                               "--track-motion", "2", "--track-fill", "-crf", "--clean", "open=1"])
    assert (a.track_reid, a.track_reid_window, a.track_reid_area) == (0.75, 256, 10)
    a = cli.parse_args(["--model", "m", "-eval", "-objects", "--track-iou", "0.5", "--match-iou", "0.5", "--track-reid", "1"])
    assert a.track_reid == 1.0
    a = cli.parse_args(BASE)
    assert a.track_reid is None and a.track_reid_window is None and a.track_reid_area is None


@pytest.mark.parametrize("argv, text", [
    (["--model", "m", "-process", "-objects", "--track-reid", "0.8"], "--track-reid belongs to --track-iou"),
    (BASE + ["--track-reid-window", "16"], "--track-reid-window belong to --track-reid"),
    (BASE + ["--track-reid-area", "16"], "--track-reid-area belong to --track-reid"),
    (BASE + ["--track-reid-window", "16", "--track-reid-area", "16"], "--track-reid-window / --track-reid-area belong to --track-reid"),
    (BASE + ["--track-reid", "0"], "--track-reid '0'"),
    (BASE + ["--track-reid", "1.5"], "--track-reid '1.5'"),
    (BASE + ["--track-reid", "0.8125"], "thousandths"),
    (BASE + ["--track-reid", "high"], "--track-reid 'high'"),
    (BASE + ["--track-reid", "0.8", "--track-reid-window", "0"], "--track-reid-window 0"),
    (BASE + ["--track-reid", "0.8", "--track-reid-window", "1025"], "--track-reid-window 1025"),
    (BASE + ["--track-reid", "0.8", "--track-reid-window", "x"], "--track-reid-window 'x'"),
    (BASE + ["--track-reid", "0.8", "--track-reid-area", "0"], "--track-reid-area 0"),
    (BASE + ["--track-reid", "0.8", "--track-reid-area", "1.5"], "--track-reid-area '1.5'"),
    (["--model", "m", "-process", "--track-iou", "0.5", "--track-reid", "0.8"], "belong to -objects"),
    (["--model", "m", "-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--track-iou", "0.5", "--track-reid", "0.8"],
     "--track-reid with --source-video"),
])
def test_flags_refused(argv, text):
    with pytest.raises(ValueError, match=text.replace("(", r"\(")):
        cli.parse_args(argv)


# ---------------------------------------------------------------- the Python layer, before the GPU
def _tracks(n=3, K=2, rows=None, extra=False):
    rows = n * K if rows is None else rows
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    return objects.Tracks(z(n, K), z(n, K), z(1)[0], z(1)[0], z(1)[0], z(1)[0], z(rows, 8), None, None, z(n, K) if extra else None,
                          z(1) if extra else None, z(rows, 2) if extra else None)


def test_appearance_argument_errors():
    frames, labels = torch.zeros((3, 4, 5, 3), dtype=torch.uint8), torch.zeros((3, 4, 5), dtype=torch.int32)
    for args, kw, text in [((frames.float(), labels), {}, "frames must be torch.uint8"),
                           ((frames, labels.long()), {}, "labels must be torch.int32"),
                           ((frames.numpy(), labels), {}, "frames must be a torch tensor"),
                           ((frames[:, :, :4], labels), {}, r"labels must be \[n,h,w\] and frames \[n,h,w,3\]"),
                           ((frames[0], labels[0]), {}, r"labels must be \[n,h,w\]"),
                           ((torch.zeros((1, 65, 4, 3), dtype=torch.uint8), torch.zeros((1, 65, 4), dtype=torch.int32)), {}, "1..64 x 1..64"),
                           ((frames, labels), {"max_objects": 65}, "max_objects must be 1..64"),
                           ((frames, labels), {"max_objects": 2, "tracks": "t"}, "tracks must be the result of objects.track"),
                           ((frames, labels), {"max_objects": 3, "tracks": _tracks()}, r"tracks.track must be int32 \[3,3\]")]:
        with pytest.raises(ValueError, match=text):
            objects.appearance(*args, **kw)
    with pytest.raises(_lib.CgsError, match="cgs_objects_appearance"):
        objects.appearance(frames, labels, _tracks(), max_objects=2)


def test_reid_argument_errors():
    tr = _tracks()
    ap = objects.Appearance(torch.zeros((6, 64), dtype=torch.int32), None)
    for args, kw, text in [(("t", ap, 3), {}, "tracks must be the result of objects.track"),
                           ((tr, objects.Appearance(None, None), 3), {}, "appearance must be the result of objects.appearance"),
                           ((tr, ap, 0), {}, "n_frames must be 1..16384"),
                           ((tr, ap, (1 << 14) + 1), {}, "n_frames must be 1..16384"),
                           ((tr, ap, 4), {}, r"tracks.track must be \[4,K\]"),
                           ((_tracks(rows=5), objects.Appearance(torch.zeros((5, 64), dtype=torch.int32), None), 3), {},
                            "a truncated table cannot be re-identified"),
                           ((tr, objects.Appearance(torch.zeros((5, 64), dtype=torch.int32), None), 3), {}, r"appearance.track_hist must be int32 \[6,64\]"),
                           ((tr, ap, 3), {"sim": 0}, "outside"), ((tr, ap, 3), {"sim": 1.5}, "outside"),
                           ((tr, ap, 3), {"sim": 0.8125}, "thousandths"), ((tr, ap, 3), {"sim": "0.8"}, "one number"),
                           ((tr, ap, 3), {"window": 0}, "window must be 1..1024"), ((tr, ap, 3), {"window": 1025}, "window must be 1..1024"),
                           ((tr, ap, 3), {"window": 2.5}, "whole number"), ((tr, ap, 3), {"min_area": 0}, "min_area must be at least 1")]:
        with pytest.raises(ValueError, match=text):
            objects.reid(*args, **kw)
    with pytest.raises(_lib.CgsError, match="cgs_objects_reid"):
        objects.reid(tr, ap, 3)


def test_reid_report_and_identity_rows():
    table = np.zeros((6, 8), dtype=np.int32)
    table[:3, 0], table[:3, 2] = [0, 2, 9], [2, 3, 1]                       # frames 0..1, 2..4 (one missed: ..5), 9
    extra = np.zeros((6, 2), dtype=np.int32)
    extra[1] = [1, 1]
    rd = objects.Reid(np.array([0, 0, 2, 0, 0, 0]), np.array([0, 3, 0, 0, 0, 0]), np.array([0, 0, 4000, 0, 0, 0]),
                      np.array([1, 2, 2, 0, 0, 0]), None, 2, 1, 3, 2)
    rep = objects.reid_report(rd, table, extra, 0.8, 64, 64)
    assert rep == {"sim": 0.8, "window": 64, "min_area": 64, "bins": 64, "eligible": 3, "links": 1, "identities": 2, "longest": 2,
                   "link_gaps": {"1": 0, "2": 0, "3-4": 1, "5-8": 0, "9-16": 0, "17-32": 0, "33+": 0}}
    assert objects.reid_report(rd, table, None, 0.8, 64, 64)["link_gaps"]["5-8"] == 1
    with pytest.raises(ValueError, match="links"):
        objects.reid_report(rd._replace(n_links=2), table, extra)
    rows = objects.identity_rows(rd.identity, rd.prev, 3, ["a", "c", "j"], ["b", "f", "j"], [2, 3, 1])
    assert rows == [{"identity": 1, "tracks": [1], "first": "a", "last": "b", "objects": 2},
                    {"identity": 2, "tracks": [2, 3], "first": "c", "last": "j", "objects": 4}]


def test_the_source_and_the_symbols_are_registered():
    assert "objects_reid.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "objects_reid.hip"))
    for name in ("cgs_objects_appearance", "cgs_objects_reid", "cgs_objects_reid_scratch_bytes"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_objects_appearance"][1]) == 11 and len(_lib.SIGNATURES["cgs_objects_reid"][1]) == 18
    header = open(os.path.join(REPO, "include", "cgs_hip.h")).read()
    for name in ("cgs_objects_appearance(", "cgs_objects_reid(", "cgs_objects_reid_scratch_bytes(", "CGS_OBJ_REID_MAX_WINDOW = 1024",
                 "CGS_OBJ_REID_MAX_FRAMES = 1 << 14", "CGS_OBJ_REID_BINS = 64"):
        assert name in header


# ---------------------------------------------------------------- the generated stack (tests/test_gpu_objects_reid.py tracks it on the GPU)
PALETTE = ((224, 32, 32), (32, 224, 32), (32, 32, 224), (224, 224, 32), (160, 96, 32), (96, 160, 224))     # bin centres
STRADDLER, SEED = 5, 12
GENERATED = dict(milli=800, W=20, min_area=64)        # W below the longest absence: the window decides some returns


def generated(n=96, cell=16, seed=SEED):
    """(frames uint8 [n,64,64,3], labels int32 [n,64,64]): one blob per cell of a 4 x 4 grid, blob i in PALETTE[i % 6] with +-20 noise
    a channel (which stays inside the bin), blob STRADDLER around (64, 160, 96) so that its red channel straddles the bin edge at 64.
    A blob is seen for 4..12 frames, then absent for 10..30, and comes back shifted by -2..2 cells; a seen frame is dropped with
    probability 0.1 (what --track-gap bridges).  The labels number the blobs of a frame in raster order, as objects.label does."""
    rs = np.random.RandomState(seed)
    per, side = 64 // cell, cell - 4
    seen, shift = np.zeros((n, per * per), dtype=bool), np.zeros((n, per * per, 2), dtype=np.int64)
    for i in range(per * per):
        f, on = 0, rs.rand() < 0.6
        while f < n:
            run = rs.randint(4, 13) if on else rs.randint(10, 31)
            if on:
                seen[f:f + run, i] = rs.rand(len(seen[f:f + run])) >= 0.1
                shift[f:f + run, i] = rs.randint(-2, 3, 2)
            f, on = f + run, not on
    frames = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    labels = np.zeros((n, 64, 64), dtype=np.int32)
    for f in range(n):
        k = 0
        for i in np.flatnonzero(seen[f]):
            k += 1
            y, x = 2 + (i // per) * cell + shift[f, i, 0], 2 + (i % per) * cell + shift[f, i, 1]
            base = np.array((64, 160, 96) if i == STRADDLER else PALETTE[i % len(PALETTE)])
            labels[f, y:y + side, x:x + side] = k
            frames[f, y:y + side, x:x + side] = base + rs.randint(-20, 21, (side, side, 3))
    return frames, labels


def generated_conditions(r, what=""):
    """What the comparison on the generated stack must not pass on: asserted on the checker's result r."""
    links, sizes = r["totals"][1], np.bincount(r["identity"][r["identity"] > 0])
    not_mutual = sum(1 for t, (u, s) in r["succ"].items() if r["pred"][u][0] != t)
    linked = np.flatnonzero(r["prev"])
    print(f"{what}: totals {r['totals']}, {len(r['admissible'])} admissible pairs, {not_mutual} best successors refused, {r['ties']} ties")
    assert links >= 20 and sizes.max() >= 3 and not_mutual >= 1 and r["ties"] >= 1
    assert len({int(t) // 4 for t in linked} | {int(r["prev"][t] - 1) // 4 for t in linked}) > 1     # four tracks a workgroup


@pytest.mark.parametrize("G", [0, 2])
def test_generated_stack_meets_its_conditions(G):
    frames, labels = generated()
    t = track_ref.track(labels, TRACK_MILLI, 64, G)
    S, H = ref.appearance(frames, labels, t["track"], 64)
    r = ref.reid(t["table"], t["extra"] if G else None, S, t["totals"][0], **GENERATED)
    generated_conditions(r, f"G={G}")
    Q = r["Q"][:t["totals"][0]]
    assert any(np.count_nonzero(q) > 1 for q in Q)                        # the straddling blob spreads over two bins
