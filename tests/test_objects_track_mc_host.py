"""CPU checks of motion-compensated tracking: the checker of tests/objects_track_mc_ref.py against objects_track_gap_ref on zero
fields and against the hand-made cases of tests/test_gpu_objects_track_mc.py (their expected arrays are asserted there; here the checker
takes the kernels' place), the window property TrackStream(motion=True) rests on, its carry of the vectors on CPU tensors, the two
flags' parsing and refusals, the report helpers' new keys, and the new symbol."""
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
import test_gpu_objects_track_mc as cases  # noqa: E402
from cgs_amd import _lib, cli, evaluate, objects, process  # noqa: E402

KEYS = ("prev", "gap", "track", "totals", "gap_links", "table", "extra", "track_labels")


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


def _small_field(n, seed, reach=4):
    return np.random.RandomState(seed).randint(-reach, reach + 1, (n - 1, 8, 8, 2)).astype(np.int8)


def test_zero_fields_give_the_gap_checker():
    for seed in range(3):
        s = _flicker(seed)
        for G in (0, 1, 3):
            for milli in (300, 1000):
                new, old = ref.track(s, np.zeros((len(s) - 1, 8, 8, 2), dtype=np.int8), milli, 16, G, want_paint=True), \
                    gap_ref.track(s, milli, 16, G, want_paint=True)
                for key in KEYS:
                    np.testing.assert_array_equal(new[key], old[key], err_msg=f"{key} seed {seed} G {G}")
                assert new["heads"] == old["heads"] and new["spans"] == old["spans"] and (milli == 1000 or new["totals"][1] > 0)


def test_the_gather_cell_by_cell_is_the_gather_at_once():
    s = _flicker(9)
    for reach, seed in ((4, 1), (127, 2)):
        bwd = _small_field(len(s), seed, reach)
        for a, f in ((0, 1), (2, 5), (0, 7)):
            np.testing.assert_array_equal(ref.carried(s[a], bwd, a, f, 16), ref.carried_plain(s[a], bwd, a, f, 16))
    far = np.full((9, 8, 8, 2), -128, dtype=np.int8)
    assert ref.offset(far, 0, 9, 63, 63) == (-9 * 128, -9 * 128) and not ref.carried(s[0], far[:7], 0, 7, 16).any()


def test_hand_made_cases(monkeypatch):
    """The literal expectations of the GPU tests hold for the checker: `_gpu` answers with the checker's own result."""
    def checker(labels, bwd, milli, K=64, G=0, max_tracks=None, paint=True):
        labels = np.asarray(labels)
        if bwd is None:
            out = gap_ref.track(labels, milli, K, G, max_tracks, want_paint=paint)
        else:
            out = ref.track(labels, bwd, milli, K, G, max_tracks, want_paint=paint)
        if paint:
            out["rgb"] = base.colours(out["track_labels"])
        return out
    monkeypatch.setattr(cases, "_gpu", checker)
    cases.test_a_pan_that_breaks_the_old_tracker()
    cases.test_carried_area_decides()
    cases.test_gap_and_pan_together()


def test_a_link_depends_on_its_two_frames_and_the_vectors_between():
    compared = 0
    for seed in range(3):
        s, bwd = _flicker(20 + seed, n=9), _small_field(9, seed)
        for G in (0, 2):
            whole = ref.all_links(s, bwd, 300, 16, G)
            assert len(whole) > 10 and (G == 0 or any(v[1] > 1 for v in whole.values()))
            for a in range(8):
                for g in range(1, min(G + 1, 8 - a) + 1):                  # the sub-stack a .. a + g with bwd[a .. a + g - 1]
                    part = ref.all_links(s[a:a + g + 1], bwd[a:a + g], 300, 16, G)
                    want = {q: v for (f, q), v in whole.items() if f == a + g and v[1] == g}
                    assert {q: v for (f, q), v in part.items() if f == g and v[1] == g} == want, (seed, G, a, g)
                    compared += len(want)
            # the stream's form: a window that starts G + 1 frames before the cut reproduces every link behind the cut
            for cut in range(1, 9):
                start = max(0, cut - (G + 1))
                part = ref.track(s[start:], bwd[start:], 300, 16, G)
                full = ref.track(s, bwd, 300, 16, G)
                np.testing.assert_array_equal(part["prev"][cut - start:], full["prev"][cut:], err_msg=f"seed {seed} G {G} cut {cut}")
                np.testing.assert_array_equal(part["gap"][cut - start:], full["gap"][cut:])
    assert compared > 60
    # and the vectors before a and behind f do not matter
    s, bwd = _flicker(30, n=6), _small_field(6, 5)
    other = bwd.copy()
    other[[0, 4]] = _small_field(3, 6)
    links = lambda field: {k: v for k, v in ref.all_links(s, field, 300, 16, 2).items() if k[0] <= 4 and k[0] - v[1] >= 1}
    assert links(bwd) == links(other) and len(links(bwd)) > 5 and ref.all_links(s, bwd, 300, 16, 2) != ref.all_links(s, other, 300, 16, 2)


def _stream(stack, rows, split, milli, K, G):
    """TrackStream.push's arithmetic with motion, the checker as the tracker, on CPU tensors: the carry holds each carried frame's
    vector beside its labels."""
    keep, n_tracks, carry, parts, lo = G + 1, 0, None, [], 0
    for m in split:
        chunk, vec = stack[lo:lo + m], rows[lo:lo + m]
        lo += m
        if carry is None:
            t = ref.track(chunk, vec[1:], milli, K, G)
            ids, n_tracks = torch.from_numpy(t["track"]), int(t["totals"][0])
            carry = (chunk[-keep:], ids[-keep:], vec[-keep:])
        else:
            last, last_ids, last_vec = carry
            c = len(last)
            t = ref.track(np.concatenate([last, chunk]), np.concatenate([last_vec[1:], vec]), milli, K, G)
            local = torch.from_numpy(t["track"])
            c0 = local[:c].max()
            ids = objects.stream_remap(local[c:], local[:c], last_ids, c0, n_tracks).to(torch.int32)
            n_tracks = n_tracks + int(t["totals"][0]) - int(c0)
            carry = (np.concatenate([last, chunk])[-keep:], torch.cat((last_ids, ids))[-keep:], np.concatenate([last_vec, vec])[-keep:])
        parts.append(ids)
    return torch.cat(parts).numpy(), n_tracks


def test_stream_carry_arithmetic_on_cpu_tensors():
    s, bwd = _flicker(40, n=10), _small_field(10, 8)
    rows = np.concatenate([np.full((1, 8, 8, 2), 99, dtype=np.int8), bwd])
    for G in (0, 2):
        whole = ref.track(s, bwd, 300, 16, G)
        assert whole["totals"][1] > 10 and not np.array_equal(whole["track"], gap_ref.track(s, 300, 16, G)["track"])
        for split in cases.SPLITS + ([5, 5], [2, 2, 2, 2, 2]):
            got, n_tracks = _stream(s, rows, split, 300, 16, G)
            np.testing.assert_array_equal(got, whole["track"], err_msg=f"G={G} split {split}")
            assert n_tracks == whole["totals"][0]


def test_flags_parse_and_refuse():
    assert objects.parse_track_motion("0") == 0 and objects.parse_track_motion(" 4 ") == 4
    assert objects.MOTION_MAX_SEARCH == _lib.TEMPORAL_MAX_SEARCH == 4 and objects.MOTION_BLOCKS == 8
    for bad in ("-1", "5", "1.5", "", "two"):
        with pytest.raises(ValueError, match="--track-motion"):
            objects.parse_track_motion(bad)
    with pytest.raises(ValueError, match="--overlay-motion"):
        objects.parse_track_motion("5", "--overlay-motion")
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3"]).track_motion == 0
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3", "--track-motion", "3"]).track_motion == 3
    assert cli.parse_args(["-process", "-objects", "--track-iou", "0.3", "--track-gap", "2", "--track-motion", "4"]).track_motion == 4
    assert cli.parse_args(["-process", "-objects", "--track-iou", "0.3", "--track-motion", "0"]).track_motion == 0
    assert cli.parse_args(["-eval"]).track_motion == 0
    for bad, word in ((["-eval", "-objects", "--track-motion", "2"], "--track-iou"), (["-process", "--track-motion", "2"], "--track-iou"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-motion", "5"], "0..4"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-motion", "-1"], "0..4"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-motion", "1.5"], "0..4"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-motion", "x"], "0..4"),
                      (["-eval", "--track-iou", "0.3", "--track-motion", "1"], "-objects")):
        with pytest.raises((ValueError, SystemExit), match=word):
            cli.parse_args(bad)
    video = ["-process", "--source-video", "a.mp4", "--overlay-video", "b.mp4"]
    assert cli.parse_args(video + ["--overlay-tracks", "0.3"]).overlay_motion == 0
    assert cli.parse_args(video + ["--overlay-tracks", "0.3", "--overlay-motion", "4"]).overlay_motion == 4
    assert cli.parse_args(video + ["--overlay-tracks", "0.3", "--overlay-gap", "2", "--overlay-motion", "1"]).overlay_motion == 1
    assert cli.parse_args(video).overlay_motion is None
    for bad, word in ((video + ["--overlay-motion", "1"], "--overlay-tracks"), (["-process", "--overlay-motion", "1"], "--source-video"),
                      (video + ["--overlay-tracks", "0.3", "--overlay-motion", "5"], "--overlay-motion"),
                      (video + ["--overlay-tracks", "0.3", "--overlay-motion", "1.5"], "--overlay-motion"),
                      (video + ["--overlay-tracks", "0.3", "--overlay-motion", "x"], "--overlay-motion")):
        with pytest.raises((ValueError, SystemExit), match=word):
            cli.parse_args(bad)


def test_python_argument_errors_come_before_the_gpu():
    a = torch.zeros((3, 64, 64), dtype=torch.int32)
    field = torch.zeros((2, 8, 8, 2), dtype=torch.int8)
    with pytest.raises(ValueError, match="64 x 64"):
        objects.track(torch.zeros((3, 32, 64), dtype=torch.int32), motion=field)
    for wrong in (field[:1], field.to(torch.int16), "bwd", (field,), (field, field, field), torch.zeros((2, 8, 8), dtype=torch.int8)):
        with pytest.raises(ValueError, match="motion"):
            objects.track(a, motion=wrong)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CgsError):
            objects.track(a, motion=field)
        with pytest.raises(_lib.CgsError):
            objects.track(a, motion=(field, field))
    ts = objects.TrackStream(0.5, max_gap=1, motion=True)
    assert ts.motion and not objects.TrackStream(0.5).motion
    for wrong in (None, field[:2], torch.zeros((3, 8, 8, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match="bwd"):
            ts.push(a, wrong)
    with pytest.raises(ValueError, match="bwd"):
        objects.TrackStream(0.5).push(a, torch.zeros((3, 8, 8, 2), dtype=torch.int8))


def test_the_entry_point_is_exported_and_checks_its_arguments():
    lib = _lib.load()
    assert len(_lib.SIGNATURES["cgs_objects_track_mc"][1]) == 21 and len(_lib.SIGNATURES["cgs_objects_track_mc_scratch_bytes"][1]) == 3
    for n, K, G in ((1, 1, 0), (2, 64, 8), (7, 3, 2), (1 << 17, 64, 8)):
        assert lib.cgs_objects_track_mc_scratch_bytes(n, K, G) == lib.cgs_objects_track_gap_scratch_bytes(n, K, G) > 0
    assert lib.cgs_objects_track_mc_scratch_bytes(5, 4, -1) == 0 and lib.cgs_objects_track_mc_scratch_bytes(5, 4, 9) == 0
    args = (None, None, 2, 64, 64, 4, 500, 1, 8) + (None,) * 10 + (0, None)
    assert lib.cgs_objects_track_mc(*args) == _lib.ERR_BADARG                 # NULL pointers: refused before anything is touched
    assert lib.cgs_abi_version() == 1
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        header = fp.read()
    assert "int cgs_objects_track_mc(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects," in header
    assert "int64_t cgs_objects_track_mc_scratch_bytes(int32_t n, int32_t max_objects, int32_t max_gap);" in header
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        with open(os.path.join(REPO, doc)) as fp:
            text = fp.read()
        assert "cgs_objects_track_mc" in text and "--track-motion" in text and "--overlay-motion" in text, doc


def test_report_helpers():
    bwd = np.zeros((3, 8, 8, 2), dtype=np.int8)
    bwd[0] = (0, -3)
    bwd[1, :4] = (4, 0)
    rep = objects.motion_report(bwd, 4)
    assert list(rep) == ["search", "block", "mean_cells_per_frame", "saturated"] and (rep["search"], rep["block"]) == (4, 8)
    assert rep["mean_cells_per_frame"] == (64 * 3 + 32 * 4) / 192 and rep["saturated"] == 32 / 192
    assert objects.motion_report(torch.from_numpy(bwd), 4) == rep
    assert objects.motion_report(bwd[:0], 2) == {"search": 2, "block": 8, "mean_cells_per_frame": None, "saturated": None}
    # without the flags the reports' keys are what they were
    s = cases._square(4, 20, 6, 3)
    flat = base.track(s, 300, 64)
    sums = lambda r: (int(r["table"][:, 6].sum()), int(r["table"][:, 7].sum()))
    side = objects.track_report(flat["totals"], flat["table"][:, 2], *sums(flat), 0)
    assert "track_motion" not in side and "motion" not in str(side)
    t = ref.track(s, cases._field(4, (0, -3)), 300, 64)
    moved = objects.track_report(t["totals"], t["table"][:, 2], *sums(t), 0)
    assert list(moved) == list(side) and moved["tracks"] == 1 and side["tracks"] == 4 and moved["link_iou"] == 1.0
    assert "low" in process.objects_and_tracks.__code__.co_varnames and "bwd" in process.video_reports.__code__.co_varnames
    assert "motion" in evaluate._tracked.__code__.co_varnames
