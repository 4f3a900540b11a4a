"""CPU checks of tracking across gaps: the checker of tests/objects_track_gap_ref.py against objects_track_ref at G = 0 and against the
hand-made cases of tests/test_gpu_objects_track_gap.py (their expected arrays are asserted there; here the checker takes the kernels'
place), the window property that TrackStream's carry of G + 1 frames rests on, its remap arithmetic on CPU tensors, fragments, the
flags' parsing and refusals, and the report helpers."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_track_gap_ref as ref  # noqa: E402
import objects_track_ref as base  # noqa: E402
import test_gpu_objects_track_gap as cases  # noqa: E402
from cgs_amd import _lib, cli, objects  # noqa: E402


def _flicker(seed, n=10, side=8, cell=4):
    """A small cousin of the GPU test's stacks: a grid of blobs, each shifted by -1..1 pixels and absent from a third of the frames."""
    rs = np.random.RandomState(seed)
    s = np.zeros((n, side + 2, side + 2), dtype=np.int32)
    per = side // cell
    for f in range(n):
        for i in range(per * per):
            if rs.rand() < 1 / 3:
                continue
            y, x = 1 + (i // per) * cell + rs.randint(-1, 2), 1 + (i % per) * cell + rs.randint(-1, 2)
            s[f, y:y + cell, x:x + cell] = i + 1
    return s[:, 1:-1, 1:-1].copy()


def test_gap_zero_is_the_adjacent_checker():
    for seed in range(4):
        s = _flicker(seed)
        for milli in (1, 300, 1000):
            new, old = ref.track(s, milli, 4, 0, want_paint=True), base.track(s, milli, 4, want_paint=True)
            for key in ("prev", "track", "totals", "table", "track_labels"):
                np.testing.assert_array_equal(new[key], old[key], err_msg=key)
            assert new["heads"] == old["heads"] and not new["extra"].any() and new["gap_links"].tolist() == [old["totals"][1]]
            np.testing.assert_array_equal(new["gap"], old["prev"] > 0)


def test_hand_made_cases(monkeypatch):
    """The literal expectations of the GPU tests hold for the checker: `_gpu` answers with the checker's own result."""
    def checker(labels, milli, K=64, G=1, max_tracks=None, paint=True):
        out = ref.track(np.asarray(labels), milli, K, G, max_tracks, want_paint=paint)
        if paint:
            out["rgb"] = base.colours(out["track_labels"])
        return out
    monkeypatch.setattr(cases, "_gpu", checker)
    cases.test_level_order()
    cases.test_an_object_that_is_taken_does_not_block_a_bridge()
    cases.test_thresholds_at_the_edge()
    for n in (1, 2, 3, 4, 5, 9, 10, 11, 17, 18, 33, 34):
        for G in (1, 2, 8):
            cases.test_blinking_objects(n, G)


def test_a_window_of_g_plus_one_frames_reproduces_every_link():
    compared = 0
    for seed in range(6):
        s = _flicker(10 + seed, n=12)
        for G in (1, 2, 3):
            whole = ref.track(s, 300, 4, G)
            assert whole["gap_links"][1:].sum() > 0
            for cut in range(1, len(s)):
                start = max(0, cut - (G + 1))
                part = ref.track(s[start:], 300, 4, G)
                np.testing.assert_array_equal(part["prev"][cut - start:], whole["prev"][cut:], err_msg=f"seed {seed} G {G} cut {cut}")
                np.testing.assert_array_equal(part["gap"][cut - start:], whole["gap"][cut:])
                compared += whole["prev"][cut:].size
    assert compared == 6 * 3 * 66 * 4
    # and G frames are not enough: the first frame behind the cut may reach G + 1 back
    for G in (1, 3):
        s = np.zeros((G + 3, 4, 4), dtype=np.int32)
        s[0, 1:3, 1:3] = s[G + 1, 1:3, 1:3] = 1
        whole = ref.track(s, 500, 2, G)
        assert whole["gap"][G + 1, 0] == G + 1 and whole["totals"][0] == 1
        assert ref.track(s[1:], 500, 2, G)["gap"][G, 0] == 0                # a carry of G frames loses the link
        np.testing.assert_array_equal(ref.track(s[0:], 500, 2, G)["gap"][G + 1:], whole["gap"][G + 1:])


def _stream(stack, split, milli, K, G):
    """TrackStream.push's arithmetic with the checker as the tracker, on CPU tensors."""
    keep, n_tracks, carry, parts, lo = G + 1, 0, None, [], 0
    for m in split:
        chunk = stack[lo:lo + m]
        lo += m
        if carry is None:
            t = ref.track(chunk, milli, K, G)
            ids, n_tracks = torch.from_numpy(t["track"]), int(t["totals"][0])
            carry = (chunk[-keep:], ids[-keep:])
        else:
            last, last_ids = carry
            c = len(last)
            t = ref.track(np.concatenate([last, chunk]), milli, K, G)
            local = torch.from_numpy(t["track"])
            c0 = local[:c].max()
            ids = objects.stream_remap(local[c:], local[:c], last_ids, c0, n_tracks).to(torch.int32)
            n_tracks = n_tracks + int(t["totals"][0]) - int(c0)
            carry = (np.concatenate([last, chunk])[-keep:], torch.cat((last_ids, ids))[-keep:])
        parts.append(ids)
    return torch.cat(parts).numpy(), n_tracks


def test_generalised_remap_on_cpu_tensors():
    s = np.concatenate([_flicker(3, n=8), np.zeros((1, 8, 8), dtype=np.int32), _flicker(4, n=3)])
    for G in (1, 3):
        whole = ref.track(s, 300, 4, G)
        assert whole["gap_links"][1:].sum() > 0
        for split in cases._splits(12):
            got, n_tracks = _stream(s, split, 300, 4, G)
            np.testing.assert_array_equal(got, whole["track"], err_msg=f"G={G} split {split}")
            assert n_tracks == whole["totals"][0]
    # the form of one carried frame is unchanged: [K] rows
    local, carried = torch.tensor([[2, 3, 0]]), torch.tensor([1, 2, 0])
    assert objects.stream_remap(local, carried, torch.tensor([7, 9, 0]), 2, 11).tolist() == [[9, 12, 0]]
    assert objects.stream_remap(local, carried[None], torch.tensor([[7, 9, 0]]), 2, 11).tolist() == [[9, 12, 0]]


def test_fragments_against_the_sets():
    """objects.fragments is torch plumbing and runs where its tensors are; the partners come from the checker."""
    K, n = 4, 12
    for G in (0, 2):
        truth = _flicker(22, n=n)
        pred = cases._dropped(truth, 21)
        pt, tt = ref.track(pred, 300, K, G), ref.track(truth, 300, K, G)
        best = np.zeros((n, 2, K, 4), dtype=np.int32)
        for f, frame in enumerate(base.truth_partners(pred, truth, K)):
            for q, (p, inter, union) in frame.items():
                area_t, area_p = int((truth[f] == q).sum()), int((pred[f] == p).sum())
                assert area_t + area_p - inter == union
                best[f, 1, q - 1] = (p, inter, area_t, area_p)
        milli = [500, 700, 1000]
        got = objects.fragments(torch.from_numpy(tt["track"]), torch.from_numpy(pt["track"]), torch.from_numpy(best), [m / 1000 for m in milli])
        assert got.dtype == torch.int64 and got.tolist() == ref.fragments(pred, truth, 300, milli, K, G).tolist() and got[0] > 0
    with pytest.raises(ValueError):
        objects.fragments(torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 2, 3, 4), dtype=torch.int32), [0.5])
    with pytest.raises(ValueError):
        objects.fragments(torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 2, 4, 4), dtype=torch.int32), [0.5])


def test_flags_parse_and_refuse():
    assert objects.parse_track_gap("0") == 0 and objects.parse_track_gap(" 8 ") == 8 and objects.TRACK_MAX_GAP == _lib.OBJ_TRACK_MAX_GAP == 8
    for bad in ("-1", "9", "1.5", "", "two"):
        with pytest.raises(ValueError, match="--track-gap"):
            objects.parse_track_gap(bad)
    with pytest.raises(ValueError, match="--overlay-gap"):
        objects.parse_track_gap("9", "--overlay-gap")
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3"]).track_gap == 0
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3", "--track-gap", "3"]).track_gap == 3
    assert cli.parse_args(["-process", "-objects", "--track-iou", "0.3", "--track-gap", "0"]).track_gap == 0
    assert cli.parse_args(["-eval"]).track_gap == 0
    for bad, word in ((["-eval", "-objects", "--track-gap", "2"], "--track-iou"), (["-process", "--track-gap", "2"], "--track-iou"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-gap", "9"], "0..8"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-gap", "-1"], "0..8"),
                      (["-eval", "-objects", "--track-iou", "0.3", "--track-gap", "1.5"], "0..8"),
                      (["-eval", "--track-iou", "0.3", "--track-gap", "1"], "-objects")):
        with pytest.raises((ValueError, SystemExit), match=word):
            cli.parse_args(bad)
    video = ["-process", "--source-video", "a.mp4", "--overlay-video", "b.mp4"]
    assert cli.parse_args(video + ["--overlay-tracks", "0.3"]).overlay_gap == 0
    assert cli.parse_args(video + ["--overlay-tracks", "0.3", "--overlay-gap", "8"]).overlay_gap == 8
    assert cli.parse_args(video).overlay_gap is None
    for bad, word in ((video + ["--overlay-gap", "1"], "--overlay-tracks"), (["-process", "--overlay-gap", "1"], "--source-video"),
                      (video + ["--overlay-tracks", "0.3", "--overlay-gap", "9"], "--overlay-gap"),
                      (video + ["--overlay-tracks", "0.3", "--overlay-gap", "x"], "--overlay-gap")):
        with pytest.raises((ValueError, SystemExit), match=word):
            cli.parse_args(bad)


def test_python_argument_errors_come_before_the_gpu():
    a = torch.zeros((3, 4, 4), dtype=torch.int32)
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="max_gap"):
            objects.track(a, max_gap=bad)
        with pytest.raises(ValueError, match="max_gap"):
            objects.TrackStream(0.5, max_gap=bad)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CgsError):
            objects.track(a, max_gap=2)
    assert objects.Tracks._fields[:9] == ("prev", "track", "n_tracks", "n_links", "n_objects", "longest", "table", "track_labels", "rgb")
    assert objects.Tracks._fields[9:] == ("gap", "gap_links", "extra") and objects.Tracks(*range(9))[9:] == (None, None, None)


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.cgs_objects_track_gap_scratch_bytes(5, 4, -1) == 0 and lib.cgs_objects_track_gap_scratch_bytes(5, 4, 9) == 0
    for n, K in ((1, 1), (2, 64), (7, 3), (1 << 17, 64)):
        old = lib.cgs_objects_track_scratch_bytes(n, K)
        for G in (0, 8):                                                    # the old layout, padded to 8 bytes, two more words per frame and object pair
            assert lib.cgs_objects_track_gap_scratch_bytes(n, K, G) == (old + 7) // 8 * 8 + 8 * n + 8 * n * K
    args = lambda G: (None, 2, 4, 4, 4, 500, G, 8) + (None,) * 10 + (0, None)
    assert lib.cgs_objects_track_gap(*args(1)) == _lib.ERR_BADARG             # NULL pointers: refused before anything is touched


def test_report_helpers():
    s = np.zeros((6, 4, 4), dtype=np.int32)
    s[[0, 1, 3, 5], 0] = 1                                                  # links of gap 1, 2, 2
    s[[0, 4], 2] = 2                                                        # gap 4: bridged only from G = 3
    flat, t = base.track(s, 500, 2), ref.track(s, 500, 2, 3)
    sums = lambda r: (int(r["table"][:, 6].sum()), int(r["table"][:, 7].sum()))
    today = objects.track_report(flat["totals"], flat["table"][:, 2], *sums(flat), 1)
    assert list(today) == ["objects", "untracked_objects", "tracks", "links", "singletons", "mean_length", "max_length", "length_hist", "link_iou"]
    assert objects.track_report(flat["totals"], flat["table"][:, 2], *sums(flat), 1, max_gap=0) == today
    assert list(objects.track_rows(flat["table"], 5)[0]) == ["track", "first_frame", "first_label", "length", "area_sum", "area_min", "area_max",
                                                             "inter_sum", "union_sum", "link_iou"]
    assert t["totals"].tolist() == [2, 4, 6, 6] and t["gap_links"].tolist() == [1, 2, 0, 1]
    side = objects.track_report(t["totals"], t["table"][:, 2], *sums(t), 0, max_gap=3, gap_links=t["gap_links"], missed=t["extra"][:, 1].sum())
    assert list(side)[:9] == list(today) and {k: side[k] for k in list(side)[9:]} == {
        "track_gap": 3, "bridged_links": 3, "missed_frames": 5, "links_by_gap": {"1": 1, "2": 2, "3": 0, "4": 1}, "max_span": 6}
    assert side["max_length"] == 4 and side["tracks"] == 2 and side["link_iou"] == 1.0
    as_tensors = objects.track_report(torch.from_numpy(t["totals"]), torch.from_numpy(t["table"])[:, 2], *sums(t), 0, max_gap=3,
                                      gap_links=torch.from_numpy(t["gap_links"]), missed=torch.tensor(5))
    assert as_tensors == side
    rows = objects.track_rows(t["table"], 2, t["extra"])
    assert [(r["length"], r["bridges"], r["missed"], r["last_frame"]) for r in rows] == [(4, 2, 2, 5), (2, 1, 3, 4)]
    for bad in ({"max_gap": 3, "gap_links": [1, 2, 1], "missed": 5}, {"max_gap": 3, "gap_links": [1, 2, 0, 2], "missed": 5},
                {"max_gap": 9, "gap_links": [4], "missed": 0}):
        with pytest.raises(ValueError):
            objects.track_report(t["totals"], t["table"][:, 2], *sums(t), 0, **bad)
    with pytest.raises(ValueError):
        objects.track_rows(t["table"], 2, t["extra"][:3])
