"""CPU checks of -objects --track-iou's host side: the checker of tests/objects_track_ref.py against expectations written out by hand,
the flag's parsing and refusals, natural_order, track_report / track_rows, the argument checks of cgs_amd.objects.track / switches and
of the entry points.  Nothing here needs a GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_track_ref as ref  # noqa: E402
from cgs_amd import _lib, build, cli, objects  # noqa: E402


def _stack(*rows):
    return np.array(rows, dtype=np.int32)[:, None, :]                      # frames of one row


def test_checker_on_hand_written_maps():
    # renumbered labels: the two objects swap numbers between the frames
    r = ref.track(_stack([1, 1, 0, 2, 2], [2, 2, 0, 1, 1]), 500, K=3, want_paint=True)
    assert r["prev"].tolist() == [[0, 0, 0], [2, 1, 0]] and r["track"].tolist() == [[1, 2, 0], [2, 1, 0]]
    assert r["totals"].tolist() == [2, 2, 4, 2] and r["heads"] == [(0, 1), (0, 2)]
    assert r["table"][:3].tolist() == [[0, 1, 2, 4, 2, 2, 2, 2], [0, 2, 2, 4, 2, 2, 2, 2], [0] * 8] and r["table"].shape == (6, 8)
    assert r["track_labels"][:, 0].tolist() == [[1, 1, 0, 2, 2], [1, 1, 0, 2, 2]]
    # split: object 1 becomes 1 (three of its pixels) and 2 (one): mutual best keeps 1, 2 is a head
    r = ref.track(_stack([1, 1, 1, 1, 0, 0], [1, 1, 1, 2, 0, 0]), 100, K=2)
    assert r["prev"].tolist() == [[0, 0], [1, 0]] and r["track"].tolist() == [[1, 0], [1, 2]] and r["totals"].tolist() == [2, 1, 3, 2]
    assert r["table"][:2].tolist() == [[0, 1, 2, 7, 3, 4, 3, 4], [1, 2, 1, 1, 1, 1, 0, 0]] and r["heads"] == [(0, 1), (1, 2)]
    # merge: 1 and 2 become 1: 1 continues, 2 ends as a singleton
    r = ref.track(_stack([1, 1, 1, 2, 0, 0], [1, 1, 1, 1, 0, 0]), 100, K=2)
    assert r["prev"].tolist() == [[0, 0], [1, 0]] and r["track"].tolist() == [[1, 2], [1, 0]] and r["totals"].tolist() == [2, 1, 3, 2]
    assert r["table"][:2].tolist() == [[0, 1, 2, 7, 3, 4, 3, 4], [0, 2, 1, 1, 1, 1, 0, 0]]
    # the threshold: 3 / 4 holds at 750 and not at 751
    assert ref.track(_stack([1, 1, 1, 2, 0, 0], [1, 1, 1, 1, 0, 0]), 750, K=2)["totals"].tolist() == [2, 1, 3, 2]
    assert ref.track(_stack([1, 1, 1, 2, 0, 0], [1, 1, 1, 1, 0, 0]), 751, K=2)["totals"].tolist() == [3, 0, 3, 1]
    # an exact tie, 2 / 4 with both: the smaller number wins; and IoU exactly 1 / 2 links at 500 and not at 501
    r = ref.track(_stack([1, 1, 2, 2], [1, 1, 1, 1]), 500, K=2)
    assert r["prev"].tolist() == [[0, 0], [1, 0]] and r["track"].tolist() == [[1, 2], [1, 0]] and r["table"][0].tolist() == [0, 1, 2, 6, 2, 4, 2, 4]
    assert ref.track(_stack([1, 1, 2, 2], [1, 1, 1, 1]), 501, K=2)["totals"].tolist() == [3, 0, 3, 1]
    r = ref.track(_stack([2, 2, 2, 2], [2, 2, 1, 1]), 500, K=2)          # the tie seen from the earlier frame
    assert r["prev"].tolist() == [[0, 0], [2, 0]] and r["track"].tolist() == [[0, 1], [1, 2]]
    # an empty frame in the middle ends every track; labels above K and below 1 take no part
    r = ref.track(_stack([1, 1, 3, -4], [0, 0, 3, 0], [1, 1, 0, 9]), 1, K=2)
    assert r["totals"].tolist() == [2, 0, 2, 1] and r["track"].tolist() == [[1, 0], [0, 0], [2, 0]] and not r["prev"].any()
    # three frames in one chain, cut rows
    r = ref.track(_stack([0, 1, 1], [2, 2, 2], [1, 1, 0]), 300, K=2, max_tracks=1)
    assert r["prev"].tolist() == [[0, 0], [0, 1], [2, 0]] and r["totals"].tolist() == [1, 2, 3, 3] and r["table"].tolist() == [[0, 1, 3, 7, 2, 3, 4, 6]]
    assert ref.colours(np.array([0, 1, 2])).tolist() == [[0, 0, 0], [64 + 0xB1 * 191 // 255, 64 + 0x79 * 191 // 255, 64 + 0x37 * 191 // 255],
                                                         [64 + 0x62 * 191 // 255, 64 + 0xF3 * 191 // 255, 64 + 0x6E * 191 // 255]]


def test_checker_switches_by_hand():
    # one truth object over four frames; the prediction covers it throughout but breaks its own track between frames 1 and 2 (the
    # predicted object jumps: no overlap with its predecessor)
    truth = _stack([1, 1, 1, 1, 0, 0, 0, 0], [0, 1, 1, 1, 1, 0, 0, 0], [0, 0, 1, 1, 1, 1, 0, 0], [0, 0, 0, 1, 1, 1, 1, 0])
    pred = _stack([1, 1, 1, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1, 1, 0])
    assert ref.track(truth, 300)["totals"].tolist() == [1, 3, 4, 4] and ref.track(pred, 300)["totals"].tolist() == [2, 2, 4, 2]
    assert ref.switches(pred, truth, 300, [500, 750], K=4).tolist() == [[4, 3, 1], [2, 0, 0]]


def test_track_iou_flag_parses_and_refuses():
    assert objects.parse_track_iou("0.3") == 0.3 and objects.parse_track_iou("1") == 1.0 and objects.parse_track_iou(" 0.001 ") == 0.001
    for bad in ("0", "1.001", "0.3005", "a", "nan", "inf", "", "0.3-0.5", "-0.5", "0.3:0.5:2"):
        with pytest.raises(ValueError):
            objects.parse_track_iou(bad)
    assert cli.parse_args(["-eval", "-objects", "--track-iou", "0.3"]).track_iou == "0.3" and cli.parse_args(["-eval", "-objects"]).track_iou == ""
    assert cli.parse_args(["-process", "-objects", "--track-iou", "0.05"]).track_iou == "0.05"
    assert cli.parse_args(["-eval", "-objects", "--match-iou", "0.5", "--track-iou", "1"]).match_iou == "0.5"
    for bad in (["-eval", "--track-iou", "0.3"], ["-process", "--track-iou", "0.3"], ["--track-iou", "0.3"],
                ["-eval", "-objects", "--track-iou", "0"], ["-eval", "-objects", "--track-iou", "1.5"],
                ["-process", "-objects", "--track-iou", "abc"], ["-eval", "-objects", "--track-iou", "0.3333"],
                ["-eval", "-objects", "--track-iou", "0.3-0.5"], ["-objects", "--track-iou", "0.3"]):
        with pytest.raises(ValueError):
            cli.parse_args(bad)
        with pytest.raises(ValueError):
            cli.main(bad + ["--model", "nowhere"])                         # before a Handler (a GPU) is asked for


def test_natural_order():
    assert objects.natural_order(["f10", "f2", "f1"]) == [2, 1, 0]
    assert objects.natural_order(["f2.x10", "f2.x9", "f10.x1"]) == [1, 0, 2]
    assert objects.natural_order(["frame1", "frame01", "frame001"]) == [2, 1, 0]          # equal as numbers: plain string order
    assert objects.natural_order(["b", "a", "10", "9", "a0"]) == [3, 2, 1, 4, 0]           # a number sorts before a letter
    assert objects.natural_order([]) == [] and objects.natural_order(["only"]) == [0]
    assert objects.natural_order(["x", "x"]) == [0, 1]
    names = [f"img{k}" for k in (100, 20, 3, 21, 0)]
    assert [names[i] for i in objects.natural_order(names)] == ["img0", "img3", "img20", "img21", "img100"]


def test_track_report_and_rows():
    table = np.zeros((6, 8), dtype=np.int32)
    table[0] = [0, 1, 4, 40, 8, 12, 27, 36]
    table[1] = [0, 2, 2, 9, 4, 5, 3, 6]
    table[2] = [3, 1, 1, 7, 7, 7, 0, 0]
    r = objects.track_report([3, 4, 7, 4], table[:, 2], table[:, 6].sum(), table[:, 7].sum(), untracked=2)
    assert r == {"objects": 7, "untracked_objects": 2, "tracks": 3, "links": 4, "singletons": 1, "mean_length": 7 / 3, "max_length": 4,
                 "length_hist": {"1": 1, "2": 1, "3-4": 1, "5-8": 0, "9-16": 0, "17-32": 0, "33+": 0}, "link_iou": 30 / 42}
    assert list(r["length_hist"]) == ["1", "2", "3-4", "5-8", "9-16", "17-32", "33+"]
    t = objects.track_report(torch.tensor([3, 4, 7, 4], dtype=torch.int32), torch.from_numpy(table)[:, 2], torch.tensor(30), torch.tensor(42), torch.tensor(2))
    assert t == r and json.loads(json.dumps(t)) == r
    lengths = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 1000, 0, 0]
    edges = objects.track_report([12, sum(lengths) - 12, sum(lengths), 1000], lengths)
    assert list(edges["length_hist"].values()) == [1, 1, 2, 2, 2, 2, 2] and edges["link_iou"] is None and edges["singletons"] == 1
    assert objects.length_hist(torch.tensor(lengths)).tolist() == objects.length_hist(lengths).tolist() == [1, 1, 2, 2, 2, 2, 2]
    empty = objects.track_report([0, 0, 0, 0], np.zeros(4, dtype=np.int32))
    assert empty["mean_length"] is None and empty["link_iou"] is None and empty["tracks"] == 0 and sum(empty["length_hist"].values()) == 0
    assert json.dumps(empty).count("null") == 2
    for bad in (([3, 4, 8, 4], table[:, 2]), ([2, 5, 7, 4], table[:, 2]), ([3, 4, 7, 4], table[:2, 2]), ([-1, 0, -1, 0], [])):
        with pytest.raises(ValueError):
            objects.track_report(*bad)
    rows = objects.track_rows(table, 3)
    assert rows[0] == {"track": 1, "first_frame": 0, "first_label": 1, "length": 4, "area_sum": 40, "area_min": 8, "area_max": 12, "inter_sum": 27,
                       "union_sum": 36, "link_iou": 0.75}
    assert rows[2]["link_iou"] is None and rows[2]["first_frame"] == 3 and len(rows) == 3
    assert objects.track_rows(torch.from_numpy(table), 3) == rows and objects.track_rows(table, 0) == []
    assert len(objects.track_rows(table[:2], 3)) == 2                      # a cut table gives the rows it has
    for bad in ((table[:, :7], 3), (table[None], 3), (table, -1)):
        with pytest.raises(ValueError):
            objects.track_rows(*bad)


def test_track_argument_errors():
    z = torch.zeros(2, 8, 8, dtype=torch.int32)
    for bad in (dict(iou=0), dict(iou=1.001), dict(iou=0.3005), dict(iou=(0.5,)), dict(iou="0.5"), dict(iou=float("nan")), dict(iou=True),
                dict(max_objects=0), dict(max_objects=65), dict(max_objects=1.5), dict(max_tracks=0), dict(max_tracks=-3), dict(max_tracks=2.5),
                dict(max_tracks=1 << 31)):
        with pytest.raises(ValueError):
            objects.track(z, **bad)
    for a in (z.float(), z.long(), z.bool(), z[0, 0], z[None], torch.zeros(2, 65, 8, dtype=torch.int32), torch.zeros(2, 8, 65, dtype=torch.int32),
              torch.zeros(0, 8, 8, dtype=torch.int32), torch.zeros(2, 0, 8, dtype=torch.int32), z.numpy(), None):
        with pytest.raises(ValueError):
            objects.track(a)
    p, b = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 2, 4, 4, dtype=torch.int32)
    for args in ((p, p[:1], b, (0.5,)), (p, p, b[:1], (0.5,)), (p.long(), p, b, (0.5,)), (p, p, b.float(), (0.5,)), (p, p, b, (0.4,)), (p, p, b, ()),
                 (p[0], p[0], b, (0.5,)), (p.numpy(), p, b, (0.5,)), (torch.zeros(2, 65, dtype=torch.int32),) * 2 + (torch.zeros(2, 2, 65, 4, dtype=torch.int32), (0.5,))):
        with pytest.raises(ValueError):
            objects.switches(*args)


def test_track_has_no_cpu_path():
    """Label maps in host memory: CgsError, with or without a GPU in the machine."""
    z = torch.zeros(2, 8, 8, dtype=torch.int32)
    with pytest.raises(_lib.CgsError):
        objects.track(z)
    with pytest.raises(_lib.CgsError):
        objects.track(z[0], iou=0.3, max_objects=7, max_tracks=2, want_labels=True, want_rgb=True)
    with pytest.raises(_lib.CgsError):
        objects.switches(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 2, 4, 4, dtype=torch.int32), (0.5, 0.75))


def test_track_entry_points_are_declared_and_check_their_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_objects_track\s*\(", text) and re.search(r"\bint cgs_objects_track_switches\s*\(", text)
    assert re.search(r"\bint64_t cgs_objects_track_scratch_bytes\s*\(", text)
    assert "objects_track.hip" in build.SOURCES
    assert all(k in _lib.SIGNATURES for k in ("cgs_objects_track", "cgs_objects_track_switches", "cgs_objects_track_scratch_bytes"))
    assert _lib.OBJ_TRACK_MAX_FRAMES == 1 << 17 and re.search(r"CGS_OBJ_TRACK_MAX_FRAMES\s*=\s*1\s*<<\s*17\b", text)
    assert "Gaps are NOT bridged" in text
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    size = lib.cgs_objects_track_scratch_bytes
    assert size(1, 1) > 0 and size(0, 4) == 0 and size(4, 0) == 0
    sizes = [size(n, 64) for n in (1, 2, 3, 100, 2450, 1 << 17)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and size(5, 3) < size(5, 4)
    assert sizes[-1] < 1 << 40 and size((1 << 31) - 1, (1 << 31) - 1) > 0          # no wrap-around
    # argument checks come before anything is launched: safe without a GPU (the pointers are never followed)
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    assert p % 8 == 0
    big = 1 << 62
    ok = dict(labels=p, n=2, h=4, w=4, K=4, iou=300, max_tracks=8, prev=p, track=p, totals=p, tracks=None, painted=None, rgb=None, scratch=p,
              bytes=big)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cgs_objects_track(a["labels"], a["n"], a["h"], a["w"], a["K"], a["iou"], a["max_tracks"], a["prev"], a["track"], a["totals"],
                                     a["tracks"], a["painted"], a["rgb"], a["scratch"], a["bytes"], None)

    for bad in (dict(labels=None), dict(prev=None), dict(track=None), dict(totals=None), dict(scratch=None), dict(n=0), dict(n=-1), dict(h=0),
                dict(w=-1), dict(K=0), dict(K=-5), dict(max_tracks=0), dict(iou=0), dict(iou=1001), dict(iou=-1), dict(labels=p + 2),
                dict(prev=p + 1), dict(track=p + 2), dict(totals=p + 3), dict(tracks=p + 2), dict(painted=p + 1), dict(scratch=p + 4),
                dict(bytes=size(2, 4) - 1), dict(bytes=0), dict(bytes=-1)):
        assert call(**bad) == _lib.ERR_BADARG, bad
    for big_shape in (dict(h=65), dict(w=65), dict(K=65), dict(n=(1 << 17) + 1), dict(h=4096, w=4096, K=4096)):
        assert call(**big_shape) == _lib.ERR_UNSUPPORTED, big_shape
    for bad in (dict(h=65, iou=0), dict(K=65, totals=None), dict(w=65, n=0), dict(n=(1 << 17) + 1, max_tracks=0), dict(K=65, bytes=size(2, 65) - 1)):
        assert call(**bad) == _lib.ERR_BADARG, bad                      # a bad argument is reported before an unsupported size

    ok = dict(prev=p, track=p, best=p, iou=p, T=1, n=2, K=4, counts=p)

    def switches(**kw):
        a = {**ok, **kw}
        return lib.cgs_objects_track_switches(a["prev"], a["track"], a["best"], a["iou"], a["T"], a["n"], a["K"], a["counts"], None)

    for bad in (dict(prev=None), dict(track=None), dict(best=None), dict(iou=None), dict(counts=None), dict(T=0), dict(T=17), dict(n=0), dict(K=0),
                dict(prev=p + 2), dict(track=p + 1), dict(best=p + 3), dict(iou=p + 2), dict(counts=p + 2), dict(K=65, T=17), dict(n=1 << 20, counts=None)):
        assert switches(**bad) == _lib.ERR_BADARG, bad
    assert switches(K=65) == _lib.ERR_UNSUPPORTED and switches(n=(1 << 17) + 1) == _lib.ERR_UNSUPPORTED
