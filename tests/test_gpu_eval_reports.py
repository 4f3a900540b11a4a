"""The reports of -eval and -process -objects as a set (cgs_amd.evaluate, cgs_amd.process): a run that asks for every report writes, for
each, the bytes a run that asks for it alone writes; the stacks are uploaded, labelled and matched once; a plain -eval asks for none
of it.  What each report must hold is checked where the report is: test_gpu_{metrics,objects,objects_match,objects_track,boundary}.py."""
import inspect
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
import objects_track_ref as track_ref  # noqa: E402
from cgs_amd import boundary, cli, handler, metrics, objects  # noqa: E402
from test_gpu_objects_match import _read, _results, _run, workdir  # noqa: E402, F401  (the small evaluation fixture of eval_match.json)
from test_gpu_objects_track import _files, _side  # noqa: E402

pytestmark = pytest.mark.gpu
WRAPPED = ((objects, "label"), (objects, "match"), (objects, "track"), (boundary, "score"), (metrics, "iou_curve"), (metrics, "iou_counts"))
REPORTS = ("sweep", "objects", "match", "tracks", "boundary")
LINES = ("THRESH SWEEP", "OBJECTS", "MATCH", "TRACKS", "BOUNDARY", "RESULTS")


class Recorder:
    """Wraps the GPU entry points the reports call; a record is (name, the call's arguments with the defaults filled in, its result).
    The records keep the tensors alive, so a data_ptr() seen twice is one tensor and not an address handed out again."""

    def __init__(self, monkeypatch):
        self.calls = []
        for mod, name in WRAPPED:
            monkeypatch.setattr(mod, name, self._wrap(name, getattr(mod, name)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def recorded(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            out = fn(*a, **kw)
            self.calls.append((name, dict(bound.arguments), out))
            return out
        return recorded

    def of(self, name):
        return [kw for n, kw, _ in self.calls if n == name]


def _prepare(root, frames):
    """The threshold and the truth of test_gpu_boundary.py: half of the pixels above the threshold, the truth the masks cut a little
    higher, so that the objects are neither none nor all and every report has something to count.  Returns (H, M, thr, truth)."""
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    return H, M, thr, truth


def _flags(thr):
    """The flags each report needs, and all of them together."""
    base = ["-crf", "-eval", "--eval-thresh", repr(thr)]                   # -crf everywhere: RESULTS then lists the same IoUs
    obj = base + ["-objects", "--min-area", "4"]
    match, track = ["--match-iou", "0.5:0.95:10"], ["--track-iou", "0.3"]
    alone = {"sweep": base + ["--thresh-grid", "0:1:21"], "objects": obj, "match": obj + match, "tracks": obj + match + track,      # (the switches of
             "boundary": obj + ["--boundary-tol", "0-1-2"]}                                          # eval_tracks.json are at --match-iou's thresholds)
    return alone, obj + ["--thresh-grid", "0:1:21"] + match + track + ["--boundary-tol", "0-1-2"]


def _reports(root):
    return {k: _read(os.path.join(root, "m", f"eval_{k}.json")) for k in REPORTS if os.path.exists(os.path.join(root, "m", f"eval_{k}.json"))}


def _attrs(H):
    return {"sweep": H.sweep, "objects": H.objects, "match": H.matches, "tracks": H.tracks, "boundary": H.boundary}


def test_combined_equals_separate(workdir, capsys):
    root, frames = workdir
    _, _, thr, _ = _prepare(root, frames)
    alone, combined = _flags(thr)
    H, out = _run(combined, capsys)
    got, attrs = _reports(root), _attrs(H)
    assert set(got) == set(REPORTS) and all(v is not None for v in attrs.values())
    lines = [ln for ln in out.split("\n") if ln.startswith(LINES)]
    assert [next(w for w in LINES if ln.startswith(w)) for ln in lines] == list(LINES)            # once each, in this order
    objects_json = json.loads(got["objects"])
    assert 0 < objects_json["mask"]["kept"] < objects_json["mask"]["found"]                       # neither none nor all
    for name, flags in alone.items():
        for k in REPORTS:
            path = os.path.join(root, "m", f"eval_{k}.json")
            if os.path.exists(path):
                os.remove(path)
        H1, out1 = _run(flags, capsys)
        one = _reports(root)
        assert name in one, name
        for k, data in one.items():                                                               # (the objects report comes with its dependants)
            assert data == got[k], (name, k)
            assert handler._json_safe(_attrs(H1)[k]) == handler._json_safe(attrs[k]), (name, k)            # (a NaN ratio equals no NaN)
        assert _results(out1) == _results(out), name
        word = LINES[REPORTS.index(name)]
        assert [ln for ln in out1.split("\n") if ln.startswith(word)] == [ln for ln in lines if ln.startswith(word)], name


def test_nothing_twice(workdir, capsys, monkeypatch):
    root, frames = workdir
    H0, M, thr, truth = _prepare(root, frames)
    crf_on = torch.from_numpy(np.ascontiguousarray(H0.crf(frames, M, truth)[:, 0])).to(H0.device)
    rec = Recorder(monkeypatch)
    _run(_flags(thr)[1], capsys)
    assert all(rec.of(name) for _, name in WRAPPED)                                               # the combined run goes through every one
    label_keys = [(kw["src"].data_ptr(),) + tuple(kw[k] for k in ("thresh", "inclusive", "connectivity", "min_area", "max_objects",
                                                                  "want_labels", "want_mask")) for kw in rec.of("label")]
    assert len(set(label_keys)) == len(label_keys), label_keys
    match_keys = [(kw["pred_labels"].data_ptr(), kw["truth_labels"].data_ptr(), tuple(kw["iou"]), kw["max_objects"], kw["want_best"])
                  for kw in rec.of("match")]
    assert len(set(match_keys)) == len(match_keys), match_keys
    # the stack each call scores or labels (its first argument), its threshold where it has one, and the truth it is scored against
    first = {"label": "src", "score": "pred", "iou_curve": "prob", "iou_counts": "labels"}
    thresh_of = lambda name, kw: kw["thresholds"] if name == "iou_curve" else kw["thresh"] if name in ("label", "score") else None
    reads = [(name, kw[first[name]], thresh_of(name, kw), kw.get("truth")) for name, kw, _ in rec.calls if name in first]
    # the mask probabilities: one tensor
    prob = [(name, t) for name, t, thr_, _ in reads if t.dtype == torch.float32 and thr_ is not None]
    assert {name for name, _ in prob} == {"label", "score", "iou_curve"} and len({t.data_ptr() for _, t in prob}) == 1
    assert np.array_equal(prob[0][1].cpu().numpy(), M[:, 0])
    # the truth: one tensor for every scorer, and the one that is labelled
    truths = {t.data_ptr() for _, _, _, t in reads if t is not None}
    assert len(truths) == 1 and sum(kw["src"].data_ptr() in truths for kw in rec.of("label")) == 1
    # the CRF labels: one tensor wherever a call is given them (the kept-pixel masks that objects.label made are not uploads)
    made = {out.mask.data_ptr() for name, _, out in rec.calls if name == "label" and out.mask is not None}
    crf = [(name, t) for name, t, thr_, _ in reads if thr_ is None and t.dtype == torch.bool and t.data_ptr() not in made | truths
           and torch.equal(t, crf_on)]
    assert {name for name, _ in crf} == {"label", "score", "iou_counts"} and len({t.data_ptr() for _, t in crf}) == 1


def test_plain_eval_stays_plain(workdir, capsys, monkeypatch):
    root, frames = workdir
    rec = Recorder(monkeypatch)
    H, out = _run(["-eval"], capsys)
    assert rec.calls == [] and _reports(root) == {} and all(v is None for v in _attrs(H).values())
    assert [ln for ln in out.split("\n") if ln.startswith(LINES)] == [ln for ln in out.split("\n") if ln.startswith("RESULTS")]


@pytest.mark.parametrize("source", ["thresholded-mask", "crf-mask"])
def test_process_objects_with_tracks(workdir, capsys, monkeypatch, source):
    """-process -objects --track-iou: objects.json and the object PNGs are those of a run without --track-iou, tracks.json is what
    test_gpu_objects_track.py's checker gives for the same objects, and the stack is labelled once for both."""
    from PIL import Image
    root, frames = workdir
    os.makedirs("S")
    numbers = (2, 10, 1, 11)                                               # natural order is not string order
    stems = [f"f{k}" for k in numbers]
    for k, stem in zip(numbers, stems):                                    # a pixel a frame in natural order: the objects persist
        Image.fromarray(np.roll(frames[0], sorted(numbers).index(k), axis=1)).save(os.path.join("S", stem + ".png"))
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S")]
    thr = float(np.median(M))
    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2"]
    common += ["-crf"] if source == "crf-mask" else []
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    rec = Recorder(monkeypatch)
    _run(common + ["--mask-output-imgs", "R2", "--track-iou", "0.3"], capsys)
    r1, r2 = _files("R1"), _files("R2")
    assert set(r2) - set(r1) == {"tracks.json"} | {f"{s}-tracks-mask.png" for s in stems}
    assert all(r2[f] == r1[f] for f in r1) and "objects.json" in r1 and all(f"{s}-objects-mask.png" in r1 for s in stems)
    assert len(rec.of("label")) == 1 and rec.of("label")[0]["want_labels"] and rec.of("label")[0]["want_mask"]      # labelled once for both
    if source == "crf-mask":
        on = np.stack([np.array(Image.open(os.path.join("R2", f"{s}-crf-mask.png")))[:, :, 0] > 0 for s in listed])
    else:
        on = objects_ref.on_pixels(M[:, 0], thr, inclusive=True)
    labels, _, kept, _, _ = objects_ref.label(on, 8, 2, 64)
    natural = sorted(stems, key=lambda s: int(s[1:]))
    order = [listed.index(s) for s in natural]
    t, side = _side(labels[order], kept[order], 300)
    assert side["links"] > 0
    rows = objects.track_rows(t["table"], side["tracks"])
    assert json.loads(r2["tracks.json"]) == {
        "source": source, "threshold": thr if source == "thresholded-mask" else None, "connectivity": 8, "min_area": 2, "max_objects": 64,
        "track_iou": 0.3, "summary": side, "order": natural,
        "frames": {s: [{"label": l + 1, "track": int(t["track"][j, l]), "prev": int(t["prev"][j, l])} for l in np.flatnonzero(t["track"][j])]
                   for j, s in enumerate(natural)},
        "tracks": [{"track": r["track"], "first": natural[r["first_frame"]], "last": natural[r["first_frame"] + r["length"] - 1],
                    "length": r["length"], "area_sum": r["area_sum"], "area_min": r["area_min"], "area_max": r["area_max"],
                    "link_iou": r["link_iou"]} for r in rows]}
    painted = track_ref.track(labels[order], 300, 64, want_paint=True)["track_labels"]
    for j, s in enumerate(natural):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R2", f"{s}-tracks-mask.png"))), track_ref.colours(painted[j]))
