"""--object-value end to end on the folder and the synthetic red-trees/ of tests/test_gpu_objects_track_gap.py: what -process -objects and
-eval -objects write with the flags is the plain report plus what tests/objects_value_ref.py and objects.value's drops give, and without
the flags nothing changes."""
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

import objects_match_ref as match_ref  # noqa: E402
import objects_ref  # noqa: E402
import objects_value_ref as ref  # noqa: E402
from cgs_amd import cli, handler, objects  # noqa: E402
from test_gpu_objects_track_gap import _files, _run, workdir  # noqa: E402,F401

pytestmark = pytest.mark.gpu
K = 64


def _values(H, frames, labels, kept):
    """objects.value with the handler's critic, as the command line asks it: (base, drop) as host arrays, fill_frame, rows."""
    eng = H._engine(2 * 32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(H.device)
    val = objects.value(lambda X: eng.infer(X, want_mask=False)[0], dev(frames), dev(labels), dev(kept), fill="low", grow=0, max_objects=K)
    return val.base.cpu().numpy(), val.drop.cpu().numpy(), val.fill_frame, val.rows


def _threshold(drop, kept):
    """V halfway between two adjacent distinct drops of the scored objects, both sides of the selection non-empty."""
    scored = np.arange(K)[None] < np.clip(kept, 0, K)[:, None]
    distinct = np.unique(drop[scored])
    assert len(distinct) >= 2, f"the fixture's critic gives {len(distinct)} distinct drops over {int(scored.sum())} objects: no threshold separates them"
    i = (len(distinct) - 1) // 2
    V = (float(distinct[i]) + float(distinct[i + 1])) / 2
    keep = ref.selected(drop, kept, V, K)
    assert keep.any() and (scored & ~keep).any(), (V, distinct[i], distinct[i + 1])
    return V, keep


def _stats(d):
    d = np.asarray(d, dtype=np.float64)
    return {"mean": float(d.mean()) if d.size else None, "min": float(d.min()) if d.size else None, "max": float(d.max()) if d.size else None,
            "negative": int(np.count_nonzero(d < 0))}


def test_cli_process_object_value(workdir, capsys):
    from PIL import Image
    root, frames = workdir
    os.makedirs("S")
    stems = [f"f{k}" for k in (1, 2, 3, 10, 11, 12, 20, 21, 100, 101)]
    shown = np.stack([frames[i] for i in (0, 1, 2, 40, 41, 42, 43, 44, 0, 1)])
    for stem, frame in zip(stems, shown):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S")]                     # the order of the reports' frames
    bytes_listed = np.stack([shown[stems.index(s)] for s in listed])
    thr = float(np.median(M))
    labels, mask, kept, _, _ = objects_ref.label(objects_ref.on_pixels(M[:, 0], thr, inclusive=True), 8, 2, 256)
    base, drop, fill_frame, rows = _values(H, bytes_listed, labels, kept)
    V, keep = _threshold(drop, kept)
    scored = np.arange(K)[None] < np.clip(kept, 0, K)[:, None]
    print(f"process: {int(scored.sum())} scored objects, drops {np.unique(drop[scored]).tolist()[:8]} ..., V = {V!r}, selected {int(keep.sum())}")

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2", "--track-iou", "0.5"]
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    _run(common + ["--mask-output-imgs", "R2", "--object-value"], capsys)
    _run(common + ["--mask-output-imgs", "R3", "--object-value", "--min-value-drop", repr(V)], capsys)
    r1, r2, r3 = _files("R1"), _files("R2"), _files("R3")
    assert b"value" not in r1["objects.json"] and b"value" not in r1["tracks.json"] and not any("valued" in f for f in r1)

    def with_values(plain, threshold):
        """What the flags add to the plain objects.json."""
        want = json.loads(plain)
        new = np.where(keep, np.cumsum(keep, axis=1), 0)
        want["object_value"] = {"fill": "low", "fill_frame": listed[fill_frame], "grow": 0, "min_value_drop": threshold, "rows": rows,
                                "unscored": int(np.maximum(kept - K, 0).sum())}
        for i, stem in enumerate(listed):
            frame = want["frames"][stem]
            want["frames"][stem] = {"found": frame["found"], "kept": frame["kept"], "value": float(base[i]), "objects": frame["objects"]}
            for row in frame["objects"]:
                k = row["label"] - 1
                row["value_drop"] = float(drop[i, k]) if k < K else None
                if threshold is not None:
                    row["selected"], row["label_selected"] = bool(k < K and keep[i, k]), int(new[i, k]) if k < K else 0
        return want

    # without a threshold: the same files, the two reports gain the values, everything else is byte for byte the plain run's
    assert set(r2) == set(r1) and all(r2[f] == r1[f] for f in r1 if f not in ("objects.json", "tracks.json"))
    got = json.loads(r2["objects.json"])
    assert got == with_values(r1["objects.json"], None)
    order = objects.natural_order(listed)
    plain_tracks, got = json.loads(r1["tracks.json"]), json.loads(r2["tracks.json"])
    members = {}
    for stem, entries in plain_tracks["frames"].items():
        for e in entries:
            members.setdefault(e["track"], []).append(float(drop[listed.index(stem), e["label"] - 1]))
    for row in plain_tracks["tracks"]:
        d = np.array(members[row["track"]], dtype=np.float64)
        row.update(value_drop_mean=float(d.mean()), value_drop_max=float(d.max()))
    assert got == plain_tracks

    # with the threshold: the selected objects are what the masks and the tracks describe
    assert set(r3) == set(r1) | {f"{s}-valued-mask.png" for s in listed}
    same = [f for f in r1 if f not in ("objects.json", "tracks.json") and not f.endswith(("-objects-mask.png", "-tracks-mask.png"))]
    assert all(r3[f] == r1[f] for f in same)
    assert json.loads(r3["objects.json"]) == with_values(r1["objects.json"], V)
    sel_labels, _, sel_kept, sel_mask, unscored = ref.select(labels, np.zeros((len(labels), 256, 8), dtype=np.int32), kept, keep, K)
    changed = 0
    for i, stem in enumerate(listed):
        png = np.array(Image.open(os.path.join("R3", f"{stem}-valued-mask.png")))
        np.testing.assert_array_equal(png, np.repeat((sel_mask[i] * np.uint8(255))[:, :, None], 3, axis=2))
        assert r3[f"{stem}-objects-mask.png"] == r3[f"{stem}-valued-mask.png"]
        changed += r3[f"{stem}-objects-mask.png"] != r1[f"{stem}-objects-mask.png"]
    assert changed >= 1                                                          # the threshold did remove something that shows
    got = json.loads(r3["tracks.json"])
    assert got["summary"]["objects"] == int(sel_kept.sum()) and got["order"] == [listed[i] for i in order]
    old_of = {(i, int(n)): k for i in range(len(listed)) for k, n in enumerate(np.where(keep[i], np.cumsum(keep[i]), 0)) if n}
    members = {}
    for stem, entries in got["frames"].items():
        i = listed.index(stem)
        assert sorted(e["label"] for e in entries) == list(range(1, int(sel_kept[i]) + 1))
        for e in entries:
            members.setdefault(e["track"], []).append(float(drop[i, old_of[(i, e["label"])]]))
    assert len(got["tracks"]) == len(members)
    for row in got["tracks"]:
        d = np.array(members[row["track"]], dtype=np.float64)
        assert row["value_drop_mean"] == float(d.mean()) and row["value_drop_max"] == float(d.max()) and d.min() >= np.float32(V)
    # the tracker saw the selected labels: objects.track on the reference's selection gives the report's track numbers
    tr = objects.track(torch.from_numpy(sel_labels[order]).to(H.device), iou=0.5)
    trk = tr.track.cpu().numpy()
    for j, i in enumerate(order):
        assert {e["label"]: e["track"] for e in got["frames"][listed[i]]} == {int(l) + 1: int(trk[j, l]) for l in np.flatnonzero(trk[j])}


def test_cli_eval_object_value(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))
    truth = np.load(os.path.join(root, "red-trees", "Y.npy"))[slice(100, 5000, 2)].all(axis=-1)
    labels, mask, kept, _, _ = objects_ref.label(objects_ref.on_pixels(M[:, 0], thr), 8, 4, K)
    truth_labels = objects_ref.label(truth, 8, 1, K)[0]
    base, drop, fill_frame, rows = _values(H, frames, labels, kept)
    V, keep = _threshold(drop, kept)
    scored = np.arange(K)[None] < np.clip(kept, 0, K)[:, None]
    print(f"eval: {int(scored.sum())} scored objects, {len(np.unique(drop[scored]))} distinct drops, V = {V!r}, selected {int(keep.sum())}")
    folder = os.path.join(root, "m")
    read = lambda name: json.load(open(os.path.join(folder, name)))
    plain_files = lambda: {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder)) if os.path.isfile(os.path.join(folder, f))}
    line = lambda text: [ln for ln in text.split("\n") if ln.startswith("OBJECTS")]

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4", "--match-iou", "0.5"]
    _, plain = _run(common, capsys)
    before, plain_objects, plain_match = plain_files(), read("eval_objects.json"), read("eval_match.json")
    assert "value" not in str(plain_objects) and "value" not in str(plain_match) and "value" not in plain

    value = {"fill": "low", "fill_frame": fill_frame, "grow": 0, "rows": rows, "unscored": int(np.maximum(kept - K, 0).sum()),
             "base_mean": float(base.astype(np.float64).mean()), "drop": _stats(drop[scored])}
    best = match_ref.match(labels, truth_labels, [500], K)[1][:, 0].astype(np.int64)
    reach = (best[..., 1] > 0) & (1000 * best[..., 1] >= 500 * (best[..., 2] + best[..., 3] - best[..., 1]))
    side = lambda d: {"n": int(d.size), "mean": float(d.mean()) if d.size else None, "median": float(np.median(d)) if d.size else None}
    match_value = {"matched": side(drop[scored & reach].astype(np.float64)), "spurious": side(drop[scored & ~reach].astype(np.float64))}

    H1, out = _run(common + ["--object-value"], capsys)
    after = plain_files()
    assert set(after) == set(before) and all(after[f] == before[f] for f in before if f not in ("eval_objects.json", "eval_match.json"))
    got = read("eval_objects.json")
    assert H1.objects == got and got["mask"].pop("value") == value and got == plain_objects
    got = read("eval_match.json")
    assert [e.pop("value") for e in got["mask"]["per_iou"]] == [match_value] and got == plain_match
    assert line(out) == [line(plain)[0] + f"; value drop mean {value['drop']['mean']:.6f}, selected {rows}/{rows}"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]

    H2, out = _run(common + ["--object-value", "--min-value-drop", repr(V)], capsys)
    sel_labels, _, sel_kept, sel_mask, unscored = ref.select(labels, np.zeros((len(labels), K, 8), dtype=np.int32), kept, keep, K)
    inter, union = int(np.count_nonzero(sel_mask.astype(bool) & truth)), int(np.count_nonzero(sel_mask.astype(bool) | truth))
    got = read("eval_objects.json")
    assert got["mask"].pop("value") == {**value, "unscored": int(unscored.sum())}
    assert got["mask"].pop("selected") == {"kept": int(sel_kept.sum()), "inter": inter, "union": union, "iou": inter / union if union else None}
    assert got == plain_objects                                                  # the block itself still describes every labelled object
    got = read("eval_match.json")
    assert [e.pop("value") for e in got["mask"]["per_iou"]] == [match_value]    # over the scored objects before the selection
    counts = match_ref.split_counts(match_ref.match(sel_labels, truth_labels, [500], K)[0])
    assert got["mask"]["pred_objects"] == int(sel_kept.sum()) == int(counts[0].sum())
    assert got["mask"]["per_iou"][0]["matched_pred"] == int(counts[2].sum()) and got["mask"]["per_iou"][0]["matched_truth"] == int(counts[3].sum())
    assert line(out) == [line(plain)[0] + f"; value drop mean {value['drop']['mean']:.6f}, selected {int(sel_kept.sum())}/{rows}"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]
