"""--track-fill end to end on the folder and the synthetic red-trees/ of tests/test_gpu_objects_track_gap.py: what -process -objects and
-eval -objects write with the flag is what tests/objects_track_fill_ref.py gives on the reference tracker's tracks, and without the flag
nothing changes."""
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
import objects_track_fill_ref as ref  # noqa: E402
from cgs_amd import cli, handler  # noqa: E402
from test_gpu_objects_track_gap import _files, _run, _side, workdir  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def test_cli_process_track_fill(workdir, capsys):
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
    stack = labels[order]
    t, _ = _side(stack, kept[order], 300, 2)
    want = ref.fill(stack, None, t["prev"], t["gap"], t["track"], 64, 2)
    print("process: fill totals", want["totals"].tolist(), "links by gap", t["gap_links"].tolist())
    assert t["gap_links"][1:].sum() > 0 and want["totals"][0] > 0 and want["totals"][1] > 0      # the folder has something to fill

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2", "--track-iou", "0.3",
              "--track-gap", "2"]
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    _run(common + ["--mask-output-imgs", "R2", "--track-fill"], capsys)
    r1, r2 = _files("R1"), _files("R2")
    assert "fill" not in r1["tracks.json"].decode() and not any("filled" in f for f in r1)
    assert set(r2) == set(r1) | {f"{s}-filled-mask.png" for s in stems}
    assert all(r2[f] == r1[f] for f in r1 if "tracks" not in f) and r2["objects.json"] == r1["objects.json"]

    report = json.loads(r1["tracks.json"])                                  # (test_gpu_objects_track_gap.py holds it against the tracker's checker)
    report["track_fill"] = dict(zip(ref.TOTALS, (int(v) for v in want["totals"])))
    for j, s in enumerate(stems):
        report["frames"][s] += [{"label": int(l) + 1, "track": int(want["track"][j, l]), "filled": int(want["age"][j, l]),
                                 "area": int(want["table"][j, l, 0])} for l in np.flatnonzero(want["age"][j])]
    per_track = np.bincount(want["track"][want["age"] > 0], minlength=len(report["tracks"]) + 1)
    for row in report["tracks"]:
        row["filled"] = int(per_track[row["track"]])
    assert json.loads(r2["tracks.json"]) == report
    assert sum(row["filled"] for row in report["tracks"]) == want["totals"][0]
    assert all(row["filled"] <= row["missed"] for row in report["tracks"])
    _, rgb = ref.paint(want["labels"], want["track"], 64)
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R2", f"{s}-tracks-mask.png"))), rgb[j])
        grey = (want["labels"][j] > 0) * np.uint8(255)
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R2", f"{s}-filled-mask.png"))), np.repeat(grey[:, :, None], 3, axis=2))


def test_cli_eval_track_fill(workdir, capsys):
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
    G = 2
    pt, pred_side = _side(pred_labels, pred_kept, 300, G)
    want = ref.fill(pred_labels, None, pt["prev"], pt["gap"], pt["track"], 64, G)
    print("eval: fill totals", want["totals"].tolist(), "links by gap", pt["gap_links"].tolist())
    assert pred_side["bridged_links"] > 0 and want["totals"][0] > 0         # the stack has bridged links at this threshold and gap
    before, after = pred_labels > 0, want["labels"] > 0
    counts = lambda on: (int((on & truth).sum()), int((on | truth).sum()))
    (inter0, union0), (inter, union) = counts(before), counts(after)
    assert after.sum() == before.sum() + want["totals"][1]
    block = {**dict(zip(ref.TOTALS, (int(v) for v in want["totals"]))), "inter": inter, "union": union, "iou": inter / union,
             "inter_before": inter0, "union_before": union0, "iou_before": inter0 / union0}
    tracks_file = os.path.join(root, "m", "eval_tracks.json")
    line = lambda text: [ln for ln in text.split("\n") if ln.startswith("TRACKS")]

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4", "--match-iou", "0.5", "--track-iou", "0.3", "--track-gap", str(G)]
    _, plain = _run(common, capsys)
    with open(tracks_file) as fp:
        plain_json = json.load(fp)
    assert "fill" not in str(plain_json) and "filled" not in plain
    H1, out = _run(common + ["--track-fill"], capsys)
    with open(tracks_file) as fp:
        filled_json = json.load(fp)
    assert line(out) == [line(plain)[0] + f"; filled {block['objects']} objects, iou {block['iou_before']:.6f} -> {block['iou']:.6f}"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]
    assert filled_json["mask"].pop("fill") == block and filled_json == plain_json and H1.tracks["mask"]["fill"] == block
