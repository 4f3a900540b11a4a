"""--track-reid end to end on the folder and the synthetic red-trees/ of tests/test_gpu_objects_track_gap.py: what -process -objects and
-eval -objects write with the flag is the plain report plus what tests/objects_reid_ref.py gives on the reference tracker's tracks, and
without the flag nothing changes."""
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
import objects_reid_ref as ref  # noqa: E402
import objects_track_fill_ref as fill_ref  # noqa: E402
import objects_track_gap_ref as track_ref  # noqa: E402
from cgs_amd import cli, handler, objects  # noqa: E402
from test_gpu_objects_track_gap import _files, _run, _side, workdir  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SIM, WINDOW, AREA = 0.8, 16, 4
FLAGS = ["--track-reid", "0.8", "--track-reid-window", "16", "--track-reid-area", "4"]


def _reid(frames, labels, kept, milli, G):
    """(the reference tracker's tracks and report side, the checker's re-identification of them)."""
    t, side = _side(labels, kept, milli, G)
    S, _ = ref.appearance(frames, labels, t["track"], 64)
    return t, side, ref.reid(t["table"], t["extra"] if G else None, S, t["totals"][0], round(SIM * 1000), WINDOW, AREA)


def _block(t, r, G):
    table = t["table"].astype(np.int64)
    last = table[:, 0] + table[:, 2] - 1 + (t["extra"][:, 1] if G else 0)
    u = np.flatnonzero(r["prev"])
    gaps = np.bincount(np.searchsorted([1, 2, 4, 8, 16, 32], table[u, 0] - last[r["prev"][u] - 1]), minlength=7)
    return {"sim": SIM, "window": WINDOW, "min_area": AREA, "bins": 64, "eligible": r["totals"][2], "links": r["totals"][1],
            "identities": r["totals"][0], "longest": r["totals"][3], "link_gaps": dict(zip(objects.LENGTH_BINS, (int(v) for v in gaps)))}


def _add(report, t, r, G):
    """What --track-reid adds to the plain tracks.json."""
    report["track_reid"] = _block(t, r, G)
    members = {}
    for row in report["tracks"]:
        k = row["track"] - 1
        row.update(identity=int(r["identity"][k]), reid_prev=int(r["prev"][k]), reid_sim=int(r["sim"][k]))
        members.setdefault(row["identity"], []).append(row)
    report["identities"] = [{"identity": i, "tracks": [m["track"] for m in rows], "first": rows[0]["first"], "last": rows[-1]["last"],
                             "objects": sum(m["length"] for m in rows)} for i, rows in sorted(members.items())]
    return report


def _painted(labels, per_object):
    """Per pixel the identity of its object (labels 1..64), as colours."""
    out = np.zeros(labels.shape, dtype=np.int64)
    for f in range(len(labels)):
        for l in range(1, 65):
            out[f][labels[f] == l] = per_object[f, l - 1]
    return track_ref.base.colours(out)


def test_cli_process_track_reid(workdir, capsys):
    from PIL import Image
    root, frames = workdir
    os.makedirs("S")
    stems = [f"f{k}" for k in (1, 2, 3, 10, 11, 12, 20, 21, 100, 101)]     # a scene, five frames of another one, the first scene again
    shown = np.stack([frames[i] for i in (0, 1, 2, 40, 41, 42, 43, 44, 0, 1)])
    for stem, frame in zip(stems, shown):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S")]
    thr = float(np.median(M))
    labels, _, kept, _, _ = objects_ref.label(objects_ref.on_pixels(M[:, 0], thr, inclusive=True), 8, 2, 64)
    order = [listed.index(s) for s in stems]
    stack, kept = labels[order], kept[order]

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2", "--track-iou", "0.5"]
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    _run(common + ["--mask-output-imgs", "R2"] + FLAGS, capsys)
    r1, r2 = _files("R1"), _files("R2")
    assert not any("identities" in f for f in r1) and b"reid" not in r1["tracks.json"] and b"identit" not in r1["tracks.json"]
    assert set(r2) == set(r1) | {f"{s}-identities-mask.png" for s in stems}
    assert all(r2[f] == r1[f] for f in r1 if f != "tracks.json")
    t, _, r = _reid(shown, stack, kept, 500, 0)
    print("process: reid totals", r["totals"], "tracks", int(t["totals"][0]), "admissible", r["admissible"])
    assert r["totals"][1] >= 1                                              # the folder has a track that comes back
    assert json.loads(r2["tracks.json"]) == _add(json.loads(r1["tracks.json"]), t, r, 0)
    rgb = _painted(stack, ref.object_identities(t["track"], r["identity"]))
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R2", f"{s}-identities-mask.png"))), rgb[j])

    more = ["--track-gap", "2", "--track-fill"]                              # with a gap and the fill: painted from the filled labels
    _run(common + more + ["--mask-output-imgs", "R3"], capsys)
    _run(common + more + ["--mask-output-imgs", "R4"] + FLAGS, capsys)
    r3, r4 = _files("R3"), _files("R4")
    assert set(r4) == set(r3) | {f"{s}-identities-mask.png" for s in stems} and all(r4[f] == r3[f] for f in r3 if f != "tracks.json")
    t, _, r = _reid(shown, stack, kept, 500, 2)
    print("process, gap 2 and fill: reid totals", r["totals"], "tracks", int(t["totals"][0]))
    assert json.loads(r4["tracks.json"]) == _add(json.loads(r3["tracks.json"]), t, r, 2)
    filled = fill_ref.fill(stack, None, t["prev"], t["gap"], t["track"], 64, 2)
    rgb = _painted(filled["labels"], ref.object_identities(filled["track"], r["identity"]))
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R4", f"{s}-identities-mask.png"))), rgb[j])


def _fragments(pred_labels, truth_labels, pred_ids, truth_ids, milli):
    """objects_track_gap_ref.fragments on identities: distinct (truth identity, predicted identity) pairs less distinct truth identities
    over the covered truth objects."""
    partners = track_ref.base.truth_partners(pred_labels, truth_labels, 64)
    reach = track_ref._reach(partners, milli)
    pairs, truths = set(), set()
    for f in range(len(partners)):
        for q in range(1, 65):
            if reach(f, q):
                pairs.add((int(truth_ids[f, q - 1]), int(pred_ids[f, partners[f][q][0] - 1])))
                truths.add(int(truth_ids[f, q - 1]))
    return len(pairs) - len(truths)


def _plain_files(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder)) if os.path.isfile(os.path.join(folder, f))}


@pytest.mark.parametrize("G", [0, 1])
def test_cli_eval_track_reid(workdir, capsys, G):
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
    truth_labels, _, truth_kept, _, _ = objects_ref.label(truth, 8, 1, 64)
    pt, _, pr = _reid(frames, pred_labels, pred_kept, 300, G)
    tt, _, tr = _reid(frames, truth_labels, truth_kept, 300, G)
    print(f"eval G={G}: pred reid totals", pr["totals"], "truth reid totals", tr["totals"])
    counts = lambda r: {"eligible": r["totals"][2], "links": r["totals"][1], "identities": r["totals"][0], "longest": r["totals"][3]}
    tracks_file = os.path.join(root, "m", "eval_tracks.json")
    line = lambda text: [ln for ln in text.split("\n") if ln.startswith("TRACKS")]

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4", "--match-iou", "0.5", "--track-iou", "0.3"] \
        + (["--track-gap", str(G)] if G else [])
    _, plain = _run(common, capsys)
    before = _plain_files(os.path.join(root, "m"))
    with open(tracks_file) as fp:
        plain_json = json.load(fp)
    assert "reid" not in str(plain_json) and "identit" not in str(plain_json) and "reid" not in plain
    H1, out = _run(common + FLAGS, capsys)
    after = _plain_files(os.path.join(root, "m"))
    assert set(after) == set(before) and all(after[f] == before[f] for f in before if f != "eval_tracks.json")
    with open(tracks_file) as fp:
        got = json.load(fp)
    assert line(out) == [line(plain)[0] + f"; reid {pr['totals'][1]} links, {pr['totals'][0]} identities"]
    assert out.split("RESULTS [")[-1].split("]")[0] == plain.split("RESULTS [")[-1].split("]")[0]
    assert H1.tracks == got
    assert got["truth"].pop("reid") == counts(tr) and got["mask"]["pred"].pop("reid") == counts(pr)
    want = _fragments(pred_labels, truth_labels, ref.object_identities(pt["track"], pr["identity"]),
                      ref.object_identities(tt["track"], tr["identity"]), 500)
    assert [e.pop("fragments_identity") for e in got["mask"]["switches"]] == [want]
    assert got == plain_json
