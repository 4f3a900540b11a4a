"""--graph-cut end to end on the GPU, on the fixtures of tests/test_gpu_clean_cli.py: -process (plain and -fit) on fixture G6, -eval on
the small synthetic red-trees/.  What the runs write must be what graphcut.cut gives when it is called directly on the masks the same
runs return; a run without the flag leaves the files it always left, byte for byte, and the flagged run leaves those same bytes plus
its own files."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from cgs_amd import cli, fit, graphcut, handler, metrics  # noqa: E402
from test_gpu_clean_cli import _grey_rgb, _json, _png, _process, evaldir  # noqa: E402, F401
from test_gpu_objects_match import _read, _results, _run  # noqa: E402
from test_gpu_process_video import workdir  # noqa: E402, F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _levels(M):
    """The median as the threshold and a band around it that leaves a quarter of the cells hard background and a fifth hard foreground
    (float32 values), and the spec written with them: the G6 masks are nearly flat, so the default band would leave every cell unknown."""
    thr, lo, hi = (float(np.float32(np.percentile(M, q))) for q in (50, 25, 80))
    assert lo < thr < hi
    return thr, f"lo={lo!r};hi={hi!r};lambda=30;it=2"


def _direct(frames, M, thr, spec, inclusive):
    res = graphcut.cut(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV), thr,
                       inclusive=inclusive, **graphcut.spec_kwargs(spec))
    return res.mask.cpu().numpy(), res.stats.cpu().numpy().astype(np.int64)


def _cut_json(thr, spec, stats, stems):
    return {"source": "thresholded-mask", "threshold": thr, "lo": spec["lo"], "hi": spec["hi"], **graphcut.cut_report(stats, spec),
            "per_frame": {s: {k: int(v) for k, v in zip(graphcut.STATS, stats[i])} for i, s in enumerate(stems)}}


def _shows(mask, stats, M, thr, inclusive):
    """The cut neither keeps the plain threshold nor fails: about the stack, so that the comparisons below compare something."""
    seed = (M[:, 0] >= np.float32(thr)) if inclusive else (M[:, 0] > np.float32(thr))
    print("stats", stats.sum(axis=0).tolist(), "rounds", stats[:, 2].max())
    return (mask != seed).any() and not (stats[:, 0] & graphcut.NOT_CONVERGED).any() and (stats[:, 1] >= 1).all()


# ---------------------------------------------------------------- -process
def test_process_graph_cut(workdir):
    root, frames, names, calls = workdir
    M0, stems0 = _process([], "S64", "P")
    thr, text = _levels(M0)
    spec, at = graphcut.parse_spec(text), ["--binarymaskthreshold", repr(thr)]
    _process(at, "S64", "R0")
    M, stems = _process(at + ["--graph-cut", text], "S64", "R")
    np.testing.assert_array_equal(M, M0)
    order = [names.index(s) for s in stems]
    mask, stats = _direct(frames[order], M, thr, spec, inclusive=True)
    assert _shows(mask, stats, M, thr, True)
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("R", f"{s}-cut-mask.png")), _grey_rgb(mask[i]), err_msg=s)
    assert _json(os.path.join("R", "cut.json")) == _cut_json(thr, spec, stats, stems)
    # nothing else changes: every file of the run without the flag is there with the same bytes, and only the cut's files are new
    assert set(os.listdir("R")) - set(os.listdir("R0")) == {f"{s}-cut-mask.png" for s in stems} | {"cut.json"}
    assert os.listdir("R0") and set(os.listdir("R0")) <= set(os.listdir("R"))
    for f in os.listdir("R0"):
        assert _read(os.path.join("R", f)) == _read(os.path.join("R0", f)), f
    # -objects --clean read the cut mask, under its own names
    _process(at + ["--graph-cut", text, "-objects", "--track-iou", "0.3"], "S64", "RO")
    rep = _json(os.path.join("RO", "objects.json"))
    assert rep["source"] == "cut-mask" and rep["threshold"] is None and rep["graph_cut"] == spec
    assert _json(os.path.join("RO", "tracks.json"))["source"] == "cut-mask"
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("RO", f"{s}-objects-mask.png")), _grey_rgb(mask[i]), err_msg=s)
    _process(at + ["--graph-cut", text, "-objects", "--clean", "open=1"], "S64", "RC")
    rep = _json(os.path.join("RC", "objects.json"))
    assert rep["source"] == "clean-cut-mask" and rep["graph_cut"] == spec and rep["clean"]["open"] == 1
    clean_rep = _json(os.path.join("RC", "clean.json"))
    assert clean_rep["source"] == "cut-mask" and clean_rep["threshold"] is None and clean_rep["on"] == int(mask.sum())
    assert _json(os.path.join("RC", "cut.json")) == _cut_json(thr, spec, stats, stems)


def test_process_graph_cut_fit(workdir):
    """-fit on the frames replicated to 128 x 128: the cut runs on the shrunk frames and its mask is brought to the frame's size as the
    CRF labels are."""
    root, frames, names, calls = workdir
    thr, text = _levels(_process([], "S64", "P")[0])
    spec, at = graphcut.parse_spec(text), ["--binarymaskthreshold", repr(thr)]
    M, stems = _process(at + ["-fit", "--graph-cut", text, "-concatenated"], "S128", "RF")
    order = [names.index(s) for s in stems]
    guide = torch.from_numpy(np.repeat(np.repeat(frames[order], 2, axis=1), 2, axis=2)).to(DEV)
    low = fit.down(guide)
    mask, stats = _direct(low.cpu().numpy(), M, thr, spec, inclusive=True)
    assert _shows(mask, stats, M, thr, True)
    assert _json(os.path.join("RF", "cut.json")) == _cut_json(thr, spec, stats, stems)
    big = fit.up(torch.from_numpy(mask.view(np.uint8)).to(DEV), guide, low, thresh=0.5, want=("hard",)).hard.cpu().numpy()
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("RF", f"{s}-cut-mask.png")), _grey_rgb(big[i]), err_msg=s)
    assert sorted(os.listdir("RF")) == sorted([f"{s}_with_mask.png" for s in stems] + [f"{s}-cut-mask.png" for s in stems] + ["cut.json", "fit.json"])
    _process(at + ["-fit", "-concatenated"], "S128", "RF0")
    assert sorted(os.listdir("RF0")) == sorted([f"{s}_with_mask.png" for s in stems] + ["fit.json"])
    for f in os.listdir("RF0"):
        assert _read(os.path.join("RF", f)) == _read(os.path.join("RF0", f)), f


# ---------------------------------------------------------------- -eval
def test_eval_graph_cut(evaldir, capsys):
    root, frames = evaldir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr, text = _levels(M)
    spec = graphcut.parse_spec(text)
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    base = ["-eval", "--eval-thresh", repr(thr)]
    reports = ("eval_objects.json", "eval_boundary.json")
    H0, out0 = _run(base + ["-objects", "--boundary-tol", "0-1"], capsys)
    path = os.path.join(root, "m", "eval_cut.json")
    assert H0.cut is None and not os.path.exists(path) and "CUT" not in out0
    before = {f: _read(os.path.join(root, "m", f)) for f in reports}
    objects0, boundary0 = (_json(os.path.join(root, "m", f)) for f in reports)
    assert "cut" not in objects0 and "cut" not in boundary0 and "graph_cut" not in objects0
    # the same run again leaves the same bytes: the reports hold nothing but what the masks give
    _run(base + ["-objects", "--boundary-tol", "0-1"], capsys)
    assert {f: _read(os.path.join(root, "m", f)) for f in reports} == before
    H1, out = _run(base + ["--graph-cut", text, "-objects", "--boundary-tol", "0-1"], capsys)
    rep = _json(path)
    assert H1.cut == rep and _results(out) == _results(out0)
    mask, stats = _direct(frames, M, thr, spec, inclusive=False)
    assert _shows(mask, stats, M, thr, False)
    plain = M[:, 0] > np.float32(thr)

    def counts(pred):
        tp, union = int((pred & truth).sum()), int((pred | truth).sum())
        return {"tp": tp, "fp": int((pred & ~truth).sum()), "fn": int((~pred & truth).sum()), "inter": tp, "union": union,
                "iou": metrics.ratio(tp, union)}
    sums = graphcut.cut_report(stats, spec)
    assert rep == {"graph_cut": spec, "threshold": thr, "lo": spec["lo"], "hi": spec["hi"], "before": counts(plain), "after": counts(mask),
                   "stats": {k: v for k, v in sums.items() if k != "spec"}}
    assert rep["before"] != rep["after"] and rep["stats"]["seed_on"] == int(plain.sum()) and rep["stats"]["on"] == int(mask.sum())
    assert out.count("\nCUT " + graphcut.spec_text(spec) + ": iou ") == 1 and out.index("\nCUT ") < out.index("OBJECTS") < out.index("RESULTS")
    # the object and outline reports gain the cut mask where the CRF mask would stand; what they say about the plain mask stays
    objects1, boundary1 = (_json(os.path.join(root, "m", f)) for f in reports)
    assert objects1["mask"] == objects0["mask"] and boundary1["mask"] == boundary0["mask"]
    assert set(objects1) - set(objects0) == {"cut"} and set(boundary1) - set(boundary0) == {"cut"}
    assert objects1["cut"]["unfiltered"] == {k: rep["after"][k] for k in ("inter", "union", "iou")} and "per_tol" in boundary1["cut"]
    assert "; cut iou " in out
    # two refinements, one slot: refused before a Handler is made
    with pytest.raises(ValueError, match="-crf"):
        cli.main(base + ["-crf", "--graph-cut", text, "--model", "m"])
