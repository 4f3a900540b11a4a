"""--clean and --overlay-clean end to end on the GPU: -process (plain, -fit, -crf) on fixture G6, -eval on a small synthetic red-trees/,
--source-video with the stub `ffprobe` / `ffmpeg` of tests/test_gpu_process_video.py.  What the runs write must be what
tests/clean_ref.py makes of the masks the same runs return, exactly; without the flags the paths leave the files they always left."""
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

import clean_ref  # noqa: E402
from cgs_amd import clean, cli, fit, handler, metrics, objects  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402
from test_gpu_objects_match import _read, _results, _run  # noqa: E402
from test_gpu_process_video import _encoder_call, _video, workdir  # noqa: E402, F401  (G6 as folders and as a raw video, the stub tools)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _levels(M):
    """A threshold that half of the masks' cells reach and a strong level that three in ten reach (float32 values), the spec written
    with them and the checker's keywords: the G6 masks are nearly flat, so fixed levels would keep all of a frame or none of it."""
    thr, strong = float(np.median(M)), float(np.float32(np.percentile(M, 70)))
    assert thr < strong
    return thr, f"hyst={strong!r};open=1;close=1;fill=8", dict(strong=strong, open=1, close=1, fill=8, shape="square", connectivity=8)


def _shows(want, M, thr):
    """The clean-up neither keeps the plain threshold nor empties the stack: about the checker's output, not the kernel's."""
    print("counts", want.counts.sum(axis=0).tolist())
    return 0 < want.counts[:, 4].sum() and (want.mask != (M[:, 0] >= np.float32(thr))).any()


def _process(argv, folder, out):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-imgs", folder, "--mask-output-imgs", out] + argv))
    assert H.load_models()
    M = H.segment(folder)
    return M, [f.rsplit(".", 1)[0] for f in os.listdir(folder)]


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _grey_rgb(mask):
    return np.repeat((np.asarray(mask) != 0)[:, :, None] * np.uint8(255), 3, axis=2)


def _json(path):
    with open(path) as fp:
        return json.load(fp)


def _clean_json(source, thresh, spec, counts, stems):
    c = counts.astype(np.int64)
    return {"source": source, "threshold": thresh, "spec": spec, "frames": len(stems),
            **{k: int(v) for k, v in zip(clean.COUNTS, c.sum(axis=0))},
            "per_frame": {s: {k: int(v) for k, v in zip(clean.COUNTS, c[i])} for i, s in enumerate(stems)}}


# ---------------------------------------------------------------- -process
def test_process_clean_objects_and_tracks(workdir):
    root, frames, names, calls = workdir
    thr, text, kw = _levels(_process([], "S64", "P")[0])
    spec, at = clean.parse_clean(text), ["--binarymaskthreshold", repr(thr)]
    M, stems = _process(at + ["--clean", text, "-objects", "--track-iou", "0.3"], "S64", "R")
    want = clean_ref.clean(M[:, 0], thresh=thr, inclusive=True, **kw)
    assert _shows(want, M, thr)
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("R", f"{s}-clean-mask.png")), _grey_rgb(want.mask[i]), err_msg=s)
    assert _json(os.path.join("R", "clean.json")) == _clean_json("thresholded-mask", thr, spec, want.counts, stems)
    # objects.json describes the cleaned stack: objects.label of the checker's mask
    res = objects.label(torch.from_numpy(want.mask).to(DEV), connectivity=8, min_area=1, max_objects=256, want_mask=True)
    rows = objects.table_rows(res.table, res.kept, width=64)
    rep = _json(os.path.join("R", "objects.json"))
    assert {k: rep[k] for k in ("source", "threshold", "connectivity", "min_area", "clean")} == \
        {"source": "clean-mask", "threshold": thr, "connectivity": 8, "min_area": 1, "clean": spec}
    kept, found = res.kept.cpu().numpy(), res.found.cpu().numpy()
    assert rep["frames"] == {s: {"found": int(found[i]), "kept": int(kept[i]), "objects": rows[i]} for i, s in enumerate(stems)}
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("R", f"{s}-objects-mask.png")), _grey_rgb(want.mask[i]), err_msg=s)
    tracks = _json(os.path.join("R", "tracks.json"))
    assert tracks["source"] == "clean-mask" and tracks["clean"] == spec and tracks["summary"]["objects"] == int(kept.clip(max=64).sum())
    # the columns are untouched and nothing else appears: a run without the flag leaves the same bytes under the same names
    M0, _ = _process(at + ["-objects", "--track-iou", "0.3"], "S64", "R0")
    np.testing.assert_array_equal(M0, M)
    extra = {f"{s}-clean-mask.png" for s in stems} | {"clean.json"}
    assert set(os.listdir("R")) - set(os.listdir("R0")) == extra and set(os.listdir("R0")) <= set(os.listdir("R"))
    for f in os.listdir("R0"):
        if f.endswith(("-raw-mask.png", "-thresholded-mask.png")):
            assert _read(os.path.join("R", f)) == _read(os.path.join("R0", f)), f
    rep0 = _json(os.path.join("R0", "objects.json"))
    assert rep0["source"] == "thresholded-mask" and "clean" not in rep0 and "clean" not in _json(os.path.join("R0", "tracks.json"))


def test_process_clean_fit_and_crf(workdir):
    root, frames, names, calls = workdir
    thr, text, kw = _levels(_process([], "S64", "P")[0])
    spec, at = clean.parse_clean(text), ["--binarymaskthreshold", repr(thr)]
    # -fit on the frames replicated to 128 x 128: the same 64 x 64 masks, the PNG brought to the frame's size as the CRF labels are
    M, stems = _process(at + ["-fit", "--clean", text, "-concatenated"], "S128", "RF")
    want = clean_ref.clean(M[:, 0], thresh=thr, inclusive=True, **kw)
    assert _shows(want, M, thr)
    assert _json(os.path.join("RF", "clean.json")) == _clean_json("thresholded-mask", thr, spec, want.counts, stems)
    order = [names.index(s) for s in stems]
    guide = torch.from_numpy(np.repeat(np.repeat(frames[order], 2, axis=1), 2, axis=2)).to(DEV)
    big = fit.up(torch.from_numpy(want.mask.view(np.uint8)).to(DEV), guide, thresh=0.5, want=("hard",)).hard.cpu().numpy()
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("RF", f"{s}-clean-mask.png")), _grey_rgb(big[i]), err_msg=s)
    assert sorted(os.listdir("RF")) == sorted([f"{s}_with_mask.png" for s in stems] + [f"{s}-clean-mask.png" for s in stems]
                                              + ["clean.json", "fit.json"])
    _process(at + ["-fit", "-concatenated"], "S128", "RF0")
    assert sorted(os.listdir("RF0")) == sorted([f"{s}_with_mask.png" for s in stems] + ["fit.json"])
    for s in stems:
        assert _read(os.path.join("RF", f"{s}_with_mask.png")) == _read(os.path.join("RF0", f"{s}_with_mask.png")), s
    # -crf: the CRF labels are the source, also at --binarymaskthreshold 0 (the CRF column is then the second one, named by position)
    hard_spec = clean.parse_clean("open=1;fill=8;conn=4")
    _, stems = _process(["-crf", "--binarymaskthreshold", "0", "--clean", "open=1;fill=8;conn=4", "-objects"], "S64", "RC")
    labels = np.stack([_png(os.path.join("RC", f"{s}-thresholded-mask.png"))[:, :, 0] > 0 for s in stems])
    want = clean_ref.clean(labels, open=1, fill=8, connectivity=4)
    print("crf counts", want.counts.sum(axis=0).tolist())
    assert _json(os.path.join("RC", "clean.json")) == _clean_json("crf-mask", None, hard_spec, want.counts, stems)
    for i, s in enumerate(stems):
        np.testing.assert_array_equal(_png(os.path.join("RC", f"{s}-clean-mask.png")), _grey_rgb(want.mask[i]), err_msg=s)
    rep = _json(os.path.join("RC", "objects.json"))
    assert rep["source"] == "clean-crf-mask" and rep["threshold"] is None and rep["clean"] == hard_spec


# ---------------------------------------------------------------- -eval
@pytest.fixture()
def evaldir(tmp_path, golden, g1, monkeypatch):
    """A synthetic red-trees/ of 112 frames (6 evaluated) and the G1 checkpoints under the names of G6; the test paints its truth."""
    root = str(tmp_path)
    for name, state in zip([str(s) for s in golden("g6_process.npz")["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    Xe = np.stack([_structured(64, 64, 200 + k)[0] for k in range(112)])
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), np.zeros((112, 64, 64, 3), dtype=bool))
    monkeypatch.chdir(root)
    return root, Xe[slice(100, 5000, 2)]


def _scores(pred, truth):
    inter, union = int((pred & truth).sum()), int((pred | truth).sum())
    return {"inter": inter, "union": union, "iou": metrics.ratio(inter, union), "precision": metrics.ratio(inter, int(pred.sum())),
            "recall": metrics.ratio(inter, int(truth.sum()))}


def test_eval_clean(evaldir, capsys):
    root, frames = evaldir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr, strong = float(np.median(M)), float(np.float32(np.percentile(M, 80)))
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    text = f"hyst={strong!r};open=1;fill=8"
    spec = clean.parse_clean(text)
    want = clean_ref.clean(M[:, 0], thresh=thr, inclusive=False, strong=strong, open=1, fill=8)
    plain = M[:, 0] > np.float32(thr)
    sums = want.counts.astype(np.int64).sum(axis=0)
    print("eval counts", sums.tolist())
    block = {**_scores(want.mask, truth), "uncleaned": _scores(plain, truth), "counts": {k: int(v) for k, v in zip(clean.COUNTS, sums)}}
    assert block["counts"]["on"] == int(plain.sum()) and block["inter"] != block["uncleaned"]["inter"]       # the clean-up shows
    base = ["-eval", "--eval-thresh", repr(thr)]
    H0, out0 = _run(base + ["-objects", "--boundary-tol", "0-1"], capsys)
    path = os.path.join(root, "m", "eval_clean.json")
    assert H0.clean is None and not os.path.exists(path) and "CLEAN" not in out0
    objects0, boundary0 = _json(os.path.join(root, "m", "eval_objects.json")), _json(os.path.join(root, "m", "eval_boundary.json"))
    assert "clean" not in objects0 and "mask_clean" not in boundary0
    H1, out = _run(base + ["--clean", text, "-objects", "--boundary-tol", "0-1"], capsys)
    rep = _json(path)
    assert rep == {"clean": spec, "threshold": thr, "mask_clean": block} and H1.clean == rep
    assert _results(out) == _results(out0)
    fmt = lambda v: "nan" if v is None else f"{v:.6f}"
    line = (f"CLEAN {clean.spec_text(spec)}: iou {fmt(block['iou'])} (uncleaned {fmt(block['uncleaned']['iou'])}), "
            f"{block['counts']['holes_filled']} holes filled, {block['counts']['components_dropped']} components dropped")
    assert out.count("\n" + line + "\n") == 1 and out.index("CLEAN") < out.index("OBJECTS") < out.index("RESULTS")
    # the object and outline reports read the cleaned stack
    objects1, boundary1 = _json(os.path.join(root, "m", "eval_objects.json")), _json(os.path.join(root, "m", "eval_boundary.json"))
    assert objects1["clean"] == spec
    assert objects1["mask"]["unfiltered"] == {k: block[k] for k in ("inter", "union", "iou")}
    assert boundary1["mask"] == boundary0["mask"] and set(boundary1) - set(boundary0) == {"mask_clean"} and "per_tol" in boundary1["mask_clean"]
    # with -crf the hard source is cleaned too; a spec with hyst is refused before a Handler is made
    with pytest.raises(ValueError, match="hyst"):
        cli.main(base + ["-crf", "--clean", text, "--model", "m"])
    H2, out2 = _run(base + ["-crf", "--clean", "close=1;fill=16"], capsys)
    rep2 = _json(path)
    crf_on = H2.crf(frames, M, truth)[:, 0]
    want2 = clean_ref.clean(crf_on, close=1, fill=16)
    assert rep2["crf_clean"] == {**_scores(want2.mask, truth), "uncleaned": _scores(crf_on, truth),
                                 "counts": {k: int(v) for k, v in zip(clean.COUNTS, want2.counts.astype(np.int64).sum(axis=0))}}
    assert "; crf iou " in out2 and set(rep2) == {"clean", "threshold", "mask_clean", "crf_clean"}


# ---------------------------------------------------------------- --source-video
def test_video_overlay_clean_in_chunks(workdir, monkeypatch):
    root, frames, names, calls = workdir
    thr, text, kw = _levels(_video(["--smooth", "1"], out="levels.mp4", results="RL")[1])
    tracked = ["--binarymaskthreshold", repr(thr), "--smooth", "1", "--overlay-tracks", "0.3", "--overlay-layout", "triple"]
    _, M0 = _video(tracked, out="plain.mp4", results="R0")
    _, sent0 = _encoder_call(calls, 1, 128, 384)
    rep0 = _json(os.path.join("R0", "plain.json"))
    assert "clean" not in rep0 and sorted(os.listdir("R0")) == ["plain-objects.json", "plain-tracks.json", "plain.json"]
    spec = clean.parse_clean(text)
    want = clean_ref.clean(M0[:, 0], thresh=thr, inclusive=True, want_gated=True, **kw)
    assert _shows(want, M0, thr)
    sent = {}
    for i, chunk in enumerate((128, 3)):
        monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", chunk)
        _, M = _video(tracked + ["--overlay-clean", text], out=f"c{chunk}.mp4", results=f"R{chunk}")
        assert M.dtype == np.float32 and M.shape == M0.shape
        np.testing.assert_array_equal(M[:, 0].view(np.int32), want.gated.view(np.int32), err_msg=f"chunks of {chunk}")
        np.testing.assert_array_equal(M[:, 0] >= np.float32(thr), want.mask)
        _, sent[chunk] = _encoder_call(calls, 2 + i, 128, 384)
        rep = _json(os.path.join(f"R{chunk}", f"c{chunk}.json"))
        assert rep["clean"] == {"spec": spec, "frames": len(M), **{k: int(v) for k, v in zip(clean.COUNTS, want.counts.astype(np.int64).sum(axis=0))}}
        assert {k: v for k, v in rep.items() if k not in ("clean", "tracks")} == {k: v for k, v in rep0.items() if k != "tracks"}
        # the object report describes the cleaned masks
        objs = _json(os.path.join(f"R{chunk}", f"c{chunk}-objects.json"))
        res = objects.label(torch.from_numpy(want.mask).to(DEV), connectivity=8, min_area=1, max_objects=256)
        assert [objs["frames"][f"{j:06d}"]["kept"] for j in range(len(M))] == res.kept.cpu().tolist()
    np.testing.assert_array_equal(sent[128], sent[3])
    assert (sent[128] != sent0).any()                                  # the clean-up shows in the video
