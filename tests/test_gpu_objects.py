"""Object labelling on the GPU (cgs_objects_label, cgs_amd.objects, -process -objects / -eval -objects) against the raster-scan flood
fill of tests/objects_ref.py.  Everything is integer: exact equality everywhere."""
import functools
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

import metrics_ref  # noqa: E402
import objects_ref  # noqa: E402
from cgs_amd import cli, handler, objects  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERNS = objects_ref.patterns()
RANDOMS = ("random0.3", "random0.45", "random0.593", "random0.7")
MIN_AREAS = (1, 2, 4, 4097)


@functools.lru_cache(maxsize=None)
def _ref(name, conn, min_area, max_objects=64):
    """The checker's answer for one named 64 x 64 pattern: computed once, shared, never written to."""
    out = objects_ref.label_frame(PATTERNS[name], conn, min_area, max_objects)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _gpu(src, **kw):
    """objects.label with both optional outputs, everything back on the host."""
    t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    res = objects.label(t, want_labels=True, want_mask=True, **kw)
    torch.cuda.synchronize()
    n, (h, w) = res.kept.shape[0], res.labels.shape[1:]
    assert res.labels.dtype == torch.int32 and res.labels.shape == (n, h, w)
    assert res.mask.dtype == torch.bool and res.mask.shape == (n, h, w)
    assert res.kept.dtype == torch.int32 and res.found.dtype == torch.int32 and res.found.shape == (n,)
    assert res.table.dtype == torch.int32 and res.table.shape == (n, kw.get("max_objects", 64), 8)
    assert all(t.device.type == "cuda" for t in res)
    return tuple(t.cpu().numpy() for t in res)


def _same(got, want):
    for g, w, what in zip(got, want, ("labels", "kept mask", "kept", "found", "table")):
        np.testing.assert_array_equal(g, w, err_msg=what)


def _check(on, conn, min_area, max_objects=64, **kw):
    """on: bool [n,h,w], labelled as a bool stack unless kw says otherwise."""
    want = objects_ref.label(on, conn, min_area, max_objects)
    _same(_gpu(kw.pop("src", on), connectivity=conn, min_area=min_area, max_objects=max_objects, **kw), want)
    return want


# ---------------------------------------------------------------- the 64 x 64 patterns
def test_patterns_are_what_the_issue_describes():
    assert PATTERNS["spiral"].sum() == 2111 and _ref("spiral", 4, 1)[3] == 1 and _ref("spiral", 8, 1)[3] == 1
    for name in ("comb", "serpentine", "full"):
        assert _ref(name, 4, 1)[3] == 1 and _ref(name, 8, 1)[3] == 1
    assert _ref("checkerboard", 4, 1)[3] == 2048 and _ref("checkerboard", 8, 1)[3] == 1 and _ref("empty", 8, 1)[3] == 0
    assert [(_ref(r, 4, 1)[3], _ref(r, 8, 1)[3]) for r in RANDOMS] == [(570, 205), (407, 40), (150, 7), (44, 1)]
    # the connectivity switch and the filter are observable on the random frames: about the checker's output, not the kernel's
    for r in RANDOMS:
        assert not np.array_equal(_ref(r, 4, 1)[0], _ref(r, 8, 1)[0])
    for conn, small in ((4, 280), (8, 29)):
        found, kept4 = _ref("random0.45", conn, 1)[3], _ref("random0.45", conn, 4)[2]
        assert found - kept4 == small and 0 < kept4 < found


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_patterns(name, conn):
    for min_area in MIN_AREAS:
        want = _ref(name, conn, min_area)
        got = _gpu(PATTERNS[name], connectivity=conn, min_area=min_area)
        _same(got, [np.asarray(w)[None] for w in want])


# ---------------------------------------------------------------- other shapes, row ends
def _row_ends(h, w):
    """Pixels on at (y, w-1) and (y+1, 0) and nothing else in those rows: neighbours in memory, not in the image."""
    a = np.zeros((h, w), dtype=bool)
    for y in range(0, h - 1, 3):
        a[y, w - 1] = a[y + 1, 0] = True
    return a


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (37, 64), (64, 33)])
def test_other_shapes(h, w, conn):
    rs = np.random.RandomState(100 * h + w)
    ends = _row_ends(h, w)
    mixed = rs.rand(h, w) < 0.5
    rows = ends.any(axis=1)
    mixed[rows] = ends[rows]                          # the random frame keeps the bare row ends
    diag = np.zeros((h, w), dtype=bool)               # the same in every row: (y, w-1) on even rows, (y, 0) on odd ones
    diag[0::2, w - 1] = True
    diag[1::2, 0] = True
    stack = np.stack([np.ones((h, w), dtype=bool), ends, mixed, diag, rs.rand(h, w) < 0.45, np.zeros((h, w), dtype=bool)])
    if h > 1 and w > 2:
        assert objects_ref.label_frame(ends, 8, 1)[3] == ends.sum()           # the checker keeps every row-end pixel apart
    for min_area in (1, 2):
        _check(stack, conn, min_area)


# ---------------------------------------------------------------- several frames in one launch
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("n", [1, 37])
def test_frames_of_one_launch_do_not_leak(n, conn):
    names = list(PATTERNS)                            # ... "full", "empty" ...: a full frame next to an empty one
    assert names.index("empty") == names.index("full") + 1
    order = [names[(k + 4) % len(names)] for k in range(n)]
    stack = np.stack([PATTERNS[k] for k in order])
    for min_area in (1, 4):
        want = [np.stack([np.asarray(_ref(k, conn, min_area)[i]) for k in order]) for i in range(5)]
        _same(_gpu(stack, connectivity=conn, min_area=min_area), want)


# ---------------------------------------------------------------- source kinds
def test_uint8_and_bool_sources():
    rs = np.random.RandomState(3)
    u8 = rs.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=(3, 64, 33))
    assert set(np.unique(u8)) == {0, 1, 2, 255}
    want = _check(u8 != 0, 8, 2, src=u8)
    _same(_gpu(torch.from_numpy(u8 != 0).to(DEV), connectivity=8, min_area=2), want)


def test_float_sources_strict_and_inclusive():
    rs = np.random.RandomState(4)
    thr = np.float32(0.3)
    v = rs.rand(4, 37, 64).astype(np.float32)
    flat = v.reshape(-1)
    flat[rs.choice(flat.size, 1500, replace=False)] = thr                        # exactly at the threshold
    sp = rs.choice(flat.size, 300, replace=False)
    flat[sp] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(300) % 3]
    strict, incl = objects_ref.on_pixels(v, thr), objects_ref.on_pixels(v, thr, inclusive=True)
    assert not np.array_equal(strict, incl)
    assert not strict[np.isnan(v)].any() and not incl[np.isnan(v)].any() and incl[np.isposinf(v)].all() and not incl[np.isneginf(v)].any()
    for conn in (4, 8):
        a = _check(strict, conn, 3, src=v, thresh=float(thr))
        b = _check(incl, conn, 3, src=v, thresh=float(thr), inclusive=True)
        assert not np.array_equal(a[0], b[0])                                    # the checker tells the two compares apart
    # an infinite threshold: nothing is > inf; +inf is >= inf
    _check(objects_ref.on_pixels(v, np.inf), 8, 1, src=v, thresh=float("inf"))
    _check(objects_ref.on_pixels(v, np.inf, inclusive=True), 8, 1, src=v, thresh=float("inf"), inclusive=True)


def test_non_contiguous_source():
    rs = np.random.RandomState(5)
    big = torch.from_numpy(rs.rand(3, 64, 128).astype(np.float32)).to(DEV)
    view = big[:, :, ::2]                                                        # [3,64,64], stride 2
    assert not view.is_contiguous()
    _check(objects_ref.on_pixels(view.cpu().numpy(), 0.5), 8, 2, src=view, thresh=0.5)
    tv = torch.from_numpy(rs.rand(64, 40) < 0.5).to(DEV).t()                     # one [40,64] frame, transposed
    assert not tv.is_contiguous()
    _check(tv.cpu().numpy()[None], 4, 1, src=tv)


# ---------------------------------------------------------------- table cap, optional outputs
@pytest.mark.parametrize("max_objects", [1, 64, 2048])
def test_table_cap(max_objects):
    board = PATTERNS["checkerboard"]
    labels, mask, kept, found, table = _gpu(board, connectivity=4, max_objects=max_objects)
    want = _ref("checkerboard", 4, 1, max_objects)
    assert kept.tolist() == [2048] and found.tolist() == [2048] and labels.max() == 2048
    np.testing.assert_array_equal(labels[0], want[0])
    np.testing.assert_array_equal(table[0], want[4])
    assert (table[0][:, 0] == 1).all() and table[0][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]        # every row an object of one pixel
    labels, mask, kept, found, table = _gpu(board, connectivity=4, min_area=2, max_objects=max_objects)
    assert kept.tolist() == [0] and found.tolist() == [2048] and not labels.any() and not mask.any() and not table.any()
    # a stale table is overwritten, zero rows included
    labels, mask, kept, found, table = _gpu(np.stack([PATTERNS["random0.45"], PATTERNS["empty"]]), connectivity=8, max_objects=max_objects)
    np.testing.assert_array_equal(table[0], _ref("random0.45", 8, 1, max_objects)[4])
    assert kept.tolist() == [40, 0] and not table[1].any()


def test_optional_outputs():
    stack = np.stack([PATTERNS["random0.45"], PATTERNS["spiral"], PATTERNS["random0.3"]])
    dev = torch.from_numpy(stack).to(DEV)
    both = _gpu(dev, connectivity=4, min_area=3)
    only_mask = objects.label(dev, connectivity=4, min_area=3, want_labels=False, want_mask=True)
    only_labels = objects.label(dev, connectivity=4, min_area=3, want_labels=True, want_mask=False)
    default = objects.label(dev, connectivity=4, min_area=3)
    neither = objects.label(dev, connectivity=4, min_area=3, want_labels=False)
    assert only_mask.labels is None and only_labels.mask is None and default.mask is None and neither.labels is None and neither.mask is None
    np.testing.assert_array_equal(only_mask.mask.cpu().numpy(), both[1])
    np.testing.assert_array_equal(only_labels.labels.cpu().numpy(), both[0])
    np.testing.assert_array_equal(default.labels.cpu().numpy(), both[0])
    for res in (only_mask, only_labels, default, neither):
        _same((res.kept.cpu().numpy(), res.found.cpu().numpy(), res.table.cpu().numpy()), both[2:])
    # a [h,w] tensor is one frame
    one = objects.label(dev[0], connectivity=4, min_area=3)
    np.testing.assert_array_equal(one.labels.cpu().numpy(), both[0][:1])


# ---------------------------------------------------------------- Handler and CLI
def _run(argv, capsys):
    capsys.readouterr()
    H = cli.main(argv + ["--model", "m"])
    return H, capsys.readouterr().out


def _results(out):
    return out.split("RESULTS [")[-1].split("]")[0]


def _block(on, truth, conn, min_area):
    """What one block of eval_objects.json must hold for the on-mask `on`, from the checker and metrics_ref."""
    _, kept_mask, kept, found, _ = objects_ref.label(on, conn, min_area, 1)
    (inter, union), (inter0, union0) = metrics_ref.counts(kept_mask, truth)[0].tolist(), metrics_ref.counts(on, truth)[0].tolist()
    block = {"inter": inter, "union": union, "iou": inter / union if union else None,
             "unfiltered": {"inter": inter0, "union": union0, "iou": inter0 / union0 if union0 else None},
             "found": int(found.sum()), "kept": int(kept.sum()), "frames_without_objects": int(np.count_nonzero(kept == 0))}
    return block, found, kept


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The synthetic red-trees/ and G1 checkpoints of test_gpu_metrics.py::test_cli_eval_sweeps, 420 frames (160 evaluated)."""
    root = str(tmp_path)
    for name, state in zip([str(s) for s in golden("g6_process.npz")["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    rs = np.random.RandomState(11)
    Xe = np.stack([_structured(64, 64, 200 + k % 40)[0] for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    Ye[:, 20:30, 10:20, 1] = rs.rand(10, 10) < 0.5
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    monkeypatch.chdir(root)
    pick = slice(100, 5000, 2)
    return root, Xe[pick], Ye[pick].all(axis=-1)


def test_cli_eval_objects(workdir, capsys):
    root, frames, truth = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))                                        # a float32 value: half of the pixels are above it
    on = objects_ref.on_pixels(M[:, 0], thr)
    want, found, kept = _block(on, truth, 8, 4)
    assert found.max() >= 2 and kept.sum() < found.sum()             # the checker sees several objects in a frame, and the filter bites
    report_file = os.path.join(root, "m", "eval_objects.json")

    _, base = _run(["-eval", "--eval-thresh", repr(thr)], capsys)
    assert not os.path.exists(report_file) and "OBJECTS" not in base
    H1, out = _run(["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4"], capsys)
    assert out.count("OBJECTS conn=8 min_area=4: iou ") == 1 and out.index("OBJECTS") < out.index("RESULTS")
    assert f"kept {want['kept']}/found {want['found']} objects" in out
    assert _results(out) == _results(base)
    with open(report_file) as fp:
        report = json.load(fp)
    assert report == H1.objects == {"connectivity": 8, "min_area": 4, "threshold": thr, "mask": want}

    _, base = _run(["-eval", "-crf", "--eval-thresh", repr(thr)], capsys)
    assert "OBJECTS" not in base
    H2, out = _run(["-eval", "-crf", "--eval-thresh", repr(thr), "-objects", "--min-area", "3", "--connectivity", "4"], capsys)
    assert _results(out) == _results(base) and out.count("OBJECTS conn=4 min_area=3: iou ") == 1
    with open(report_file) as fp:
        report = json.load(fp)
    crf_on = H.crf(frames, M, truth)[:, 0]
    assert report == H2.objects == {"connectivity": 4, "min_area": 3, "threshold": thr, "mask": _block(on, truth, 4, 3)[0],
                                    "crf": _block(crf_on, truth, 4, 3)[0]}


def _files(folder):
    out = {}
    for f in sorted(os.listdir(folder)):
        with open(os.path.join(folder, f), "rb") as fp:
            out[f] = fp.read()
    return out


def test_cli_process_objects(workdir, capsys):
    from PIL import Image
    root, frames, _ = workdir
    os.makedirs("S")
    stems = [f"frame{k}" for k in range(5)]
    for stem, frame in zip(stems, frames[::8]):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")                                              # the masks of these frames, in os.listdir's order
    order = [f.rsplit(".", 1)[0] for f in os.listdir("S")]
    thr = float(np.median(M))
    on = objects_ref.on_pixels(M[:, 0], thr, inclusive=True)
    labels, kept_mask, kept, found, table = objects_ref.label(on, 8, 2, 256)
    assert found.max() >= 2 and kept.sum() < found.sum()

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr)]
    _, base = _run(common + ["--mask-output-imgs", "R1"], capsys)
    _, out = _run(common + ["--mask-output-imgs", "R2", "-objects", "--min-area", "2"], capsys)
    r1, r2 = _files("R1"), _files("R2")
    assert set(r2) - set(r1) == {"objects.json"} | {f"{s}-objects-mask.png" for s in stems}
    assert all(r2[f] == r1[f] for f in r1) and len(r1) == 2 * len(stems)
    report = json.loads(r2["objects.json"])
    rows = objects.table_rows(table, kept)
    assert report == {"source": "thresholded-mask", "threshold": thr, "connectivity": 8, "min_area": 2, "max_objects": 256,
                      "frames": {s: {"found": int(found[i]), "kept": int(kept[i]), "objects": rows[i]} for i, s in enumerate(order)}}
    for i, s in enumerate(order):
        png = np.array(Image.open(os.path.join("R2", f"{s}-objects-mask.png")))
        np.testing.assert_array_equal(png, np.repeat(kept_mask[i][:, :, None], 3, axis=2) * np.uint8(255))

    # -crf, -concatenated: the CRF mask is what is labelled; the strips are untouched
    common = ["-process", "-crf", "-concatenated", "--source-imgs", "S", "--binarymaskthreshold", repr(thr)]
    _, base = _run(common + ["--mask-output-imgs", "R3"], capsys)
    _, out = _run(common + ["--mask-output-imgs", "R4", "-objects", "--connectivity", "4"], capsys)
    r3, r4 = _files("R3"), _files("R4")
    assert set(r4) - set(r3) == {"objects.json"} | {f"{s}-objects-mask.png" for s in stems}
    assert all(r4[f] == r3[f] for f in r3) and set(r3) == {f"{s}_with_mask.png" for s in stems}
    crf_on = np.stack([np.array(Image.open(os.path.join("R4", f"{s}_with_mask.png")))[:, 192:256, 0] > 0 for s in order])
    labels, kept_mask, kept, found, table = objects_ref.label(crf_on, 4, 1, 256)
    report = json.loads(r4["objects.json"])
    rows = objects.table_rows(table, kept)
    assert report == {"source": "crf-mask", "threshold": None, "connectivity": 4, "min_area": 1, "max_objects": 256,
                      "frames": {s: {"found": int(found[i]), "kept": int(kept[i]), "objects": rows[i]} for i, s in enumerate(order)}}
    for i, s in enumerate(order):
        png = np.array(Image.open(os.path.join("R4", f"{s}-objects-mask.png")))
        np.testing.assert_array_equal(png, np.repeat(kept_mask[i][:, :, None], 3, axis=2) * np.uint8(255))
