"""CPU checks of --object-value: the by-hand cases of the rule of cgs_objects_ablate / cgs_objects_select and of objects.value's chunking
on tests/objects_value_ref.py (the checker of the GPU tests), the host helpers, the CLI's refusals (all before any GPU work), and the
binding."""
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

import objects_value_ref as ref  # noqa: E402
from cgs_amd import _lib, build, cli, objects  # noqa: E402


def _frames(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 64, 64, 3), dtype=np.uint8)


def _changed(images, frame):
    return (images != frame[None]).any(axis=-1)


# ---------------------------------------------------------------------------------------------------------------- the reference, by hand
def test_ref_corner_cell_grow_4():
    frames = np.full((1, 64, 64, 3), 7, dtype=np.uint8)
    labels = np.zeros((1, 64, 64), dtype=np.int32)
    labels[0, 63, 0] = 1                                       # one cell in the bottom-left corner
    images, row_frame, row_label, offsets = ref.ablate(frames, labels, [1], (200, 100, 50), 4)
    assert images.shape == (1, 64, 64, 3) and row_frame.tolist() == [0] and row_label.tolist() == [1] and offsets.tolist() == [0, 1]
    want = np.zeros((64, 64), dtype=bool)
    want[59:64, 0:5] = True                                    # the 9 x 9 square clipped by two borders: 5 x 5
    np.testing.assert_array_equal(_changed(images, frames[0])[0], want)
    assert (images[0][want] == (200, 100, 50)).all() and (images[0][~want] == 7).all()


def test_ref_two_objects_one_cell_apart_grow_1():
    frames = _frames(1, 1)
    labels = np.zeros((1, 64, 64), dtype=np.int32)
    labels[0, 10, 10], labels[0, 10, 12] = 1, 2                # one empty cell between them
    fill = np.full((64, 64, 3), 0, dtype=np.uint8)
    frames[frames == 0] = 1                                    # so that every replaced byte shows
    images, _, row_label, offsets = ref.ablate(frames, labels, [2], fill, 1)
    assert row_label.tolist() == [1, 2] and offsets.tolist() == [0, 2]
    ch = _changed(images, frames[0])
    a, b = np.zeros((64, 64), dtype=bool), np.zeros((64, 64), dtype=bool)
    a[9:12, 9:12], b[9:12, 11:14] = True, True
    np.testing.assert_array_equal(ch[0], a)
    np.testing.assert_array_equal(ch[1], b)
    assert not ch[0][10, 12] and not ch[1][10, 10]             # at grow 1 neither reaches the other's cell ...
    ch2 = _changed(ref.ablate(frames, labels, [2], fill, 2)[0], frames[0])
    assert ch2[0][10, 12] and ch2[1][10, 10]                   # ... at grow 2 the other object's cell is replaced too
    # grow 0: only the object's own cell
    ch0 = _changed(ref.ablate(frames, labels, [2], fill, 0)[0], frames[0])
    assert ch0[0].sum() == 1 and ch0[0][10, 10] and ch0[1].sum() == 1 and ch0[1][10, 12]


def test_ref_mean_rounds_half_up_and_falls_back_to_all_cells():
    frame = np.zeros((64, 64, 3), dtype=np.uint8)
    labels = np.ones((64, 64), dtype=np.int32)
    labels[0, 0:2] = 0                                         # two background cells
    frame[0, 0], frame[0, 1] = (10, 0, 255), (11, 1, 255)      # means 10.5, 0.5, 255
    assert ref.mean_fill(frame, labels) == (11, 1, 255)
    frame[0, 1] = (12, 0, 254)                                 # 11 exactly, 0, 254.5
    assert ref.mean_fill(frame, labels) == (11, 0, 255)
    full = np.ones((64, 64), dtype=np.int32)                   # a full-frame object: no cell of label 0, all 4096 count
    frame[:] = 0
    frame[0, :, 0] = 32                                        # S = 64 * 32 = 2048 over N = 4096: 0.5 exactly
    frame[1, :, 1] = 31                                        # 1984 / 4096 < 0.5
    assert ref.mean_fill(frame, full) == (1, 0, 0)
    images, _, _, _ = ref.ablate(frame[None], full[None], [1], "mean", 0)
    assert (images[0] == (1, 0, 0)).all()                      # the whole frame is the object
    above = np.full((64, 64), 65, dtype=np.int32)              # a label above K is not background either
    assert ref.mean_fill(frame, above) == (1, 0, 0)


def test_ref_labels_above_kept_or_K_get_no_row():
    frames = _frames(2, 2)
    labels = np.zeros((2, 64, 64), dtype=np.int32)
    labels[0, 0, 0], labels[0, 5, 5], labels[1, 3, 3] = 65, 1, 2
    images, row_frame, row_label, offsets = ref.ablate(frames, labels, [65, 1], (0, 0, 0), 0)
    assert offsets.tolist() == [0, 64, 65] and row_frame.tolist() == [0] * 64 + [1] and row_label.tolist() == list(range(1, 65)) + [1]
    assert (images[:, 0, 0][:64] == frames[0, 0, 0]).all()     # the cell of label 65 is never replaced
    np.testing.assert_array_equal(images[64], frames[1])       # frame 1 has kept 1 and no cell of label 1: its row is the frame


def test_ref_chunks():
    rows = [64, 0, 1, 63, 2]
    assert ref.chunks(rows, 64) == [(0, 2, 64), (2, 4, 64), (4, 5, 2)]
    assert ref.chunks(rows, 65) == [(0, 3, 65), (3, 5, 65)]
    assert ref.chunks([0, 0, 0], 64) == [] and ref.chunks([0, 3, 0], 64) == [(0, 3, 3)]
    for chunk_rows in (64, 65, 100, 2048):
        assert objects.value_chunks(rows, chunk_rows) == ref.chunks(rows, chunk_rows)
    assert objects.value_chunks([0, 0], 64) == []
    with pytest.raises(ValueError, match="chunk_rows"):
        objects.value_chunks([65], 64)


def test_ref_select_and_selected():
    labels = np.zeros((2, 4, 4), dtype=np.int32)
    labels[0, 0] = [1, 2, 3, 70]
    labels[1, 1] = [1, 1, 2, 0]
    table = np.arange(2 * 64 * 8, dtype=np.int32).reshape(2, 64, 8)
    keep = np.zeros((2, 64), dtype=bool)
    keep[0, [0, 2, 5]] = True                                  # labels 1, 3, 6 become 1, 2, 3; label 70 is above K and goes
    keep[1, [1, 2]] = True                                     # label 3 is above kept[1] = 2: no such object
    out, tab, kept, mask, unscored = ref.select(labels, table, [70, 2], keep)
    assert out[0, 0].tolist() == [1, 0, 2, 0] and out[1, 1].tolist() == [0, 0, 1, 0]
    assert kept.tolist() == [3, 1] and unscored.tolist() == [6, 0]
    np.testing.assert_array_equal(tab[0, :3], table[0, [0, 2, 5]])
    assert not tab[0, 3:].any() and not tab[1, 1:].any()
    np.testing.assert_array_equal(tab[1, 0], table[1, 1])
    np.testing.assert_array_equal(mask, (out != 0).astype(np.uint8))
    drop = np.zeros((1, 64), dtype=np.float32)
    drop[0, :4] = [0.25, np.nan, np.float32(0.1), -1.0]
    got = ref.selected(drop, [3], 0.1)                          # 0.1 as float32 on both sides: equal, selected
    assert got[0, :4].tolist() == [True, False, True, False] and not got[0, 3:].any()


# ---------------------------------------------------------------------------------------------------------------- host helpers
def test_parse_helpers():
    assert objects.parse_object_value_fill("low") == "low" and objects.parse_object_value_fill(" mean ") == "mean"
    assert objects.parse_object_value_fill("0,128, 255") == (0, 128, 255)
    for bad in ("", "high", "1,2", "1,2,3,4", "1,2,256", "-1,0,0", "1.5,0,0", "a,b,c"):
        with pytest.raises(ValueError, match="--object-value-fill"):
            objects.parse_object_value_fill(bad)
    assert [objects.parse_object_value_grow(s) for s in ("0", "4", " 2 ")] == [0, 4, 2]
    for bad in ("5", "-1", "1.5", "x", ""):
        with pytest.raises(ValueError, match="--object-value-grow"):
            objects.parse_object_value_grow(bad)
    assert objects.parse_min_value_drop("0.25") == 0.25 and objects.parse_min_value_drop("-1e-3") == -1e-3
    for bad in ("nan", "inf", "-inf", "x", ""):
        with pytest.raises(ValueError, match="--min-value-drop"):
            objects.parse_min_value_drop(bad)


def test_value_keep_and_report_on_the_host():
    drop = torch.zeros((2, 64), dtype=torch.float32)
    drop[0, :3] = torch.tensor([0.5, float("nan"), -0.25])
    drop[1, 0] = 0.1
    kept = torch.tensor([3, 70], dtype=torch.int32)
    keep = objects.value_keep(drop, kept, 0.1)
    np.testing.assert_array_equal(keep.numpy(), ref.selected(drop.numpy(), kept.numpy(), 0.1))
    assert keep[0, :3].tolist() == [True, False, False] and keep[1, 0].item() and int(keep[1].sum()) == 1
    drop[0, 1] = 0.0
    val = objects.Values(torch.tensor([1.0, 3.0]), drop, 1, 67, [(0, 2, 67)])
    rep = objects.value_report(val, kept, "low", 0, stems=["a", "b"])
    assert rep["fill"] == "low" and rep["fill_frame"] == "b" and rep["grow"] == 0 and rep["min_value_drop"] is None
    assert rep["rows"] == 67 and rep["unscored"] == 6 and rep["base_mean"] == 2.0
    assert rep["drop"]["negative"] == 1 and rep["drop"]["max"] == 0.5 and rep["drop"]["min"] == -0.25
    assert rep["drop"]["mean"] == pytest.approx((0.5 - 0.25 + np.float32(0.1)) / 67)
    rep = objects.value_report(val._replace(fill_frame=None), kept, (1, 2, 3), 2, 0.1, keep=keep)
    assert rep["fill"] == [1, 2, 3] and rep["fill_frame"] is None and rep["min_value_drop"] == 0.1 and rep["selected_objects"] == 2


def test_no_gpu_is_an_error_not_a_fallback():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    frames, labels, kept = torch.zeros((1, 64, 64, 3), dtype=torch.uint8), torch.zeros((1, 64, 64), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.CgsError, match="cgs_objects_ablate"):
        objects.ablate(frames, labels, kept)
    with pytest.raises(_lib.CgsError, match="cgs_objects_ablate"):
        objects.value(lambda X: X.sum(dim=(1, 2, 3)).float(), frames, labels, kept)
    res = objects.Objects(labels, None, kept, kept, torch.zeros((1, 64, 8), dtype=torch.int32))
    with pytest.raises(_lib.CgsError, match="cgs_objects_select"):
        objects.select(res, torch.zeros((1, 64), dtype=torch.bool))


def test_argument_checks_come_first():
    frames, labels, kept = torch.zeros((1, 64, 64, 3), dtype=torch.uint8), torch.zeros((1, 64, 64), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    infer = lambda X: X.sum(dim=(1, 2, 3)).float()
    for kw in (dict(fill="low"), dict(fill=(1, 2)), dict(fill=(1, 2, 256)), dict(fill=torch.zeros((64, 64, 3))), dict(grow=5), dict(grow=-1),
               dict(max_objects=65), dict(max_objects=0), dict(frames_range=(1, 0)), dict(frames_range=(0, 2))):
        with pytest.raises(ValueError):
            objects.ablate(frames, labels, kept, **kw)
    with pytest.raises(ValueError, match="64"):
        objects.ablate(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), torch.zeros((1, 32, 32), dtype=torch.int32), kept)
    with pytest.raises(ValueError, match="torch.int32"):
        objects.ablate(frames, labels.long(), kept)
    with pytest.raises(ValueError, match="chunk_rows"):
        objects.value(infer, frames, labels, kept, chunk_rows=63)
    with pytest.raises(ValueError, match="callable"):
        objects.value(None, frames, labels, kept)
    with pytest.raises(ValueError, match="fill"):
        objects.value(infer, frames, labels, kept, fill="median")
    res = objects.Objects(labels, None, kept, kept, torch.zeros((1, 64, 8), dtype=torch.int32))
    for keep in (torch.zeros((1, 65), dtype=torch.bool), torch.zeros((2, 64), dtype=torch.bool), torch.zeros((1, 64)), None):
        with pytest.raises(ValueError):
            objects.select(res, keep)
    with pytest.raises(ValueError):
        objects.select(res._replace(table=torch.zeros((1, 32, 8), dtype=torch.int32)), torch.zeros((1, 64), dtype=torch.bool))
    with pytest.raises(ValueError):
        objects.select(res._replace(labels=None), torch.zeros((1, 64), dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------- the command line
PROCESS = ["--model", "m", "-process", "--source-imgs", "S", "-objects"]


def test_cli_accepts_and_fills_in_defaults():
    a = cli.parse_args(PROCESS)
    assert a.object_value is False and a.object_value_fill is None and a.object_value_grow is None and a.min_value_drop is None
    a = cli.parse_args(PROCESS + ["--object-value"])
    assert a.object_value and a.object_value_fill == "low" and a.object_value_grow == 0 and a.min_value_drop is None
    a = cli.parse_args(PROCESS + ["--object-value", "--object-value-fill", "3,4,5", "--object-value-grow", "4", "--min-value-drop", "-0.5",
                                  "--track-iou", "0.5"])
    assert a.object_value_fill == (3, 4, 5) and a.object_value_grow == 4 and a.min_value_drop == -0.5
    a = cli.parse_args(["--model", "m", "-eval", "-objects", "--object-value", "--object-value-fill", "mean", "--match-iou", "0.5"])
    assert a.object_value_fill == "mean"


@pytest.mark.parametrize("argv, match", [
    (["--model", "m", "-process", "--object-value"], "-objects"),
    (["--model", "m", "-eval", "--object-value", "--min-value-drop", "0.1"], "-objects"),
    (PROCESS + ["--object-value-fill", "mean"], "--object-value"),
    (PROCESS + ["--object-value-grow", "1"], "--object-value"),
    (PROCESS + ["--min-value-drop", "0.1"], "--object-value"),
    (["--model", "m", "--min-value-drop", "0.1"], "--object-value"),
    (["--model", "m", "-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "--object-value"], "--source-video"),
    (["--model", "m", "-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4", "-objects", "--object-value"], "--source-video"),
    (PROCESS + ["--object-value", "-noevalmode"], "-noevalmode"),
    (["--model", "m", "-eval", "-objects", "--object-value", "-noevalmode"], "-noevalmode"),
    (PROCESS + ["--object-value", "--object-value-fill", "median"], "--object-value-fill"),
    (PROCESS + ["--object-value", "--object-value-fill", "1,2,300"], "--object-value-fill"),
    (PROCESS + ["--object-value", "--object-value-grow", "5"], "--object-value-grow"),
    (PROCESS + ["--object-value", "--object-value-grow", "one"], "--object-value-grow"),
    (PROCESS + ["--object-value", "--min-value-drop", "nan"], "--min-value-drop"),
    (PROCESS + ["--object-value", "--min-value-drop", "inf"], "--min-value-drop"),
    (PROCESS + ["--object-value", "--min-value-drop", "big"], "--min-value-drop"),
    (["--model", "m", "-objects", "--object-value"], "-process or -eval"),
])
def test_cli_refusals(argv, match):
    with pytest.raises(ValueError, match=re.escape(match)):
        cli.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_binding_and_header():
    assert "objects_value.hip" in build.SOURCES
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    for name in ("cgs_objects_ablate(", "cgs_objects_select(", "CGS_OBJ_VALUE_MAX_OBJECTS = 64", "CGS_OBJ_VALUE_MAX_GROW = 4"):
        assert name in text
    assert len(_lib.SIGNATURES["cgs_objects_ablate"][1]) == 17 and len(_lib.SIGNATURES["cgs_objects_select"][1]) == 14
    assert (objects.VALUE_MAX_OBJECTS, objects.VALUE_MAX_GROW, objects.VALUE_SIDE) == (64, 4, 64)
    assert (objects.VALUE_FILL, objects.VALUE_GROW) == ("low", 0)
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    # the refusals of the two entries come before any launch: no GPU is needed to see them
    assert lib.cgs_objects_ablate(None, None, None, 1, 0, 1, 64, 0, 0, 0, None, 0, 1, None, None, None, None) == _lib.ERR_BADARG
    assert lib.cgs_objects_select(None, None, None, None, 1, 64, 64, 64, None, None, None, None, None, None) == _lib.ERR_BADARG
    buf = np.zeros(64, dtype=np.int64).ctypes.data                               # any aligned non-NULL address: nothing is launched
    bad = lambda **kw: lib.cgs_objects_ablate(*[{**dict(frames=buf, labels=buf, offsets=buf, n=2, f0=0, f1=2, K=64, grow=0, mode=0, rgb=0,
                                                         fill=None, stride=0, rows=1, out=buf, rf=buf, rl=buf, stream=None), **kw}[k]
                                                for k in ("frames", "labels", "offsets", "n", "f0", "f1", "K", "grow", "mode", "rgb", "fill",
                                                          "stride", "rows", "out", "rf", "rl", "stream")])
    for kw in (dict(f1=0), dict(f1=3), dict(f0=-1), dict(rows=0), dict(K=0), dict(grow=-1), dict(mode=3), dict(mode=1), dict(fill=buf),
               dict(rgb=1 << 24), dict(stride=16), dict(out=buf + 4), dict(frames=buf + 8), dict(labels=buf + 2)):
        assert bad(**kw) == _lib.ERR_BADARG, kw
    for kw in (dict(K=65), dict(grow=5)):
        assert bad(**kw) == _lib.ERR_UNSUPPORTED, kw
    sel = lambda **kw: lib.cgs_objects_select(*[{**dict(labels=buf, table=buf, kept=buf, keep=buf, n=1, h=64, w=64, K=64, ol=buf, ot=buf,
                                                        ok=buf, mask=buf, un=buf, stream=None), **kw}[k]
                                                for k in ("labels", "table", "kept", "keep", "n", "h", "w", "K", "ol", "ot", "ok", "mask", "un",
                                                          "stream")])
    for kw in (dict(n=0), dict(h=0), dict(K=0), dict(keep=None), dict(table=buf + 2)):
        assert sel(**kw) == _lib.ERR_BADARG, kw
    for kw in (dict(h=65), dict(w=65), dict(K=65)):
        assert sel(**kw) == _lib.ERR_UNSUPPORTED, kw
