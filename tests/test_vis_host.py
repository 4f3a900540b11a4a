"""CPU checks of the -viscritic / -vismasker videos (Handler.visualize, main.py:702-884): the numpy + PIL restatement tests/vis_ref.py
against the reference's own streams (G14, tests/golden/make_golden_vis.py), PIL's blend formula, the plot rows, the label atlas, the
sortings, the C ABI entry and the command line."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REPO)

import vis_ref  # noqa: E402
from loop_inputs import synthetic_frames  # noqa: E402
from cgs_amd import _lib, build, cli, handler, video, vis  # noqa: E402


def g14_inputs(g):
    """(X of the test split, N) of the capture, re-generated from its seed."""
    n = int(g["n"])
    X, Y, _ = synthetic_frames(int(g["datasize"]) + n, int(g["data_seed"]))
    np.testing.assert_array_equal(g["values"][0], Y[1, -n:])
    return X[-n:], n


def same_text_rendering(g):
    import PIL
    from PIL import features
    here = (PIL.__version__, features.version("freetype2"), bool(features.check("raqm")))
    there = (str(g["pil_version"]), str(g["freetype_version"]), bool(g["raqm"]))
    if here != there:
        print(f"label rectangles blanked on both sides: PIL / FreeType / raqm {here} here, {there} in the capture")
    return here == there


# ---------------------------------------------------------------- the restatement against the reference's streams
def test_restatement_reproduces_the_reference_streams(golden):
    g = golden("g14_vis.npz")
    X, n = g14_inputs(g)
    exact = same_text_rendering(g)
    view = (lambda a: a) if exact else vis_ref.blank_labels
    for k, sorting in enumerate((None, g["sorting_pred"], g["sorting_gt"])):
        got = vis_ref.frames(X, g["masks"], g["values"], sorting)
        assert got.shape == (n, 768, 256, 3)
        np.testing.assert_array_equal(view(got), view(g["vismasker_frames"][k]), err_msg=f"-vismasker video {k}")
        crit = vis_ref.frames(X, None, g["values"], sorting)
        assert crit.shape == (n, 512, 256, 3)
        if exact:
            assert [hashlib.sha256(f.tobytes()).hexdigest() for f in crit] == [str(h) for h in g["viscritic_sha256"][k]]
        else:               # (hashes cannot be blanked) the -viscritic frame is the -vismasker frame without its second tile; what
            # is left of that frame's index label (rows 512-514) lands inside the -viscritic label rectangle (rows 243-258)
            ref = np.concatenate((g["vismasker_frames"][k][:, :256], g["vismasker_frames"][k][:, 512:]), axis=1)
            np.testing.assert_array_equal(vis_ref.blank_labels(crit), vis_ref.blank_labels(ref), err_msg=f"-viscritic video {k}")


def test_g14_recorded_encoder_arguments_and_names(golden):
    g = golden("g14_vis.npz")
    for key, R in (("vismasker_ffmpeg_json", 2), ("viscritic_ffmpeg_json", 1)):
        recs = json.loads(str(g[key]))
        p = vis.plan(R == 2)
        assert (p.R, p.V, p.width, p.height) == (R, 2, 256, 4 * (64 * R + 64))
        assert [r["file"] for r in recs] == [f"m/curves{s}.mp4" for s, _ in vis.sortings(g["values"], 1)]
        for r in recs:
            argv = video.ffmpeg_argv("ffmpeg", r["file"], p.width, p.height, framerate=vis.FRAMERATE)
            i = argv.index("-i")
            pairs = lambda a: {(x, y) for x, y in zip(a, a[1:])}
            inp, out = r["input"], r["output"]
            assert r["input_args"] == ["pipe:"] and argv[i + 1] == "pipe:"
            assert {("-f", inp["format"]), ("-pix_fmt", inp["pix_fmt"]), ("-s", inp["s"]), ("-r", str(inp["r"]))} <= pairs(argv[:i])
            assert {("-pix_fmt", out["pix_fmt"]), ("-vcodec", out["vcodec"]), ("-r", str(out["r"]))} <= pairs(argv[i:])
            assert inp["r"] == out["r"] == 4 and "overwrite_output" in r["calls"] and argv[-1] == "-y"
    args = cli.parse_args(json.loads(str(g["argv_vismasker_json"])))
    tags = handler.checkpoint_names(args)
    assert [str(s) for s in g["checkpoint_names"]] == [f"m/saves/critic-{tags[0]}.pt", f"m/saves/masker-{tags[1]}.pt"]


# ---------------------------------------------------------------- PIL's blend
def test_blend_formula_matches_pil_for_every_dst_and_alpha():
    from PIL import Image, ImageDraw
    dst, alpha = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    want = vis_ref.blend(dst, alpha)
    # every (dst, alpha) pair through the call ImageDraw.text ends in: draw_bitmap = the ink pasted through an "L" mask
    img = Image.fromarray(np.repeat(dst[:, :, None], 3, axis=2).copy())
    ImageDraw.Draw(img).bitmap((0, 0), Image.fromarray(alpha), fill=(255, 255, 255))
    got = np.array(img)
    for c in range(3):
        np.testing.assert_array_equal(got[:, :, c], want)
    assert want[0].tolist() == list(range(256)) and (want[:, 0] == np.arange(256)).all() and (want[:, 255] == 255).all()


def test_blend_formula_matches_drawn_text_over_random_backgrounds():
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(5)
    seen = set()
    for text in ("0.467", "12345", "-0.02", "1e-05", "9876"):
        cell = vis.render_label(text)
        seen |= set(np.unique(cell).tolist())
        for x, y in ((1, 1), (1, 16), (230, 499)):
            bg = rs.randint(0, 256, (768, 256, 3)).astype(np.uint8)
            img = Image.fromarray(bg.copy())
            ImageDraw.Draw(img).text((x, y), text, fill=(255, 255, 255))
            w = min(vis.CELL_W, 256 - x)                                  # clipped at the frame edge, as PIL clips
            want = bg.copy()
            want[y:y + vis.CELL_H, x:x + w] = vis_ref.blend(bg[y:y + vis.CELL_H, x:x + w], cell[:, :w, None])
            np.testing.assert_array_equal(np.array(img), want, err_msg=f"{text!r} at {(x, y)}")
    assert 0 in seen and len(seen) > 2


# ---------------------------------------------------------------- plot rows, labels, sortings
def test_plot_rows_match_the_restatement():
    rs = np.random.RandomState(0)
    for values in (rs.rand(2, 150), rs.randn(2, 37) * 100, np.stack((np.zeros(9), np.full(9, 0.4673))), np.array([[3.0], [-1.0]]),
                   np.stack((np.linspace(0, 1, 33), np.linspace(-5, 5, 33)))):
        got = vis.plot_rows(values)
        assert got.dtype == np.uint8 and got.shape == values.shape
        for v in range(2):
            np.testing.assert_array_equal(got[v], vis_ref.plot_rows(values[v]))
    const = vis.plot_rows(np.full((2, 12), 0.25))                        # max == 0 after the shift: every row is 31
    assert (const == 31).all()
    assert vis.plot_rows(np.array([[0.0, 1.0], [0.0, 1.0]])).tolist() == [[31, 0], [31, 0]]      # floor(32 / 1.01) = 31


def test_labels_round_trip():
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(1)
    n = 40
    values = np.stack((np.round(rs.rand(n), 2), np.full(n, 0.46731)))
    atlas, ids, strings = vis.labels(values, n)
    assert atlas.dtype == np.uint8 and atlas.shape == (len(strings), vis.CELL_H, vis.CELL_W)
    assert ids.dtype == np.int32 and ids.shape == (n, 3) and ids.min() == 0 and ids.max() == len(strings) - 1
    assert len(set(strings)) == len(strings)                             # one cell per DISTINCT string
    assert len(set(ids[:, 2].tolist())) == 1                             # a constant prediction: one cell for all frames
    for p in range(n):
        want = vis_ref.label_strings(values, p)
        assert [strings[i] for i in ids[p]] == want == vis.label_strings(values, n)[p]
    for s, cell in zip(strings, atlas):                                   # the cell is what PIL draws, white on black
        img = Image.new("RGB", (vis.CELL_W, vis.CELL_H))
        ImageDraw.Draw(img).text((0, 0), s, fill=(255, 255, 255))
        np.testing.assert_array_equal(np.array(img), np.repeat(cell[:, :, None], 3, axis=2))
        assert cell.any()
    assert vis.label_positions(768) == vis_ref.label_positions(768) == [(230, 499), (1, 1), (1, 16)]
    assert vis.label_positions(512) == vis_ref.label_positions(512)
    big = vis.labels(np.zeros((2, 3)), 3)[2]
    assert big == ["0", "0.0", "1", "2"]
    with pytest.raises(ValueError, match="atlas cell"):
        vis.render_label("0.123456789012345678")


def test_atlas_cells_reproduce_pil_frames_on_g14(golden):
    """The canvas of the restatement with the atlas cells blended in (what the kernel does) equals PIL drawing on it."""
    g = golden("g14_vis.npz")
    X, n = g14_inputs(g)
    atlas, ids, _ = vis.labels(g["values"], n)
    for sorting in (None, g["sorting_gt"]):
        perm = np.arange(n) if sorting is None else sorting
        got = vis_ref.canvas(X, g["masks"], g["values"], sorting)
        for j in range(n):
            for (x, y), cell in zip(vis.label_positions(768), atlas[ids[perm[j]]]):
                w = min(vis.CELL_W, 256 - x)
                got[j, y:y + vis.CELL_H, x:x + w] = vis_ref.blend(got[j, y:y + vis.CELL_H, x:x + w], cell[:, :w, None])
        np.testing.assert_array_equal(got, vis_ref.frames(X, g["masks"], g["values"], sorting))


@pytest.mark.parametrize("sortidx", [0, 1])
def test_sortings_are_the_reference_numpy_calls(sortidx):
    values = np.random.RandomState(7).rand(2, 300)
    got = vis.sortings(values, sortidx)
    assert got[0] == ("", None)
    assert got[1][0] == "-pred-sorted"
    np.testing.assert_array_equal(got[1][1], np.argsort(values[sortidx])[::-1])
    if sortidx:
        assert len(got) == 3 and got[2][0] == "-GT-sorted"
        np.testing.assert_array_equal(got[2][1], np.argsort(values[0])[::-1])
    else:
        assert len(got) == 2                                             # two videos, not three (main.py:882)


# ---------------------------------------------------------------- C ABI
def test_vis_entry_is_declared_built_and_validates_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert "int cgs_vis_compose(" in text and "main.py:818-874" in text
    assert "vis.hip" in build.SOURCES and "cgs_vis_compose" in _lib.SIGNATURES
    for name, value in (("CGS_VIS_VALUES", 2), ("CGS_VIS_CELL_W", 64), ("CGS_VIS_CELL_H", 16), ("CGS_VIS_NONTEMPORAL", 1),
                        ("CGS_VIS_INDEX_X", 230), ("CGS_VIS_VALUE_X", 1), ("CGS_VIS_VALUE_Y", 1), ("CGS_VIS_VALUE_DY", 15)):
        assert f"{name} = {value}" in text
        assert getattr(_lib, name[4:]) == value
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16              # a non-null, 16-byte aligned address: nothing below reaches the GPU
    call = lambda **kw: lib.cgs_vis_compose(*[{**dict(X=p, masks=p, perm=None, rows=p, ids=p, atlas=p, n_labels=1, N=10, R=2, j0=0,
                                                      n=1, flags=0, out=p, stream=None), **kw}[k]
                                              for k in ("X", "masks", "perm", "rows", "ids", "atlas", "n_labels", "N", "R", "j0", "n",
                                                        "flags", "out", "stream")])
    assert call(out=None) == _lib.ERR_BADARG                  # null out
    assert call(out=p + 4) == _lib.ERR_BADARG                 # unaligned out
    assert call(n=0) == _lib.ERR_BADARG                       # n < 1
    assert call(R=0) == _lib.ERR_BADARG and call(R=3) == _lib.ERR_BADARG
    assert call(masks=None) == _lib.ERR_BADARG                # R = 2 without masks
    assert call(j0=9, n=2) == _lib.ERR_BADARG                 # j0 + n > N
    assert call(j0=-1) == _lib.ERR_BADARG
    assert call(flags=2) == _lib.ERR_BADARG                   # unknown flag bit
    assert call(X=None) == _lib.ERR_BADARG and call(rows=None) == _lib.ERR_BADARG and call(ids=None) == _lib.ERR_BADARG
    assert call(atlas=None) == _lib.ERR_BADARG and call(n_labels=0) == _lib.ERR_BADARG


# ---------------------------------------------------------------- command line
@pytest.mark.parametrize("flag", ["-viscritic", "-vismasker"])
def test_cli_without_train_raises_value_error(flag):
    with pytest.raises(ValueError, match="-train"):
        cli.main(["--model", "m", flag])


def test_purevis_and_trainasvis_stay_refused(monkeypatch):
    with pytest.raises(NotImplementedError, match="--purevis"):
        cli.main(["-train", "--model", "m", "-viscritic", "--purevis", "0,1"])
    # --trainasvis: refused where it always was (after the Handler and load_data), with its message
    monkeypatch.setattr(handler.Handler, "__init__", lambda self, args: setattr(self, "args", args))
    monkeypatch.setattr(handler.Handler, "load_data", lambda self: None)
    with pytest.raises(NotImplementedError, match=r"--trainasvis \(dataset visualisation\) is outside this build's scope"):
        cli.main(["-train", "--model", "m", "-viscritic", "--trainasvis", "5"])


class _SweepStarted(Exception):
    pass


def _bare_handler(argv, monkeypatch):
    H = handler.Handler.__new__(handler.Handler)
    H.args, H.rank, H.path = cli.parse_args(argv), 0, "m/"
    H.XX, H.YY = np.zeros((3, 64, 64, 3), np.uint8), np.zeros((7, 3))

    def sweep(*a, **k):
        raise _SweepStarted()
    monkeypatch.setattr(H, "_sweep_masks", sweep)
    return H


def test_missing_ffmpeg_raises_before_the_sweep(tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path))
    H = _bare_handler(["-train", "-vismasker", "--model", "m"], monkeypatch)
    with pytest.raises(FileNotFoundError, match="ffmpeg"):
        H.visualize()
    exe = tmp_path / "ffmpeg"
    exe.write_text("#!/bin/sh\n")
    exe.chmod(0o755)
    with pytest.raises(_SweepStarted):
        H.visualize()


def test_visualize_without_the_test_split_raises(monkeypatch):
    H = _bare_handler(["-train", "-viscritic", "--model", "m"], monkeypatch)
    del H.XX
    with pytest.raises(ValueError, match="-train"):
        H.visualize()
