"""CPU checks of the evaluation video (-test / --output-video, main.py:1027-1087): the layout plan, the ffmpeg command line, the output
path, the font order, the gating and the early refusals of Handler.eval, the C ABI entry, and what of the reference's G13 capture needs
no GPU (its recorded ffmpeg arguments, file name, bands and the RGB / ground-truth / constant tiles)."""
import ctypes
import json
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REPO)

import video_ref  # noqa: E402
from loop_inputs import synthetic_eval_set  # noqa: E402
from cgs_amd import _lib, build, cli, handler, video  # noqa: E402

TITLES = ["RGB\nimage", "ground\ntruth", "mask", "thresholded\nmask\nIoU=0.41", "mask\nCRF\nIoU=0.45", "saliency\nmap",
          "thresholded\nsaliency\nIoU=0.22", "salience\nCRF\nIoU=0.11"]
G, C, K = video.GREY, video.CODE, video.CONST


def _dejavu():
    import matplotlib
    return os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf")


# ---------------------------------------------------------------- layout plan
def test_layout_salience_five_columns():
    lay = video.plan(crf=False, salience=True)
    assert lay.row1 == (("X", G), ("Y", G), ("hardM", G), ("M", G), ("salhardM", G))
    assert lay.row2 == (("X", G), ("Y", C), ("hardM", C), (None, K), (None, K))
    assert list(lay.titles) == [TITLES[i] for i in (0, 1, 3, 2, 5)]
    assert (lay.width, lay.height, lay.h_top, lay.h_bottom, lay.short) == (960, 624, 120, 120, True)


def test_layout_salience_crf_eight_columns():
    lay = video.plan(crf=True, salience=True)
    assert [nm for nm, _ in lay.row1] == ["X", "Y", "crfM", "hardM", "M", "salcrfM", "salhardM", "salM"]
    assert all(mode == G for _, mode in lay.row1)
    assert lay.row2 == (("X", G), ("Y", C), ("crfM", C), ("hardM", C), (None, K), ("salcrfM", C), ("salhardM", C), (None, K))
    assert list(lay.titles) == [TITLES[i] for i in (0, 1, 4, 3, 2, 7, 6, 5)]
    assert (lay.width, lay.height, lay.h_top, lay.h_bottom, lay.short) == (1536, 564, 120, 60, False)


@pytest.mark.parametrize("crf", [False, True])
def test_layout_agrees_with_the_test_restatement(crf):
    lay, ref = video.plan(crf=crf, salience=True), video_ref.LAYOUTS[crf]
    assert [nm for nm, _ in lay.row1] == ref["row1"]
    want2 = [("X", G) if s == "X" else ((None, K) if s == "const" else (s[5:], C)) for s in ref["row2"]]
    assert list(lay.row2) == want2
    assert list(lay.titles) == [TITLES[i] for i in ref["titles"]]
    assert (lay.h_top, lay.h_bottom) == (ref["h_top"], ref["h_bottom"])


@pytest.mark.parametrize("crf", [False, True])
def test_layouts_without_salience_are_refused(crf):
    with pytest.raises(NotImplementedError, match=r"main\.py:1028-1055"):
        video.plan(crf=crf, salience=False)


# ---------------------------------------------------------------- encoder command line, output path, font
def _pairs(argv):
    return {(a, b) for a, b in zip(argv, argv[1:])}


def test_ffmpeg_argv_carries_the_reference_settings():
    argv = video.ffmpeg_argv("/x/ffmpeg", "v/iou=0.5.mp4", 960, 624)
    assert argv[0] == "/x/ffmpeg"
    i = argv.index("-i")
    inp, out = _pairs(argv[:i]), _pairs(argv[i:])
    assert {("-f", "rawvideo"), ("-pix_fmt", "rgb24"), ("-s", "960x624"), ("-r", "10")} <= inp
    assert argv[i + 1] == "pipe:"
    assert {("-pix_fmt", "yuv420p"), ("-vcodec", "libx264"), ("-r", "10")} <= out
    assert "v/iou=0.5.mp4" in argv[i:] and argv[-1] == "-y"


def test_output_path_with_and_without_output_video():
    assert video.output_path("v", 0.03) == "v/iou=0.03.mp4"
    assert video.output_path("out/dir", 0.41) == "out/dir/iou=0.41.mp4"
    assert video.output_path("", 0.5) == "iou=0.5.mp4"
    assert video.output_path("", 0.12345) == "iou=0.123.mp4"


def test_font_resolution_order(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _, where = video.resolve_font()
    assert where == _dejavu()                                   # no reference font here: matplotlib's DejaVuSans
    os.makedirs("isy_minerl/segm/etc")
    shutil.copy(_dejavu(), video.REFERENCE_FONT)
    font, where = video.resolve_font()
    assert where == video.REFERENCE_FONT and font.size == 30
    os.remove(video.REFERENCE_FONT)
    monkeypatch.setitem(sys.modules, "matplotlib", None)        # matplotlib not importable: PIL's own font
    font, where = video.resolve_font()
    assert where == "PIL default"


# ---------------------------------------------------------------- gating and early refusals in Handler.eval
@pytest.mark.parametrize("argv,want", [(["-eval"], False), (["-eval", "-crf"], False), (["-eval", "-salience"], False),
                                       (["-eval", "--output-video", "v"], True), (["-test"], True),
                                       (["-test", "-visbesteval", ""], True),               # -test forces it on (main.py:1543)
                                       (["-eval", "-salience", "--output-video", "v", "-visbesteval", ""], False)])
def test_gating(argv, want):
    assert video.wanted(cli.parse_args(argv)) is want


class _SweepStarted(Exception):
    pass


def _bare_handler(argv, monkeypatch):
    """A Handler without GPU set-up whose sweep raises: anything raised before it is raised before any GPU work."""
    H = handler.Handler.__new__(handler.Handler)
    H.args, H.rank, H.ious = cli.parse_args(argv), 0, (0, 0)

    def sweep(*a, **k):
        raise _SweepStarted()
    monkeypatch.setattr(H, "_sweep_masks", sweep)
    monkeypatch.setattr(np, "load", lambda *a, **k: np.zeros((200, 64, 64, 3), np.uint8))
    return H


def test_missing_ffmpeg_raises_before_the_sweep(tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path))
    H = _bare_handler(["-test", "--model", "m"], monkeypatch)
    with pytest.raises(FileNotFoundError, match="ffmpeg"):
        H.eval()


def test_unsupported_layout_raises_before_the_sweep(tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path))
    for argv in (["-eval", "--output-video", "v"], ["-eval", "-crf", "--output-video", "v"]):
        H = _bare_handler(argv + ["--model", "m"], monkeypatch)
        with pytest.raises(NotImplementedError, match=r"main\.py:1028-1055"):
            H.eval()


def test_plain_eval_goes_to_the_sweep_without_ffmpeg(tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path))
    for argv in (["-eval"], ["-eval", "-crf"], ["-eval", "-salience"], ["-eval", "-salience", "--output-video", "v", "-visbesteval", ""]):
        H = _bare_handler(argv + ["--model", "m"], monkeypatch)
        with pytest.raises(_SweepStarted):
            H.eval()


# ---------------------------------------------------------------- C ABI
def test_video_entry_is_declared_built_and_validates_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert "int cgs_video_compose(" in text and "main.py:1027-1087" in text
    assert "video.hip" in build.SOURCES
    assert ctypes.sizeof(_lib.VideoCell) == 32
    for name, value in (("CGS_VIDEO_RGB8", 0), ("CGS_VIDEO_MASK8", 1), ("CGS_VIDEO_F32", 2), ("CGS_VIDEO_F64", 3),
                        ("CGS_VIDEO_GREY", 0), ("CGS_VIDEO_CODE", 1), ("CGS_VIDEO_CONST", 2), ("CGS_VIDEO_MAX_CELLS", 16),
                        ("CGS_VIDEO_NONTEMPORAL", 1)):
        assert f"{name} = {value}" in text
        assert getattr(_lib, name[4:]) == value
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    cells = (_lib.VideoCell * 2)(_lib.VideoCell(None, None, 0.1, 0, _lib.VIDEO_CONST), _lib.VideoCell(None, None, 0.0, 1, _lib.VIDEO_GREY))
    buf = ctypes.create_string_buffer(64)
    out = (ctypes.addressof(buf) + 15) // 16 * 16
    # argument errors come back before anything reaches the GPU
    assert lib.cgs_video_compose(cells, 1, 1, 0, 0, None, 0, None, 0, 0, out, None) == _lib.ERR_BADARG            # n = 0
    assert lib.cgs_video_compose(cells, 1, 1, 0, 1, None, 0, None, 0, 2, out, None) == _lib.ERR_BADARG            # unknown flag
    assert lib.cgs_video_compose(cells, 1, 1, 0, 1, None, 0, None, 0, 0, out + 1, None) == _lib.ERR_BADARG        # unaligned out
    assert lib.cgs_video_compose(cells, 1, 2, 0, 1, None, 0, None, 0, 0, out, None) == _lib.ERR_BADARG            # GREY without src
    assert lib.cgs_video_compose(cells, 4, 5, 0, 1, None, 0, None, 0, 0, out, None) == _lib.ERR_BADARG            # > 16 cells
    code_rgb = (_lib.VideoCell * 1)(_lib.VideoCell(out, out, 0.0, _lib.VIDEO_RGB8, _lib.VIDEO_CODE))
    assert lib.cgs_video_compose(code_rgb, 1, 1, 0, 1, None, 0, None, 0, 0, out, None) == _lib.ERR_BADARG         # CODE needs MASK8


# ---------------------------------------------------------------- G13 (the reference's -test video), the parts without a GPU
def _g13(golden):
    return golden("g13_test_video.npz")


def test_g13_recorded_encoder_arguments_match(golden):
    g = _g13(golden)
    inp, out = json.loads(str(g["input_kwargs_json"])), json.loads(str(g["output_kwargs_json"]))
    assert json.loads(str(g["input_args_json"])) == ["pipe:"]
    n, h, w, _ = g["frames"].shape
    argv = video.ffmpeg_argv("ffmpeg", str(g["file_name"]), w, h)
    i = argv.index("-i")
    assert {("-f", inp["format"]), ("-pix_fmt", inp["pix_fmt"]), ("-s", inp["s"]), ("-r", str(inp["r"]))} <= _pairs(argv[:i])
    assert {("-pix_fmt", out["pix_fmt"]), ("-vcodec", out["vcodec"]), ("-r", str(out["r"]))} <= _pairs(argv[i:])
    assert "overwrite_output" in json.loads(str(g["calls_json"])) and argv[-1] == "-y"
    assert (w, h) == (video.plan(False, True).width, video.plan(False, True).height)
    assert int(g["stream_bytes"]) == n * h * w * 3
    assert str(g["file_name"]) == video.output_path("v", float(g["ious"][0]))


def test_g13_rgb_truth_and_constant_tiles(golden):
    g = _g13(golden)
    X, Yrgb = synthetic_eval_set(int(g["n_set"]), int(g["data_seed"]))
    pick = slice(100, 5000, 2)
    X, Y = X[pick], Yrgb[pick].all(axis=-1)
    ref = g["frames"]
    assert len(ref) == len(X) == 8
    lay = video.plan(False, True)
    zeros = np.zeros((len(X), 64, 64), bool)
    src = {"X": X, "Y": Y, "M": zeros.astype(np.float32), "hardM": zeros, "salhardM": zeros}
    want = video_ref.middle(src, crf=False)
    got = ref[:, lay.h_top:lay.h_top + 2 * video.CELL]
    for row in (0, 1):
        for col in (0, 1):                      # RGB frame, ground truth (grey / colour-coded against itself)
            sl = (slice(None), slice(row * 192, row * 192 + 192), slice(col * 192, col * 192 + 192))
            np.testing.assert_array_equal(got[sl], want[sl], err_msg=f"row {row} col {col}")
    np.testing.assert_array_equal(got[:, 192:, 3 * 192:], 25)              # the two constant 0.1 tiles


def test_g13_bands_match_when_fonts_render_alike(golden):
    import PIL
    from PIL import features
    g = _g13(golden)
    versions = (PIL.__version__, features.version("freetype2"))
    if versions != (str(g["pil_version"]), str(g["freetype_version"])):
        pytest.skip(f"bands not compared: PIL / FreeType {versions} here, {(str(g['pil_version']), str(g['freetype_version']))} "
                    "in the capture")
    lay = video.plan(False, True)
    from PIL import ImageFont
    top, bottom = video.render_bands(lay, ImageFont.truetype(_dejavu(), video.FONT_SIZE))
    ref = g["frames"]
    for f in ref:
        np.testing.assert_array_equal(f[:lay.h_top], top)
        np.testing.assert_array_equal(f[lay.height - lay.h_bottom:], bottom)
