"""The evaluation video on the GPU (cgs_video_compose / cgs_amd.video / -test on the CLI) against the numpy restatement tests/video_ref.py
and against the reference's own -test video (G13, tests/golden/make_golden_video.py)."""
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REPO)

import video_ref  # noqa: E402
from loop_inputs import synthetic_eval_set  # noqa: E402
from cgs_amd import cli, video  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- kernel vs restatement
def _edge_values(rs, n, dtype):
    """[n,64,64] maps in [0, 1] that put many products 255 v on and next to integers: k / 255 exactly (in `dtype`), nextafter on both
    sides, 0, 1 and uniform values."""
    k = rs.randint(0, 256, (n, 64, 64))
    exact = (k / 255.0).astype(dtype)
    side = rs.randint(0, 3, (n, 64, 64))
    v = np.where(side == 1, np.nextafter(exact, dtype(0)), np.where(side == 2, np.nextafter(exact, dtype(1)), exact))
    v = np.where(rs.rand(n, 64, 64) < 0.2, rs.rand(n, 64, 64).astype(dtype), v)
    v[:, :2] = 0
    v[:, 2:4] = 1
    return np.clip(v, 0, 1).astype(dtype)


def _sources(n, seed=0):
    rs = np.random.RandomState(seed)
    src = {"X": rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8), "Y": rs.rand(n, 64, 64) < 0.5,
           "M": _edge_values(rs, n, np.float32), "salM": _edge_values(rs, n, np.float64)}
    src["salM"][:, 10:20] = np.minimum(rs.rand(n, 10, 64) * 3, 1.0)          # clipped at exactly 1.0 (grey 255) as main.py:994
    src["hardM"] = src["M"] > 0.5
    src["crfM"] = rs.rand(n, 64, 64) < 0.5
    src["salhardM"] = (src["salM"] > 0.5).astype(np.uint8)
    src["salcrfM"] = rs.rand(n, 64, 64) < 0.3
    return src


def _bands(lay):
    return video.render_bands(lay, video.resolve_font()[0])


@pytest.mark.parametrize("crf", [False, True])
@pytest.mark.parametrize("nontemporal", [False, True])
def test_compose_bit_exact_vs_restatement(crf, nontemporal):
    n = 7
    src = _sources(n, seed=3 + crf)
    for nm in ("hardM", "crfM", "salhardM", "salcrfM"):             # all four (y, m) cases occur in every coded column
        y, m = src["Y"].astype(bool), src[nm].astype(bool)
        assert (y & m).any() and (y & ~m).any() and (~y & m).any() and (~y & ~m).any()
    lay = video.plan(crf, True)
    comp = video.Composer(lay, src)
    top, bottom = comp.bands
    want = video_ref.frames(src, crf, top, bottom)
    assert want.shape == (n, lay.height, lay.width, 3)
    got = comp.compose(0, n, nontemporal=nontemporal).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    # one frame from the middle of the stack, and ragged chunks through the pinned double buffer (3 + 3 + 1)
    np.testing.assert_array_equal(comp.compose(5, 1, nontemporal=nontemporal).cpu().numpy()[0], want[5])
    sink = io.BytesIO()
    assert video.stream_frames(comp, sink, chunk=3) == want.nbytes
    np.testing.assert_array_equal(np.frombuffer(sink.getvalue(), np.uint8).reshape(want.shape), want)


def test_single_frame_video_and_argument_checks():
    src = {k: v[:1] for k, v in _sources(1, seed=9).items()}
    lay = video.plan(False, True)
    comp = video.Composer(lay, src)
    want = video_ref.frames(src, False, *comp.bands)
    sink = io.BytesIO()
    video.stream_frames(comp, sink)
    np.testing.assert_array_equal(np.frombuffer(sink.getvalue(), np.uint8).reshape(want.shape), want)
    with pytest.raises(ValueError):
        comp.compose(0, 2)                                       # past the end of the sources
    with pytest.raises(ValueError):
        video.Composer(lay, {k: v for k, v in src.items() if k != "M"})


# ---------------------------------------------------------------- the CLI, end to end
STUB = """#!{python}
import os, shutil, sys
out = {out!r}
n = len([f for f in os.listdir(out) if f.endswith(".argv")])
with open(os.path.join(out, f"{{n}}.argv"), "w") as fp:
    fp.write("\\n".join(sys.argv))
with open(os.path.join(out, f"{{n}}.stdin"), "wb") as fp:
    shutil.copyfileobj(sys.stdin.buffer, fp)
"""


def _stub_ffmpeg(root):
    """A test-written `ffmpeg` first on PATH: it saves its argv and everything on stdin under root/ffmpeg_calls/."""
    bindir, calls = os.path.join(root, "bin"), os.path.join(root, "ffmpeg_calls")
    os.makedirs(bindir)
    os.makedirs(calls)
    exe = os.path.join(bindir, "ffmpeg")
    with open(exe, "w") as fp:
        fp.write(STUB.format(python=sys.executable, out=calls))
    os.chmod(exe, 0o755)
    return bindir, calls


def _setup(root, golden, g1):
    pc, pm = g1
    cn = [str(s) for s in golden("g6_process.npz")["checkpoint_names"]]
    for c, state in zip(cn, (pc, pm)):
        os.makedirs(os.path.dirname(os.path.join(root, c)), exist_ok=True)
        torch.save(state, os.path.join(root, c))
    g = golden("g13_test_video.npz")
    X, Yrgb = synthetic_eval_set(int(g["n_set"]), int(g["data_seed"]))
    os.makedirs(os.path.join(root, "red-trees"))
    np.save(os.path.join(root, "red-trees", "X.npy"), X)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Yrgb)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory, golden, g1):
    """`main.py -test --model m --output-video v` once, in-process, with the stub ffmpeg; the arrays Handler.eval hands to the video."""
    root = str(tmp_path_factory.mktemp("video"))
    _setup(root, golden, g1)
    bindir, calls = _stub_ffmpeg(root)
    mp = pytest.MonkeyPatch()
    seen = []
    real = video.write_video

    def spy(path, layout, sources, *a, **k):
        seen.append((path, layout, {nm: np.array(v, copy=True) for nm, v in sources.items()}))
        return real(path, layout, sources, *a, **k)
    try:
        mp.chdir(root)
        mp.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
        mp.setattr(video, "write_video", spy)
        out = io.StringIO()
        mp.setattr(sys, "stdout", out)
        H = cli.main(["-test", "--model", "m", "--output-video", "v"])
    finally:
        mp.undo()
    printed = out.getvalue()
    sys.stdout.write(printed[-2000:])
    ious = [float(v) for v in printed.split("RESULTS [")[-1].split("]")[0].split(",")]
    assert len(seen) == 1 and sorted(os.listdir(calls)) == ["0.argv", "0.stdin"]
    with open(os.path.join(calls, "0.argv")) as fp:
        argv = fp.read().split("\n")
    with open(os.path.join(calls, "0.stdin"), "rb") as fp:
        stream = fp.read()
    return {"root": root, "H": H, "ious": ious, "seen": seen[0], "argv": argv, "stream": stream}


def test_cli_test_writes_the_video(cli_run):
    path, lay, src = cli_run["seen"]
    n = len(src["X"])
    assert n == 8 and (lay.width, lay.height) == (960, 624)
    assert len(cli_run["stream"]) == n * lay.height * lay.width * 3
    got = np.frombuffer(cli_run["stream"], np.uint8).reshape(n, lay.height, lay.width, 3)
    np.testing.assert_array_equal(got, video_ref.frames(src, False, *_bands(lay)))
    assert path == video.output_path("v", cli_run["ious"][0]) == f"v/iou={cli_run['ious'][0]}.mp4"
    argv = cli_run["argv"]
    assert argv[argv.index("-i") + 1:].count(path) == 1 and ("-s", "960x624") in set(zip(argv, argv[1:]))
    assert os.path.isdir(os.path.join(cli_run["root"], "v"))                     # the output directory is created


def test_cli_test_video_vs_reference_capture(cli_run, golden):
    g = golden("g13_test_video.npz")
    ref = g["frames"]
    path, lay, src = cli_run["seen"]
    got = np.frombuffer(cli_run["stream"], np.uint8).reshape(-1, lay.height, lay.width, 3)
    assert got.shape == ref.shape
    assert cli_run["ious"] == [float(v) for v in g["ious"]]
    assert path == str(g["file_name"])
    h0, c = lay.h_top, video.CELL

    def tile(a, row, col):
        return a[:, h0 + row * c:h0 + (row + 1) * c, col * c:(col + 1) * c].astype(np.int32)

    def up(m):                                      # [n,64,64] -> the tile's pixel grid
        return np.repeat(np.repeat(m, 3, axis=1), 3, axis=2)
    for row, col in ((0, 0), (1, 0), (0, 1), (1, 1), (1, 3), (1, 4)):       # RGB, ground truth, constant tiles: exact
        np.testing.assert_array_equal(tile(got, row, col), tile(ref, row, col), err_msg=f"row {row} col {col}")
    assert np.abs(tile(got, 0, 3) - tile(ref, 0, 3)).max() <= 1             # the mask M in grey: within 1 LSB
    H = cli_run["H"]
    near = {"hardM": np.abs(src["M"].astype(np.float64) - H.args.eval_thresh) <= 1e-5,
            "salhardM": np.abs(src["salM"] - H.args.salience_thresh) <= 1e-5}
    for (row, col), nm in (((0, 2), "hardM"), ((1, 2), "hardM"), ((0, 4), "salhardM")):
        diff = (tile(got, row, col) != tile(ref, row, col)).any(axis=-1)
        assert not (diff & ~up(near[nm])).any(), f"{nm} differs from the reference away from its threshold (row {row} col {col})"
    import PIL
    from PIL import features
    here = (PIL.__version__, features.version("freetype2"))
    there = (str(g["pil_version"]), str(g["freetype_version"]))
    if here != there:
        print(f"title / legend bands not compared: PIL / FreeType {here} here, {there} in the capture")
        return
    np.testing.assert_array_equal(got[:, :h0], ref[:, :h0])
    np.testing.assert_array_equal(got[:, lay.height - lay.h_bottom:], ref[:, lay.height - lay.h_bottom:])


def test_plain_eval_never_starts_ffmpeg(tmp_path, golden, g1, monkeypatch):
    root = str(tmp_path)
    _setup(root, golden, g1)
    bindir, calls = _stub_ffmpeg(root)
    monkeypatch.chdir(root)
    monkeypatch.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
    for argv in (["-eval"], ["-eval", "-salience"]):
        cli.main(argv + ["--model", "m"])
    assert os.listdir(calls) == []
    assert not [f for f in os.listdir(root) if re.match(r"iou=.*\.mp4", f)]
