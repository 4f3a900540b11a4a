"""-process --source-video --smooth R --smooth-motion S end to end on the GPU, with the stub `ffprobe` / `ffmpeg` arrangement of
tests/test_gpu_process_video.py: a clip of eight frames made by sliding a 64 x 64 window three cells a frame over two frames of fixture G6
set side by side (so there is real motion), replicated x2 per axis to 128 x 128 and written as one raw rgb24 file, is "decoded" by the stub,
and what the encoder is handed is saved.  With --smooth 2 --smooth-motion 4 and chunks of 3 frames and of 1 frame the masks
are temporal.smooth(..., motion=temporal.flow(low, 4)) of the unsmoothed stack in one call, bit for bit -- which fails when the motion is
taken from another window than the smoother's --, the encoder receives the frames composed from them and the report carries the motion
figures of the whole clip, each frame pair counted once.  Without --smooth-motion the report has no such key and the masks are those of
the plain filter."""
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

from cgs_amd import cli, fit, handler, objects, overlay, temporal  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES, STEP = 8, 3                     # frames of the clip, cells a frame

FFMPEG = """#!{python}
import os, shutil, sys
out = {out!r}
a = sys.argv[1:]
src = a[a.index("-i") + 1]
if src == "pipe:":                      # the encoder: keep the command line and everything on stdin
    n = len([f for f in os.listdir(out) if f.endswith(".argv")])
    with open(os.path.join(out, f"{{n}}.argv"), "w") as fp:
        fp.write("\\n".join(sys.argv))
    with open(os.path.join(out, f"{{n}}.stdin"), "wb") as fp:
        shutil.copyfileobj(sys.stdin.buffer, fp)
else:                                   # the decoder: the file is raw rgb24 already
    assert a[-1] == "pipe:" and a[a.index("-pix_fmt") + 1] == "rgb24" and a[a.index("-f") + 1] == "rawvideo", a
    with open(src, "rb") as fp:
        shutil.copyfileobj(fp, sys.stdout.buffer)
"""
FFPROBE = """#!{python}
import sys
assert sys.argv[-1].endswith(".raw") and "stream=width,height,r_frame_rate" in sys.argv, sys.argv
sys.stdout.write("128,128,10/1\\n")
"""


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The G1 checkpoints under the names of G6, the sliding clip as in.raw (128 x 128), and the stub executables first on PATH.
    Returns (the clip at 64 x 64 [8,64,64,3], the folder of the encoder's calls)."""
    root = str(tmp_path)
    g = golden("g6_process.npz")
    for name, state in zip([str(s) for s in g["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    order = objects.natural_order([str(s) for s in g["names"]])
    wide = np.concatenate((g["frames"][order[0]], g["frames"][order[1]]), axis=1)        # 64 x 128
    clip = np.stack([wide[:, STEP * f:STEP * f + 64] for f in range(FRAMES)])
    with open(os.path.join(root, "in.raw"), "wb") as fp:
        fp.write(np.ascontiguousarray(np.repeat(np.repeat(clip, 2, axis=1), 2, axis=2)).tobytes())
    bindir, calls = os.path.join(root, "bin"), os.path.join(root, "ffmpeg_calls")
    os.makedirs(bindir)
    os.makedirs(calls)
    for exe, text in (("ffmpeg", FFMPEG.format(python=sys.executable, out=calls)), ("ffprobe", FFPROBE.format(python=sys.executable))):
        with open(os.path.join(bindir, exe), "w") as fp:
            fp.write(text)
        os.chmod(os.path.join(bindir, exe), 0o755)
    monkeypatch.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
    monkeypatch.chdir(root)
    return np.ascontiguousarray(clip), calls


def _video(argv, out, results):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-video", "in.raw", "--overlay-video", out,
                                        "--mask-output-imgs", results] + argv))
    assert H.load_models()
    return H.segment(folder=H.args.source_imgs)


def _sent(calls, i):
    return np.fromfile(os.path.join(calls, f"{i}.stdin"), dtype=np.uint8).reshape(-1, 128, 128, 3)


def _expected_frames(M, clip):
    guide = torch.from_numpy(np.repeat(np.repeat(clip, 2, axis=1), 2, axis=2)).to(DEV)
    up = fit.up(torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV), guide, thresh=0.5, want=("grey", "hard"))
    return overlay.compose(guide, up.grey, up.hard, layout="overlay").cpu().numpy()


def test_video_smoothed_along_the_motion_in_chunks(workdir, monkeypatch):
    clip, calls = workdir
    M0 = _video([], "plain.mp4", "R0")
    assert M0.shape == (FRAMES, 1, 64, 64)
    low = torch.from_numpy(clip).to(DEV)                                  # fit.down of the replicated frames is the 64 x 64 frame
    z = torch.from_numpy(np.ascontiguousarray(M0[:, 0])).to(DEV)
    fwd, bwd = temporal.flow(low, 4)
    assert float((fwd == torch.tensor([0, -STEP], dtype=torch.int8, device=DEV)).all(dim=-1).float().mean()) > 0.5       # the slide is found
    want = temporal.smooth(z, low, 2, 16.0, motion=(fwd, bwd)).cpu().numpy()[:, None]
    plain = temporal.smooth(z, low, 2, 16.0).cpu().numpy()[:, None]
    assert np.abs(want - plain).max() > 1e-3                              # the motion changes these masks
    lengths = fwd.double().pow(2).sum(dim=-1).sqrt()
    for i, chunk in enumerate((3, 1)):                                    # chunks with a halo each; chunks shorter than the radius
        monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", chunk)
        M = _video(["--smooth", "2", "--smooth-motion", "4"], f"m{chunk}.mp4", f"RM{chunk}")
        np.testing.assert_array_equal(M, want, err_msg=f"chunks of {chunk}")
        np.testing.assert_array_equal(_sent(calls, 1 + i), _expected_frames(want, clip), err_msg=f"chunks of {chunk}")
        with open(os.path.join(f"RM{chunk}", f"m{chunk}.json")) as fp:
            rep = json.load(fp)["smooth"]
        motion = rep.pop("motion")
        assert rep == {"radius": 2, "sigma_t": 1.0, "sigma_range": 16.0}
        assert sorted(motion) == ["block", "mean_cells_per_frame", "saturated", "search"] and (motion["search"], motion["block"]) == (4, 8)
        assert 0.0 <= motion["saturated"] <= 1.0
        assert abs(motion["saturated"] - float((fwd.abs().amax(dim=-1) >= 4).double().mean())) < 1e-12      # every pair once, whatever the chunks
        assert abs(motion["mean_cells_per_frame"] - float(lengths.mean())) < 1e-12 and 2.0 < motion["mean_cells_per_frame"] < 4.0
    # a smaller search reaches the kernel and the report: the slide of 3 is out of reach of S = 2, more vectors saturate
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    M2 = _video(["--smooth", "2", "--smooth-motion", "2"], "s2.mp4", "RS2")
    near = temporal.flow(low, 2)
    np.testing.assert_array_equal(M2, temporal.smooth(z, low, 2, 16.0, motion=near).cpu().numpy()[:, None])
    with open(os.path.join("RS2", "s2.json")) as fp:
        motion2 = json.load(fp)["smooth"]["motion"]
    assert motion2["search"] == 2 and abs(motion2["saturated"] - float((near[0].abs().amax(dim=-1) >= 2).double().mean())) < 1e-12
    assert motion2["saturated"] > motion["saturated"]

    # the same run without --smooth-motion: no such key, the masks of the plain filter
    Mp = _video(["--smooth", "2"], "p.mp4", "RP")
    np.testing.assert_array_equal(Mp, plain)
    with open(os.path.join("RP", "p.json")) as fp:
        assert json.load(fp)["smooth"] == {"radius": 2, "sigma_t": 1.0, "sigma_range": 16.0}
    with open(os.path.join("R0", "plain.json")) as fp:
        assert json.load(fp)["smooth"] is None
