"""-process --source-video end to end on the GPU, on fixture G6 with a stub `ffprobe` / `ffmpeg`: the G6 frames, replicated x2 per axis to
128 x 128 and written in natural name order as one raw rgb24 file, are "decoded" by the stub, and what the encoder is handed is saved.
Without --smooth the masks are those of plain -process on the 64 x 64 frames bit for bit and the encoder's bytes are
overlay.compose(fit.up(...)) of them; with --smooth 2 and chunks of 3 frames the masks are temporal.smooth of the unsmoothed stack in one
call, bit for bit -- which fails when a halo or the order of the two stages is wrong.  An odd size is refused after the probe, before a
decoder is started, and the paths without the new flags leave exactly the files they always left."""
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
    open(os.path.join(out, "decoded"), "a").close()
    assert a[-1] == "pipe:" and a[a.index("-pix_fmt") + 1] == "rgb24" and a[a.index("-f") + 1] == "rawvideo", a
    with open(src, "rb") as fp:
        shutil.copyfileobj(fp, sys.stdout.buffer)
"""
FFPROBE = """#!{python}
import sys
assert sys.argv[-1].endswith(".raw") and "stream=width,height,r_frame_rate" in sys.argv, sys.argv
sys.stdout.write(open({answer!r}).read())
"""


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The G1 checkpoints under the names of G6, the G6 frames as S64/ and S128/ (PNG) and as in.raw (128 x 128, natural name order), and
    the stub executables first on PATH."""
    from PIL import Image
    root = str(tmp_path)
    g = golden("g6_process.npz")
    for name, state in zip([str(s) for s in g["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    frames, names = g["frames"], [str(s) for s in g["names"]]
    os.makedirs(os.path.join(root, "S64"))
    os.makedirs(os.path.join(root, "S128"))
    big = np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)
    for nm, x, b in zip(names, frames, big):
        Image.fromarray(x).save(os.path.join(root, "S64", nm + ".png"))
        Image.fromarray(b).save(os.path.join(root, "S128", nm + ".png"))
    order = objects.natural_order(names)
    with open(os.path.join(root, "in.raw"), "wb") as fp:
        fp.write(np.ascontiguousarray(big[order]).tobytes())
    bindir, calls = os.path.join(root, "bin"), os.path.join(root, "ffmpeg_calls")
    os.makedirs(bindir)
    os.makedirs(calls)
    with open(os.path.join(root, "probe.txt"), "w") as fp:
        fp.write("128,128,10/1\n")
    for exe, text in (("ffmpeg", FFMPEG.format(python=sys.executable, out=calls)),
                      ("ffprobe", FFPROBE.format(python=sys.executable, answer=os.path.join(root, "probe.txt")))):
        with open(os.path.join(bindir, exe), "w") as fp:
            fp.write(text)
        os.chmod(os.path.join(bindir, exe), 0o755)
    monkeypatch.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
    monkeypatch.chdir(root)
    return root, frames[order], [names[i] for i in order], calls


def _video(argv, out="out.mp4", results="R"):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-video", "in.raw", "--overlay-video", out,
                                        "--mask-output-imgs", results] + argv))
    assert H.load_models()
    return H, H.segment(folder=H.args.source_imgs)


def _encoder_call(calls, i, h, w):
    with open(os.path.join(calls, f"{i}.argv")) as fp:
        argv = fp.read().split("\n")
    raw = np.fromfile(os.path.join(calls, f"{i}.stdin"), dtype=np.uint8)
    return argv, raw.reshape(-1, h, w, 3)


def _plain_masks(frames_in_order, names_in_order):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-imgs", "S64", "--mask-output-imgs", "R64"]))
    assert H.load_models()
    M = H.segment("S64")
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S64")]
    return np.stack([M[listed.index(s)] for s in names_in_order])


def _expected_frames(M, frames64, layout="overlay", thr=0.5, **kw):
    guide = torch.from_numpy(np.repeat(np.repeat(frames64, 2, axis=1), 2, axis=2)).to(DEV)
    up = fit.up(torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV), guide, thresh=thr if thr else None,
                want=("grey", "hard") if thr else ("grey",))
    return overlay.compose(guide, up.grey, up.hard, layout=layout, **kw).cpu().numpy(), up


def test_video_without_smoothing(workdir):
    root, frames, names, calls = workdir
    plain = _plain_masks(frames, names)
    before = set(os.listdir(root))
    H, M = _video([])
    assert M.shape == (len(names), 1, 64, 64) and M.dtype == np.float32
    np.testing.assert_array_equal(M, plain)                              # the network saw exactly what plain -process shows it
    argv, sent = _encoder_call(calls, 0, 128, 128)
    assert argv[argv.index("-s") + 1] == "128x128" and [argv[i + 1] for i, a in enumerate(argv) if a == "-r"] == ["10/1", "10/1"]
    assert argv[argv.index("-i") + 1] == "pipe:" and "out.mp4" in argv and argv[argv.index("-pix_fmt") + 1] == "rgb24"
    want, up = _expected_frames(M, frames)
    assert 0 < float(up.hard.float().mean()) < 1
    np.testing.assert_array_equal(sent, want)
    assert (sent != np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).any()
    with open(os.path.join("R", "out.json")) as fp:
        assert json.load(fp) == {"frame_size": [128, 128], "frames": len(names), "rate": "10/1", "layout": "overlay", "color": [0, 255, 0],
                                 "alpha256": 128, "outline": 1, "threshold": 0.5, "smooth": None, "sigma_spatial": 1.0, "sigma_range": 16.0}
    assert os.listdir("R") == ["out.json"]                               # no PNG
    assert set(os.listdir(root)) - before == {"R"}                       # (the stub encoder writes no out.mp4)

    # side by side, other colour / alpha / outline / sigmas, no hard mask at threshold 0: all of it reaches the kernels and the report
    H2, M2 = _video(["--overlay-layout", "side", "--overlay-color", "255,0,200", "--overlay-alpha", "0.25", "--overlay-outline", "3",
                     "--fit-range", "4"], out="v/side.mp4", results="R2")
    np.testing.assert_array_equal(M2, M)
    argv2, sent2 = _encoder_call(calls, 1, 128, 256)
    assert argv2[argv2.index("-s") + 1] == "256x128" and "v/side.mp4" in argv2
    guide = torch.from_numpy(np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).to(DEV)
    up2 = fit.up(torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV), guide, sigma_r=4.0, thresh=0.5, want=("grey", "hard"))
    want2 = overlay.compose(guide, up2.grey, up2.hard, color=(255, 0, 200), alpha256=64, outline=3, layout="side").cpu().numpy()
    np.testing.assert_array_equal(sent2, want2)
    np.testing.assert_array_equal(sent2[:, :, :128], guide.cpu().numpy())
    with open(os.path.join("R2", "side.json")) as fp:
        rep = json.load(fp)
    assert (rep["layout"], rep["color"], rep["alpha256"], rep["outline"], rep["sigma_range"]) == ("side", [255, 0, 200], 64, 3, 4.0)
    H3, M3 = _video(["--binarymaskthreshold", "0", "--overlay-layout", "triple"], out="t.mp4", results="R3")
    _, sent3 = _encoder_call(calls, 2, 128, 384)
    want3, _ = _expected_frames(M, frames, layout="triple", thr=0)
    np.testing.assert_array_equal(sent3, want3)


def test_video_with_smoothing_in_chunks(workdir, monkeypatch):
    root, frames, names, calls = workdir
    _, M0 = _video([], out="plain.mp4", results="R0")
    low = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)          # fit.down of the replicated frames is the 64 x 64 frame
    z = torch.from_numpy(np.ascontiguousarray(M0[:, 0])).to(DEV)
    want = temporal.smooth(z, low, 2, 16.0).cpu().numpy()[:, None]
    assert np.abs(want - M0).max() > 1e-3                                 # the smoothing changes these masks
    for i, chunk in enumerate((3, 1, 128)):                               # two chunks with a halo each; chunks shorter than the radius; one chunk
        monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", chunk)
        H, M = _video(["--smooth", "2"], out=f"s{chunk}.mp4", results=f"RS{chunk}")
        np.testing.assert_array_equal(M, want, err_msg=f"chunks of {chunk}")
        _, sent = _encoder_call(calls, 1 + i, 128, 128)
        np.testing.assert_array_equal(sent, _expected_frames(want, frames)[0], err_msg=f"chunks of {chunk}")
        with open(os.path.join(f"RS{chunk}", f"s{chunk}.json")) as fp:
            assert json.load(fp)["smooth"] == {"radius": 2, "sigma_t": 1.0, "sigma_range": 16.0}
    # the range sigma reaches the kernel
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    _, M4 = _video(["--smooth", "1", "--smooth-range", "64"], out="r.mp4", results="RR")
    np.testing.assert_array_equal(M4, temporal.smooth(z, low, 1, 64.0).cpu().numpy()[:, None])


def test_odd_size_is_refused_after_the_probe_and_the_old_paths_are_unchanged(workdir):
    root, frames, names, calls = workdir
    with open("probe.txt", "w") as fp:
        fp.write("128,129,10/1\n")
    with pytest.raises(ValueError, match="even"):
        _video([])
    with open("probe.txt", "w") as fp:
        fp.write("129,128,10/1\n")
    with pytest.raises(ValueError, match="even"):
        _video(["--overlay-layout", "triple"])
    with open("probe.txt", "w") as fp:
        fp.write("32,128,10/1\n")
    with pytest.raises(ValueError, match="w = 32"):
        _video([])
    assert os.listdir(calls) == [] and not os.path.exists("R")           # no decoder and no encoder was started, nothing was written
    # plain -process and -process -fit: exactly the files they left before
    for argv, folder, out, extra in (([], "S64", "P64", []), (["-fit"], "S128", "P128", ["fit.json"])):
        H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-imgs", folder, "--mask-output-imgs", out] + argv))
        assert H.load_models()
        H.segment(folder)
        assert sorted(os.listdir(out)) == sorted([f"{s}-{k}.png" for s in names for k in ("raw-mask", "thresholded-mask")] + extra)
    assert os.listdir(calls) == []
