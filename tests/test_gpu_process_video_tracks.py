"""-process --source-video --overlay-tracks end to end on the GPU, on fixture G6 with the stub `ffprobe` / `ffmpeg` of
tests/test_gpu_process_video.py (its fixture code is copied here): with --smooth 2 and the triple layout, one chunk and chunks of 3 frames
hand the encoder the same bytes, and those are overlay_tracks_ref's frames composed from the returned masks with objects.label and
objects.track of the whole stack -- which fails when the stream's numbers drift from the whole stack's at a chunk boundary.  The two
reports carry the numbers drawn, no PNG appears, and without the flag the path leaves what it always left."""
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

import overlay_tracks_ref as ref  # noqa: E402
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


def _read(path):
    with open(path) as fp:
        return json.load(fp)


def test_tracks_on_the_video_in_one_chunk_and_in_chunks_of_three(workdir, monkeypatch):
    root, frames, names, calls = workdir
    n = len(names)
    argv = ["--overlay-tracks", "0.3", "--overlay-layout", "triple", "--smooth", "2"]
    H1, M1 = _video(argv, out="one.mp4", results="R1")
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    H3, M3 = _video(argv, out="three.mp4", results="R3")
    assert n > 3                                                          # chunks of 3 split this stream
    np.testing.assert_array_equal(M1, M3)
    _, sent1 = _encoder_call(calls, 0, 128, 384)
    _, sent3 = _encoder_call(calls, 1, 128, 384)
    assert sent1.shape == (n, 128, 384, 3)
    np.testing.assert_array_equal(sent1, sent3)                           # the encoder's bytes do not depend on the chunking

    # the reference, composed from the returned masks with the whole stack's labels and tracks
    z = torch.from_numpy(np.ascontiguousarray(M1[:, 0])).to(DEV)
    guide = torch.from_numpy(np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).to(DEV)
    up = fit.up(z, guide, thresh=0.5, want=("grey", "hard"))
    res = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, min_area=1, max_objects=64)
    tr = objects.track(res.labels, iou=0.3, max_objects=64)
    ids = tr.track.cpu().numpy()
    assert int(tr.n_objects) > 0 and (ids[3:] > 0).any()                  # there are objects, also behind the chunk boundary
    want = ref.compose_tracks_ref(guide.cpu().numpy(), up.grey.cpu().numpy(), up.hard.cpu().numpy(), res.labels.cpu().numpy(), ids,
                                  res.table.cpu().numpy(), overlay.FONT, (0, 255, 0), 128, 1, 1, "triple")
    np.testing.assert_array_equal(sent1, want)
    plain = overlay.compose(guide, up.grey, up.hard, layout="triple").cpu().numpy()
    assert (sent1 != plain).any()                                         # and they are not the untracked overlay

    # TrackStream over chunks of 3 gives the numbers of tracks.json
    ts = objects.TrackStream(0.3)
    streamed = torch.cat([ts.push(res.labels[lo:lo + 3]) for lo in range(0, n, 3)]).cpu().numpy()
    np.testing.assert_array_equal(streamed, ids)
    for folder, stem in (("R1", "one"), ("R3", "three")):
        assert sorted(os.listdir(folder)) == sorted([f"{stem}.json", f"{stem}-objects.json", f"{stem}-tracks.json"])       # no PNG
        rep = _read(os.path.join(folder, f"{stem}-tracks.json"))
        keys = [f"{i:06d}" for i in range(n)]
        assert rep["order"] == keys and list(rep["frames"]) == keys and rep["track_iou"] == 0.3 and rep["min_area"] == 1
        for i, key in enumerate(keys):
            assert {r["label"]: r["track"] for r in rep["frames"][key]} == {int(l) + 1: int(streamed[i, l]) for l in np.flatnonzero(streamed[i])}
        assert rep["summary"]["tracks"] == int(tr.n_tracks) == int(ts.n_tracks)
        obj = _read(os.path.join(folder, f"{stem}-objects.json"))
        assert list(obj["frames"]) == keys and obj["connectivity"] == 8 and obj["threshold"] == 0.5
        assert [obj["frames"][k]["kept"] for k in keys] == res.kept.cpu().numpy().tolist()
        info = _read(os.path.join(folder, f"{stem}.json"))
        assert info["tracks"] == {"iou": 0.3, "min_area": 1, "boxes": 1, "scale": 1, "max_objects": 64, "n_tracks": int(tr.n_tracks),
                                  "reports": [f"{stem}-objects.json", f"{stem}-tracks.json"]}
        assert info["layout"] == "triple" and info["smooth"]["radius"] == 2


def test_the_options_reach_the_kernel_and_the_report(workdir):
    root, frames, names, calls = workdir
    H, M = _video(["--overlay-tracks", "0.6", "--overlay-boxes", "0", "--overlay-color", "255,0,200"], results="RA")
    _, sent = _encoder_call(calls, 0, 128, 128)
    z = torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV)
    guide = torch.from_numpy(np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).to(DEV)
    up = fit.up(z, guide, thresh=0.5, want=("grey", "hard"))
    res = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, min_area=1, max_objects=64)
    ids = objects.track(res.labels, iou=0.6, max_objects=64).track
    want = overlay.compose_tracks(guide, up.grey, up.hard, res.labels, ids, res.table, color=(255, 0, 200), boxes=0).cpu().numpy()
    np.testing.assert_array_equal(sent, want)
    info = _read(os.path.join("RA", "out.json"))["tracks"]
    assert (info["iou"], info["min_area"], info["boxes"]) == (0.6, 1, 0)
    # an area filter that drops the smallest object of the stream and keeps the others (the masks do not depend on it)
    areas = res.table[:, :, 0].cpu().numpy()
    least = int(areas[areas > 0].min()) + 1
    H2, M2 = _video(["--overlay-tracks", "0.6", "--overlay-min-area", str(least), "--overlay-boxes", "4"], out="b.mp4", results="RB")
    np.testing.assert_array_equal(M2, M)
    _, sent2 = _encoder_call(calls, 1, 128, 128)
    res2 = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, min_area=least, max_objects=64)
    assert 0 < int(res2.kept.sum()) < int(res.kept.sum())
    ids2 = objects.track(res2.labels, iou=0.6, max_objects=64).track
    want2 = overlay.compose_tracks(guide, up.grey, up.hard, res2.labels, ids2, res2.table, boxes=4).cpu().numpy()
    np.testing.assert_array_equal(sent2, want2)
    assert (sent2 != overlay.compose_tracks(guide, up.grey, up.hard, res2.labels, ids2, res2.table, boxes=1).cpu().numpy()).any()
    info = _read(os.path.join("RB", "b.json"))["tracks"]
    assert (info["min_area"], info["boxes"]) == (least, 4) and _read(os.path.join("RB", "b-tracks.json"))["min_area"] == least
    assert sum(f["kept"] for f in _read(os.path.join("RB", "b-objects.json"))["frames"].values()) == int(res2.kept.sum())


def test_without_the_flag_nothing_changes(workdir):
    root, frames, names, calls = workdir
    H, M = _video(["--overlay-layout", "triple", "--smooth", "2"], out="plain.mp4", results="RP")
    _, sent = _encoder_call(calls, 0, 128, 384)
    z = torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV)
    guide = torch.from_numpy(np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).to(DEV)
    up = fit.up(z, guide, thresh=0.5, want=("grey", "hard"))
    np.testing.assert_array_equal(sent, overlay.compose(guide, up.grey, up.hard, layout="triple").cpu().numpy())
    assert os.listdir("RP") == ["plain.json"]
    assert _read(os.path.join("RP", "plain.json")) == {
        "frame_size": [128, 128], "frames": len(names), "rate": "10/1", "layout": "triple", "color": [0, 255, 0], "alpha256": 128, "outline": 1,
        "threshold": 0.5, "smooth": {"radius": 2, "sigma_t": temporal.sigma_t(2), "sigma_range": 16.0}, "sigma_spatial": 1.0,
        "sigma_range": 16.0}
