"""-process --source-video --overlay-tracks T --overlay-gap 2 --overlay-fill end to end on the GPU, on fixture G6 with the stub `ffprobe` /
`ffmpeg` of tests/test_gpu_process_video_tracks.py (its fixture code is copied here), with --smooth 2 and the triple layout: one chunk and
chunks of 3 frames hand the encoder the same bytes and as many frames as without the flag, the masks returned are the segmented ones, and
the bytes are tests/overlay_fill_ref.py's frames composed from objects.fill of the whole stack.  G6's five frames are unrelated stills:
whether their masks hold a bridged link is printed and asserted either way, and the same path is driven once more with masks made to
flicker (process.fit_infer patched to blank two frames), where a carried object must appear."""
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

import overlay_fill_ref as ref  # noqa: E402
import overlay_tracks_ref as otr  # noqa: E402
from cgs_amd import cli, fit, handler, objects, overlay, process, temporal  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAGS = ["--overlay-tracks", "0.3", "--overlay-gap", "2", "--overlay-layout", "triple", "--smooth", "2"]

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
    """The G1 checkpoints under the names of G6, the G6 frames as in.raw (128 x 128, natural name order), and the stub executables
    first on PATH."""
    root = str(tmp_path)
    g = golden("g6_process.npz")
    for name, state in zip([str(s) for s in g["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    frames, names = g["frames"], [str(s) for s in g["names"]]
    big = np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)
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


def _sent(calls, i):
    return np.fromfile(os.path.join(calls, f"{i}.stdin"), dtype=np.uint8).reshape(-1, 128, 384, 3)


def _read(path):
    with open(path) as fp:
        return json.load(fp)


def _whole_stack(M, frames, motion=0):
    """What the path has to draw, from the returned masks: labels and tracks of the whole stack (with motion S > 0 along temporal.flow of
    the shrunk frames), objects.fill of them, the smoothed mask set to 1 where the filled label differs, the labeller's table plus the
    carried objects' rows.  Returns the pieces on the host."""
    z = torch.from_numpy(np.ascontiguousarray(M[:, 0])).to(DEV)
    guide = torch.from_numpy(np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2)).to(DEV)
    res = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, min_area=1, max_objects=64)
    bwd = temporal.flow(fit.down(guide), motion)[1] if motion else None
    tr = objects.track(res.labels, iou=0.3, max_objects=64, max_gap=2, motion=bwd)
    fl = objects.fill(res.labels, tr, motion=bwd, max_objects=64)
    zf = torch.where(fl.labels != res.labels, torch.ones_like(z), z)
    up = fit.up(zf, guide, thresh=0.5, want=("grey", "hard"))
    plain = fit.up(z, guide, thresh=0.5, want=("grey", "hard"))
    host = lambda t: t.cpu().numpy()
    return dict(guide=host(guide), grey=host(up.grey), hard=host(up.hard), labels=host(fl.labels), ids=host(fl.track),
                table=host(res.table + fl.table), age=host(fl.age), totals=objects.fill_report(fl), n_tracks=int(tr.n_tracks),
                seg=dict(grey=host(plain.grey), hard=host(plain.hard), labels=host(res.labels), ids=host(tr.track), table=host(res.table)))


def _filled_runs(calls, monkeypatch, first, extra=()):
    """The flag's run in one chunk and in chunks of 3, and the run without it: (M, the encoder's bytes with and without the flag)."""
    H1, M1 = _video(FLAGS + list(extra) + ["--overlay-fill"], out="one.mp4", results="R1")
    H0, M0 = _video(FLAGS + list(extra), out="off.mp4", results="R0")
    monkeypatch.setattr(handler.Handler, "VIDEO_CHUNK_FRAMES", 3)
    H3, M3 = _video(FLAGS + list(extra) + ["--overlay-fill"], out="three.mp4", results="R3")
    np.testing.assert_array_equal(M1, M3)
    np.testing.assert_array_equal(M1, M0)                                 # the masks returned stay the segmented ones
    sent1, sent0, sent3 = _sent(calls, first), _sent(calls, first + 1), _sent(calls, first + 2)
    assert sent1.shape == sent0.shape == (len(M1), 128, 384, 3) and len(M1) > 3          # as many frames; chunks of 3 split this stream
    np.testing.assert_array_equal(sent1, sent3)                           # the encoder's bytes do not depend on the chunking
    return M1, sent1, sent0


def _check(M, sent, sent_off, frames, motion=0):
    w = _whole_stack(M, frames, motion)
    want = ref.compose_carried_ref(w["guide"], w["grey"], w["hard"], w["labels"], w["ids"], w["table"], w["age"], overlay.FONT,
                                   (0, 255, 0), 128, 1, 1, "triple")
    np.testing.assert_array_equal(sent, want)
    s = w["seg"]                                                          # without the flag: what the path left before, by its own reference
    off = otr.compose_tracks_ref(w["guide"], s["grey"], s["hard"], s["labels"], s["ids"], s["table"], overlay.FONT, (0, 255, 0), 128, 1, 1,
                                 "triple")
    np.testing.assert_array_equal(sent_off, off)
    for folder, stem in (("R1", "one"), ("R3", "three")):
        assert sorted(os.listdir(folder)) == sorted([f"{stem}.json", f"{stem}-objects.json", f"{stem}-tracks.json"])
        info, rep = _read(os.path.join(folder, f"{stem}.json")), _read(os.path.join(folder, f"{stem}-tracks.json"))
        assert info["tracks"]["fill"] == rep["track_fill"] == w["totals"] and info["tracks"]["gap"] == 2
        assert info["tracks"]["n_tracks"] == w["n_tracks"] == rep["summary"]["tracks"]
        filled = [(key, r["label"], r["track"], r["filled"]) for key, rows in rep["frames"].items() for r in rows if "filled" in r]
        assert filled == [(f"{m:06d}", int(l) + 1, int(w["ids"][m, l]), int(w["age"][m, l])) for m, l in zip(*np.nonzero(w["age"]))]
    off_info = _read(os.path.join("R0", "off.json"))
    assert "fill" not in off_info["tracks"] and "track_fill" not in _read(os.path.join("R0", "off-tracks.json"))
    return w


def test_fill_on_the_video_in_one_chunk_and_in_chunks_of_three(workdir, monkeypatch):
    root, frames, names, calls = workdir
    M, sent, sent_off = _filled_runs(calls, monkeypatch, 0)
    w = _check(M, sent, sent_off, frames)
    new = w["totals"]["objects"]
    print(f"G6 at {' '.join(FLAGS)}: {new} carried objects, fill totals {w['totals']}")
    if new == 0:                                                          # G6's stills hold no bridged link: then the flag changes nothing here,
        np.testing.assert_array_equal(sent, sent_off)                     # and test_fill_on_flickering_masks is the one that draws a carried mask
    else:
        assert (sent != sent_off).any()


def _flicker(monkeypatch, n):
    """process.fit_infer patched: the masks of the frames BLANK of the stream are blanked, every other frame gets frame 0's mask."""
    real = process.fit_infer
    state = {"first": None, "seen": 0}

    def flicker(eng, low, *args, **kw):
        z = real(eng, low, *args, **kw).clone()
        if state["first"] is None:
            state["first"] = z[0].clone()
        for i in range(len(z)):
            z[i] = BLANK_VALUE if (state["seen"] + i) % n in BLANK else state["first"]
        state["seen"] += len(z)
        return z

    monkeypatch.setattr(process, "fit_infer", flicker)


BLANK, BLANK_VALUE = (2, 3), 0.0                                            # the frames of the stream whose masks are blanked, and to what


def test_fill_on_flickering_masks(workdir, monkeypatch):
    """The same path with the masks of frames 2 and 3 blanked and the other frames' masks made one and the same (frame 0's): the object
    of frames 0, 1 and 4 is linked over frames 2 and 3, where its carried mask is drawn hatched, at ages 1 and 2."""
    root, frames, names, calls = workdir
    _flicker(monkeypatch, len(names))
    M, sent, sent_off = _filled_runs(calls, monkeypatch, 0)
    w = _check(M, sent, sent_off, frames)
    print(f"flickering masks: fill totals {w['totals']}, ages {sorted(set(w['age'][w['age'] > 0].tolist()))}")
    assert w["totals"]["objects"] > 0 and (w["age"][list(BLANK)] > 0).any(axis=1).all()  # a carried object in every blanked frame
    assert (sent[list(BLANK)] != sent_off[list(BLANK)]).any()             # and it shows
    keep = [i for i in range(len(names)) if i not in BLANK]
    assert w["age"][keep].max() == 0


def test_fill_on_flickering_masks_with_motion(workdir, monkeypatch):
    """The same with --overlay-motion 2: the stream fills along the backward block vectors of the shrunk frames, chunk by chunk, as
    objects.fill does along temporal.flow of the whole stack."""
    root, frames, names, calls = workdir
    _flicker(monkeypatch, len(names))
    M, sent, sent_off = _filled_runs(calls, monkeypatch, 0, extra=["--overlay-motion", "2"])
    w = _check(M, sent, sent_off, frames, motion=2)
    print(f"flickering masks along motion: fill totals {w['totals']}")
    assert w["totals"]["objects"] > 0 and (sent != sent_off).any()
    assert _read(os.path.join("R1", "one.json"))["tracks"]["motion"] == 2
