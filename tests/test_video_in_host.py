"""Host side of -process --source-video: the flags and their refusals (cli.check_video_flags, cli.check_video_size), the ffprobe / ffmpeg
command lines and the streaming reader (cgs_amd.video_in) against a stub `ffmpeg` / `ffprobe` that the test writes into a temporary
bin/.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from cgs_amd import cli, handler, video, video_in  # noqa: E402

BASE = ["-process", "--source-video", "in.mp4", "--overlay-video", "out.mp4"]


# ---------------------------------------------------------------- flags
def test_flags_parse_and_defaults():
    a = cli.parse_args([])
    assert a.source_video == "" and a.overlay_video == "" and a.fit is False
    assert all(getattr(a, k) is None for k in ("smooth", "smooth_range", "overlay_layout", "overlay_color", "overlay_alpha", "overlay_outline"))
    a = cli.parse_args(BASE)
    assert a.fit is True and (a.fit_spatial, a.fit_range) == (1.0, 16.0)                 # --source-video turns the -fit machinery on
    assert (a.smooth, a.smooth_range, a.overlay_layout, a.overlay_panels) == (0, 16.0, "overlay", 1)
    assert (a.overlay_color, a.overlay_alpha, a.overlay_alpha256, a.overlay_outline) == ((0, 255, 0), 0.5, 128, 1)
    a = cli.parse_args(BASE + ["--smooth", "8", "--smooth-range", "4", "--overlay-layout", "triple", "--overlay-color", "255,0,10",
                               "--overlay-alpha", "1", "--overlay-outline", "0", "--fit-spatial", "0.5", "--fit-range", "2",
                               "--binarymaskthreshold", "0", "-fp16"])
    assert (a.smooth, a.smooth_range, a.overlay_layout, a.overlay_panels) == (8, 4.0, "triple", 3)
    assert (a.overlay_color, a.overlay_alpha256, a.overlay_outline, a.fit_spatial, a.fit_range) == ((255, 0, 10), 256, 0, 0.5, 2.0)
    assert a.fp16 and a.binarymaskthreshold == 0
    assert cli.parse_args(BASE + ["--overlay-alpha", "0.3"]).overlay_alpha256 == 77


@pytest.mark.parametrize("option", [["--overlay-video", "o.mp4"], ["--smooth", "2"], ["--smooth-range", "8"], ["--overlay-layout", "side"],
                                    ["--overlay-color", "1,2,3"], ["--overlay-alpha", "0.2"], ["--overlay-outline", "2"]])
def test_an_option_without_source_video_is_refused(option):
    with pytest.raises(ValueError) as e:
        cli.parse_args(["-process"] + option)
    assert option[0] in str(e.value) and "--source-video" in str(e.value)


def test_source_video_needs_process():
    with pytest.raises(ValueError, match="-process"):
        cli.parse_args(["--source-video", "in.mp4", "--overlay-video", "out.mp4"])


def test_source_video_needs_overlay_video():
    with pytest.raises(ValueError, match="--overlay-video"):
        cli.parse_args(["-process", "--source-video", "in.mp4"])


@pytest.mark.parametrize("extra, word", [(["-eval"], "-eval"), (["-test"], "-eval"), (["-crf"], "-crf"), (["-objects"], "-objects"),
                                         (["-salience"], "-salience"), (["-salience", "-process_salience"], "-salience"),
                                         (["-concatenated"], "-concatenated")])
def test_paths_outside_this_build_are_refused(extra, word):
    with pytest.raises(ValueError) as e:
        cli.parse_args(BASE + extra)
    assert word in str(e.value) and "outside this build" in str(e.value)


@pytest.mark.parametrize("extra, word", [
    (["--smooth", "9"], "--smooth"), (["--smooth", "-1"], "--smooth"),
    (["--smooth-range", "0"], "--smooth-range"), (["--smooth-range", "-2"], "--smooth-range"), (["--smooth-range", "nan"], "--smooth-range"),
    (["--smooth-range", "inf"], "--smooth-range"),
    (["--overlay-layout", "quad"], "--overlay-layout"),
    (["--overlay-color", "1,2"], "--overlay-color"), (["--overlay-color", "1,2,256"], "--overlay-color"),
    (["--overlay-color", "green"], "--overlay-color"), (["--overlay-color", "1,2,3,4"], "--overlay-color"),
    (["--overlay-alpha", "1.1"], "--overlay-alpha"), (["--overlay-alpha", "-0.1"], "--overlay-alpha"), (["--overlay-alpha", "nan"], "--overlay-alpha"),
    (["--overlay-outline", "5"], "--overlay-outline"), (["--overlay-outline", "-1"], "--overlay-outline"),
    (["--fit-spatial", "0.2"], "--fit-spatial"),
])
def test_values_out_of_range_are_refused(extra, word):
    with pytest.raises(ValueError) as e:
        cli.parse_args(BASE + extra)
    assert word in str(e.value)


def test_more_than_one_rank_is_refused(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one stream"):
        cli.parse_args(BASE)


def test_frame_size_checks():
    cli.check_video_size(1920, 1080, 1)
    cli.check_video_size(129, 128, 2)                                  # an odd W is fine when k W is even
    cli.check_video_size(64, 64, 3)
    for w, h, k, word in ((128, 129, 1, "even"), (129, 128, 1, "even"), (129, 128, 3, "even"), (63, 64, 1, "w = 63"),
                          (64, 4098, 1, "h = 4098"), (4097, 64, 2, "w = 4097")):
        with pytest.raises(ValueError) as e:
            cli.check_video_size(w, h, k)
        assert word in str(e.value) and "--source-video" in str(e.value)


def test_the_chunk_limits_are_class_attributes():
    assert handler.Handler.VIDEO_CHUNK_FRAMES == 128 and handler.Handler.VIDEO_CHUNK_BYTES == 256 << 20


# ---------------------------------------------------------------- command lines
def test_argv_functions():
    assert video_in.probe_argv("/x/ffprobe", "a b.mp4") == ["/x/ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
                                                            "stream=width,height,r_frame_rate", "-of", "csv=p=0", "a b.mp4"]
    assert video_in.decode_argv("/x/ffmpeg", "a b.mp4") == ["/x/ffmpeg", "-v", "error", "-i", "a b.mp4", "-an", "-sn", "-f", "rawvideo",
                                                            "-pix_fmt", "rgb24", "pipe:"]
    # the probed rate goes unchanged to both -r of the encoder
    argv = video.ffmpeg_argv("ffmpeg", "o.mp4", 3840, 1080, framerate="30000/1001")
    assert argv[argv.index("-s") + 1] == "3840x1080" and [argv[i + 1] for i, a in enumerate(argv) if a == "-r"] == ["30000/1001"] * 2


def test_parse_probe():
    assert video_in.parse_probe("1920,1080,30000/1001\n") == (1920, 1080, "30000/1001")
    assert video_in.parse_probe("128,128,10/1,\n\n") == (128, 128, "10/1")         # (some ffprobe builds end the line with a comma)
    assert video_in.parse_probe("640,360,25") == (640, 360, "25")
    for bad in ("", "\n", "1920,1080", "a,b,c", "0,1080,25/1", "1920,1080,0/1", "1920,1080,25/0", "1920,1080,x/1"):
        with pytest.raises(ValueError, match="ffprobe"):
            video_in.parse_probe(bad, "in.mp4")


# ---------------------------------------------------------------- the reader against stub executables
FFMPEG = """#!{python}
import shutil, sys
a = sys.argv[1:]
assert a[:2] == ["-v", "error"] and a[-1] == "pipe:" and "-an" in a and "-sn" in a, a
with open(a[a.index("-i") + 1], "rb") as fp:
    shutil.copyfileobj(fp, sys.stdout.buffer)
sys.stdout.buffer.flush()
sys.exit({status})
"""
FFPROBE = """#!{python}
import sys
sys.stdout.write("{answer}\\n")
sys.exit({status})
"""


def _stubs(tmp_path, monkeypatch, answer="6,4,10/1", status=0, probe_status=0, ffmpeg=True, ffprobe=True):
    bindir = tmp_path / "bin"
    bindir.mkdir()
    for name, text, wanted in (("ffmpeg", FFMPEG.format(python=sys.executable, status=status), ffmpeg),
                               ("ffprobe", FFPROBE.format(python=sys.executable, answer=answer, status=probe_status), ffprobe)):
        if wanted:
            exe = bindir / name
            exe.write_text(text)
            exe.chmod(0o755)
    monkeypatch.setenv("PATH", str(bindir))                            # nothing else: a real ffmpeg on the machine must not be found
    return bindir


def _raw(tmp_path, frames, extra=b""):
    path = tmp_path / "in.raw"
    path.write_bytes(frames.tobytes() + extra)
    return str(path)


def test_read_chunks_seven_frames_in_chunks_of_three(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch)
    frames = np.random.RandomState(0).randint(0, 256, (7, 4, 6, 3)).astype(np.uint8)
    path = _raw(tmp_path, frames)
    assert video_in.probe(path) == (6, 4, "10/1")
    got = [c.copy() for c in video_in.read_chunks(path, 3)]
    assert [len(c) for c in got] == [3, 3, 1] and all(c.dtype == np.uint8 and c.shape[1:] == (4, 6, 3) for c in got)
    np.testing.assert_array_equal(np.concatenate(got), frames)
    # the views are of two buffers: the third chunk reuses the first one's memory
    bases = [c.__array_interface__["data"][0] for c in video_in.read_chunks(path, 3, size=(6, 4))]
    assert bases[0] == bases[2] != bases[1]
    # a frame count that is a multiple of the chunk ends on the boundary; a chunk larger than the video gives one short chunk
    assert [len(c) for c in video_in.read_chunks(_raw(tmp_path, frames[:6]), 3)] == [3, 3]
    assert [len(c) for c in video_in.read_chunks(_raw(tmp_path, frames), 128)] == [7]
    # leaving the iteration early stops the decoder and the thread
    it = video_in.read_chunks(_raw(tmp_path, frames), 2)
    np.testing.assert_array_equal(next(it), frames[:2])
    it.close()


def test_read_chunks_trailing_partial_frame(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch)
    frames = np.zeros((4, 4, 6, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="5 bytes into frame 4"):
        list(video_in.read_chunks(_raw(tmp_path, frames, b"12345"), 3))


def test_read_chunks_non_zero_exit(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch, status=3)
    with pytest.raises(RuntimeError, match="status 3"):
        list(video_in.read_chunks(_raw(tmp_path, np.zeros((4, 4, 6, 3), dtype=np.uint8)), 3))


def test_read_chunks_zero_frames(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match="no frames"):
        list(video_in.read_chunks(_raw(tmp_path, np.zeros((0, 4, 6, 3), dtype=np.uint8)), 3))


def test_probe_failures(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch, answer="", probe_status=0)
    with pytest.raises(ValueError, match="ffprobe"):
        video_in.probe("in.mp4")
    monkeypatch.undo()
    (tmp_path / "bin").rename(tmp_path / "bin0")
    _stubs(tmp_path, monkeypatch, probe_status=1)
    with pytest.raises(RuntimeError, match="status 1"):
        video_in.probe("in.mp4")


def test_missing_executables(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch, ffmpeg=False, ffprobe=False)
    with pytest.raises(FileNotFoundError, match="ffprobe"):
        video_in.find_ffprobe()
    with pytest.raises(FileNotFoundError, match="ffmpeg"):
        video_in.find_ffmpeg()
    with pytest.raises(FileNotFoundError, match="ffprobe"):
        video_in.probe("in.mp4")
    with pytest.raises(FileNotFoundError, match="ffmpeg"):
        list(video_in.read_chunks("in.mp4", 3, size=(6, 4)))


def test_main_looks_for_the_executables_before_any_gpu_work(tmp_path, monkeypatch):
    _stubs(tmp_path, monkeypatch, ffprobe=False)

    def boom(*a, **k):
        raise AssertionError("the Handler was built")
    monkeypatch.setattr(handler, "Handler", boom)
    with pytest.raises(FileNotFoundError, match="ffprobe"):
        cli.main(BASE)


def test_the_documents_describe_the_path():
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(REPO, doc)) as fp:
            text = fp.read()
        assert "--source-video" in text and "--overlay-video" in text, doc
