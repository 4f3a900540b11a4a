"""A video file as the source of ``-process --source-video``: ``probe`` asks ``ffprobe`` for the size and the frame rate, ``read_chunks``
starts ``ffmpeg`` as a decoder and hands out its raw rgb24 frames a chunk at a time.  The mirror of ``video.stream_frames``: two (pinned)
host buffers and a reader thread that fills them with ``readinto``, so that decoding chunk c + 1 overlaps the GPU work on chunk c and
host memory stays at two chunks whatever the length of the video.  Host only; nothing here touches the GPU beyond pinning the buffers."""
import queue
import shutil
import subprocess
import threading

import torch


def find_ffprobe():
    path = shutil.which("ffprobe")
    if path is None:
        raise FileNotFoundError("the size and frame rate of --source-video are read by `ffprobe`, and no `ffprobe` is on PATH")
    return path


def find_ffmpeg():
    path = shutil.which("ffmpeg")
    if path is None:
        raise FileNotFoundError("--source-video is decoded and --overlay-video encoded by `ffmpeg`, and no `ffmpeg` is on PATH")
    return path


def probe_argv(exe, path):
    """The command line that prints "width,height,rate" of the first video stream."""
    return [exe, "-v", "error", "-select_streams", "v:0", "-show_entries", "stream=width,height,r_frame_rate", "-of", "csv=p=0", path]


def decode_argv(exe, path):
    """The command line that writes every frame of `path` as raw rgb24 to stdout, without audio and subtitles."""
    return [exe, "-v", "error", "-i", path, "-an", "-sn", "-f", "rawvideo", "-pix_fmt", "rgb24", "pipe:"]


def parse_probe(text, path=""):
    """"1920,1080,30000/1001" -> (1920, 1080, "30000/1001"): the rate stays ffprobe's own string (it goes unchanged to the encoder's -r)."""
    lines = [ln.strip() for ln in text.splitlines() if ln.strip()]
    parts = lines[0].rstrip(",").split(",") if lines else []
    try:
        if len(parts) != 3:
            raise ValueError
        w, h, rate = int(parts[0]), int(parts[1]), parts[2].strip()
        num, _, den = rate.partition("/")
        if w < 1 or h < 1 or float(num) <= 0 or (den and float(den) <= 0):
            raise ValueError
    except ValueError:
        raise ValueError(f"ffprobe {path!r}: expected 'width,height,rate' of a video stream, got {text.strip()!r}") from None
    return w, h, rate


def probe(path, ffprobe=None):
    """(W, H, rate) of the first video stream of `path`; RuntimeError when ffprobe fails, ValueError when it names no video stream."""
    exe = ffprobe or find_ffprobe()
    r = subprocess.run(probe_argv(exe, path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"ffprobe exited with status {r.returncode} on {path}: {r.stderr.strip()}")
    return parse_probe(r.stdout, path)


def _buffer(shape):
    """uint8 host array, pinned when a GPU is there to copy to (the tensor keeps the memory alive)."""
    t = torch.empty(shape, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    return t, t.numpy()


def read_chunks(path, frames_per_chunk, size=None, ffmpeg=None):
    """Yields uint8 [m,H,W,3] views (1 <= m <= frames_per_chunk) of two host buffers, the frames of `path` in order; a view is valid until
    the next one is asked for.  size: (W, H) when the caller has probed already.  The frame count is not known up front: the end of the
    stream on a frame boundary ends the iteration.  Raises RuntimeError when ffmpeg exits with a non-zero status, ValueError for a
    trailing partial frame and for a video of no frames."""
    if frames_per_chunk < 1:
        raise ValueError(f"frames_per_chunk = {frames_per_chunk}: at least 1")
    exe = ffmpeg or find_ffmpeg()
    W, H = size if size is not None else probe(path)[:2]
    frame = 3 * H * W
    keep, bufs = zip(*(_buffer((frames_per_chunk, H, W, 3)) for _ in range(2)))
    free = [threading.Semaphore(1) for _ in range(2)]
    filled, stop = queue.Queue(), threading.Event()
    proc = subprocess.Popen(decode_argv(exe, path), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE)

    def reader():
        try:
            k = 0
            while True:
                free[k].acquire()                     # the consumer is done with this buffer
                if stop.is_set():
                    return
                flat, got = memoryview(bufs[k].reshape(-1)), 0
                while got < len(flat):
                    m = proc.stdout.readinto(flat[got:])
                    if not m:
                        break
                    got += m
                filled.put((k, got))
                if got < len(flat):                   # the end of the stream
                    return
                k ^= 1
        except BaseException as e:
            filled.put(e)

    t = threading.Thread(target=reader, name="video-reader", daemon=True)
    t.start()
    frames = 0
    try:
        while True:
            item = filled.get()
            if isinstance(item, BaseException):
                raise item
            k, got = item
            whole, rest = divmod(got, frame)
            last = got < frames_per_chunk * frame
            if last:
                rc = proc.wait()
                if rc != 0:
                    raise RuntimeError(f"ffmpeg exited with status {rc} while decoding {path}")
                if rest:
                    raise ValueError(f"{path}: the stream ends {rest} bytes into frame {frames + whole} ({W}x{H} rgb24 frames are {frame} bytes)")
                if frames + whole == 0:
                    raise ValueError(f"{path}: the video holds no frames")
            if whole:
                frames += whole
                yield bufs[k][:whole]
            if last:
                return
            free[k].release()
    finally:
        stop.set()
        if proc.poll() is None:
            proc.kill()
        for s in free:
            s.release()
        t.join()
        proc.stdout.close()
        proc.wait()
        del keep
