"""The evaluation video of ``-test`` / ``-eval --output-video`` (main.py:1027-1087): the layout plan, the title and legend bands, the
GPU frame composition (``cgs_video_compose``, csrc/video.hip) and the ffmpeg pipe.

The reference builds every frame on the host (about 11 GB of float32 interpolation output and 18 GB of finished frames at the full
evaluation set) and hands the whole stack to ffmpeg.  Here the frames are composed on the GPU a chunk at a time into two pinned host
buffers, and a writer thread feeds the encoder: composing chunk k + 1 overlaps writing chunk k, and host memory stays at two chunks."""
import os
import queue
import shutil
import subprocess
import threading
from collections import namedtuple

import numpy as np
import torch

from . import _lib

REFERENCE_FONT = "./isy_minerl/segm/etc/Ubuntu-R.ttf"     # main.py:1036, relative to the working directory
FONT_SIZE = 30                                             # fosi
TILE, SCALE = 64, 3                                        # 64 x 64 tiles, x3 nearest (scalef)
CELL = TILE * SCALE
FRAMERATE = 10
CHUNK = 64                                                 # frames per composition launch / pinned buffer
NONTEMPORAL = True                                         # non-temporal stores: measured faster (tools/time_video.py)
TITLES = ["RGB\nimage", "ground\ntruth", "mask", "thresholded\nmask\nIoU=0.41", "mask\nCRF\nIoU=0.45", "saliency\nmap",
          "thresholded\nsaliency\nIoU=0.22", "salience\nCRF\nIoU=0.11"]
LEGEND = ["GREEN = True Positive", "RED = False Negative", "GRAY = False Positive", "BLACK = True Negative"]
LEGEND_COLORS = [(0, 255, 0), (255, 0, 0), (125, 125, 125), (255, 255, 255)]
CODED = (0, 2, 3, 5, 6)           # allM indices shown colour-coded in the second row; every other index is a constant 0.1 tile
CONST_VALUE = 0.1
GREY, CODE, CONST = _lib.VIDEO_GREY, _lib.VIDEO_CODE, _lib.VIDEO_CONST

# row1 / row2: one (source name, mode) per column; the name is None for a CONST tile.  Source names are the reference's: "X" (the RGB
# frames) and the entries of its allM list.
Layout = namedtuple("Layout", "row1 row2 titles short h_top h_bottom width height")


def wanted(args):
    """The video is rendered for -test (which forces -visbesteval on) and for -eval with --output-video; -visbesteval '' turns it off.
    A plain -eval writes none (the reference would, at main.py:1027, and raise for most flag sets)."""
    return bool(args.visbesteval) and bool(args.test or args.output_video)


def allm_names(crf):
    """The reference's allM list (main.py:929, 957, 970, 997, 1001) by name."""
    return ["Y", "M", "hardM"] + (["crfM"] if crf else []) + ["salM", "salhardM"] + (["salcrfM"] if crf else [])


def plan(crf, salience):
    """Columns, modes, titles and sizes of the frame as main.py:1028-1083 assemble it.  The reference only renders with -salience:
    without it (with or without -crf) its colour columns are indexed past their end."""
    if not salience:
        raise NotImplementedError("the evaluation video needs -salience: without it the reference's frame assembly indexes past its "
                                  "column lists (main.py:1028-1055, IndexError at main.py:1055)" + (" with -crf" if crf else ""))
    names = allm_names(crf)
    reordering = [0, 1, 4, 3, 2, 7, 6, 5] if crf else [0, 1, 3, 2, 5]
    grey = ["X"] + names
    row1 = tuple((grey[i], GREY) for i in reordering[:len(names) + 1])
    coded = [("X", GREY)] + [(nm, CODE) if i in CODED else (None, CONST) for i, nm in enumerate(names)]
    row2 = tuple(coded[i] for i in reordering)
    short = len(reordering) != 8
    h_top, h_bottom = FONT_SIZE * 4, FONT_SIZE * (4 if short else 2)
    width = CELL * len(reordering)
    return Layout(row1, row2, tuple(TITLES[i] for i in reordering), short, h_top, h_bottom, width, h_top + 2 * CELL + h_bottom)


def resolve_font(size=FONT_SIZE):
    """(font, where it came from): the reference's TrueType file when it exists, else matplotlib's DejaVuSans.ttf, else PIL's default."""
    from PIL import ImageFont
    if os.path.isfile(REFERENCE_FONT):
        return ImageFont.truetype(REFERENCE_FONT, size), REFERENCE_FONT
    try:
        import matplotlib
        path = os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf")
    except ImportError:
        path = None
    if path and os.path.isfile(path):
        return ImageFont.truetype(path, size), path
    return ImageFont.load_default(size=size), "PIL default"


def render_bands(layout, font):
    """The title band (white titles at (6 + 192 i, 6)) and the legend band (four coloured entries, int((W - 2) / 4) apart) of
    main.py:1060-1078, drawn once: uint8 [h_top, W, 3], [h_bottom, W, 3]."""
    from PIL import Image, ImageDraw
    top = Image.fromarray(np.zeros((layout.h_top, layout.width, 3), dtype=np.uint8))
    draw = ImageDraw.Draw(top)
    for i, text in enumerate(layout.titles):
        draw.text((FONT_SIZE // 5 + CELL * i, FONT_SIZE // 5), text, font=font)
    bottom = Image.fromarray(np.zeros((layout.h_bottom, layout.width, 3), dtype=np.uint8))
    spacing = int((layout.width - 2) / len(LEGEND))
    draw = ImageDraw.Draw(bottom)
    for i, text in enumerate(LEGEND):
        draw.text((FONT_SIZE // 5 + i * spacing, FONT_SIZE // 5), text + ("\n" if layout.short and i > 1 else ""), font=font,
                  fill=LEGEND_COLORS[i])
    return np.array(top), np.array(bottom)


def find_ffmpeg():
    path = shutil.which("ffmpeg")
    if path is None:
        raise FileNotFoundError("the evaluation video is encoded by `ffmpeg` (libx264), and no `ffmpeg` is on PATH")
    return path


def ffmpeg_argv(exe, path, width, height, framerate=FRAMERATE):
    """The command line of vidwrite's ffmpeg chain (main.py:45-55): raw rgb24 frames on stdin, yuv420p libx264 out, overwrite."""
    return [exe, "-f", "rawvideo", "-pix_fmt", "rgb24", "-r", str(framerate), "-s", f"{width}x{height}", "-i", "pipe:",
            "-pix_fmt", "yuv420p", "-r", str(framerate), "-vcodec", "libx264", path, "-y"]


def output_path(output_video, iou):
    """main.py:1085-1087: f"{output_video}/iou={round(iou, 3)}.mp4", or iou=....mp4 in the working directory without --output-video."""
    return f"{output_video + '/' if output_video else ''}iou={round(iou, 3)}.mp4"


def _source(a):
    """numpy stack -> (contiguous array, cell kind): RGB frames uint8 [n,64,64,3]; masks bool / uint8 0/1 and maps fp32 / fp64
    [n,64,64] (or [n,1,64,64])."""
    a = np.asarray(a)
    if a.ndim == 4 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim == 4 and a.shape[1:] == (TILE, TILE, 3) and a.dtype == np.uint8:
        return np.ascontiguousarray(a), _lib.VIDEO_RGB8
    if a.ndim != 3 or a.shape[1:] != (TILE, TILE):
        raise ValueError(f"a video source must be [n,{TILE},{TILE}] (or RGB uint8 [n,{TILE},{TILE},3]), got {a.dtype} {a.shape}")
    if a.dtype == bool or a.dtype == np.uint8:
        return np.ascontiguousarray(a, dtype=np.uint8), _lib.VIDEO_MASK8
    if a.dtype == np.float32:
        return np.ascontiguousarray(a), _lib.VIDEO_F32
    if a.dtype == np.float64:
        return np.ascontiguousarray(a), _lib.VIDEO_F64
    raise ValueError(f"unsupported video source dtype {a.dtype}")


class Composer:
    """The sources of one video on the device and the launch descriptor; ``compose(f0, n)`` gives frames f0 .. f0 + n - 1."""

    def __init__(self, layout, sources, device="cuda", font=None):
        if not torch.cuda.is_available():
            raise _lib.CgsError("the video frames are composed on the GPU (cgs_video_compose); no GPU is visible and there is no CPU fallback")
        device = torch.device(device)
        self.layout = layout
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        needed = {nm for nm, mode in layout.row1 + layout.row2 if nm is not None}
        if any(mode == CODE for _, mode in layout.row2):
            needed.add("Y")
        missing = needed - set(sources)
        if missing:
            raise ValueError(f"video sources missing: {sorted(missing)}")
        self._dev, kinds, counts = {}, {}, set()
        for nm in sorted(needed):
            a, kinds[nm] = _source(sources[nm])
            counts.add(len(a))
            self._dev[nm] = torch.from_numpy(a).to(self.device)
        if len(counts) != 1 or 0 in counts:
            raise ValueError(f"video sources must hold the same (non-zero) number of frames, got {sorted(counts)}")
        self.n = counts.pop()
        font = font if font is not None else resolve_font()[0]
        top, bottom = render_bands(layout, font)
        self.bands = (top, bottom)
        self._top, self._bottom = torch.from_numpy(top).to(self.device), torch.from_numpy(bottom).to(self.device)
        cells = []
        for nm, mode in layout.row1 + layout.row2:
            if mode == CONST:
                cells.append(_lib.VideoCell(None, None, CONST_VALUE, 0, CONST))
            else:
                y = self._dev["Y"].data_ptr() if mode == CODE else None
                if mode == CODE and kinds[nm] != _lib.VIDEO_MASK8:
                    raise ValueError(f"colour-coded column {nm} must be a 0/1 mask")
                cells.append(_lib.VideoCell(self._dev[nm].data_ptr(), y, 0.0, kinds[nm], mode))
        self._cols = len(layout.row1)
        self._cells = (_lib.VideoCell * len(cells))(*cells)
        self.frame_shape = (layout.height, layout.width, 3)

    def compose(self, f0, n, out=None, nontemporal=NONTEMPORAL):
        """Frames f0 .. f0 + n - 1 as device uint8 [n, H, W, 3] (into `out` when given), on the current stream."""
        if not (0 <= f0 and 1 <= n and f0 + n <= self.n):
            raise ValueError(f"frames {f0}..{f0 + n} outside the {self.n} frames of this video")
        if out is None:
            out = torch.empty((n,) + self.frame_shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape[1:]) != self.frame_shape or len(out) < n \
                or out.device != self.device:
            raise ValueError(f"out must be contiguous uint8 [>={n}, {self.frame_shape}] on {self.device}")
        flags = _lib.VIDEO_NONTEMPORAL if nontemporal else 0
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.call("cgs_video_compose", self._cells, 2, self._cols, f0, n, self._top.data_ptr(), self.layout.h_top,
                      self._bottom.data_ptr(), self.layout.h_bottom, flags, out.data_ptr(), stream)
        return out[:n]


def stream_frames(comp, sink, chunk=CHUNK):
    """Every frame of `comp`, in order, written to sink.write (bytes-like, rgb24): composed on the GPU `chunk` frames at a time, copied
    into one of two pinned host buffers and written by a second thread while the next chunk is composed.  Returns the bytes written."""
    n, c = comp.n, min(chunk, comp.n)
    dev_out = torch.empty((c,) + comp.frame_shape, dtype=torch.uint8, device=comp.device)
    hosts = [torch.empty((c,) + comp.frame_shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    free = [threading.Semaphore(1) for _ in range(2)]
    todo, err, written = queue.Queue(), [], [0]

    def writer():
        while True:
            item = todo.get()
            if item is None:
                return
            k, cnt, ev = item
            try:
                if not err:
                    ev.synchronize()
                    buf = hosts[k].numpy()[:cnt].reshape(-1)
                    sink.write(memoryview(buf))
                    written[0] += buf.nbytes
            except BaseException as e:      # (a closed pipe: reported by the caller after the thread has stopped)
                err.append(e)
            finally:
                free[k].release()

    t = threading.Thread(target=writer, name="video-writer", daemon=True)
    t.start()
    try:
        with torch.cuda.device(comp.device):
            for i, f0 in enumerate(range(0, n, c)):
                k, cnt = i % 2, min(c, n - f0)
                free[k].acquire()                    # the writer is done with this buffer
                if err:
                    break
                comp.compose(f0, cnt, out=dev_out)
                hosts[k][:cnt].copy_(dev_out[:cnt], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                todo.put((k, cnt, ev))
    finally:
        todo.put(None)
        t.join()
    if err:
        raise err[0]
    return written[0]


class FrameWriter:
    """Finished frames from the device to a byte sink (an encoder's stdin), a chunk at a time: ``submit`` copies a device chunk into one of
    two pinned host buffers without waiting, and a writer thread hands the buffer to sink.write once its copy has landed -- the
    double buffer of stream_frames for a caller that composes its chunks itself.  ``close`` drains and re-raises a failed write."""

    def __init__(self, sink, frame_shape, chunk):
        self.sink, self.frame_shape, self.written = sink, tuple(frame_shape), 0
        self._hosts = [torch.empty((chunk,) + self.frame_shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._free = [threading.Semaphore(1) for _ in range(2)]
        self._todo, self._err, self._i = queue.Queue(), [], 0
        self._thread = threading.Thread(target=self._run, name="video-writer", daemon=True)
        self._thread.start()

    def _run(self):
        while True:
            item = self._todo.get()
            if item is None:
                return
            k, cnt, ev = item
            try:
                if not self._err:
                    ev.synchronize()
                    buf = self._hosts[k].numpy()[:cnt].reshape(-1)
                    self.sink.write(memoryview(buf))
                    self.written += buf.nbytes
            except BaseException as e:      # (a closed pipe: reported by close after the thread has stopped)
                self._err.append(e)
            finally:
                self._free[k].release()

    def submit(self, frames):
        """frames: device uint8 [m, *frame_shape], m at most the chunk; copied on the current stream."""
        cnt = len(frames)
        if tuple(frames.shape[1:]) != self.frame_shape or frames.dtype != torch.uint8 or not 1 <= cnt <= len(self._hosts[0]):
            raise ValueError(f"a chunk is uint8 [1..{len(self._hosts[0])}, {self.frame_shape}], got {frames.dtype} {tuple(frames.shape)}")
        k = self._i % 2
        self._i += 1
        self._free[k].acquire()                  # the writer is done with this buffer
        if self._err:
            self._free[k].release()
            raise self._err[0]
        self._hosts[k][:cnt].copy_(frames, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._todo.put((k, cnt, ev))

    def close(self):
        if self._thread is not None:
            self._todo.put(None)
            self._thread.join()
            self._thread = None
        if self._err:
            raise self._err[0]
        return self.written


def write_video(path, layout, sources, device="cuda", ffmpeg=None, chunk=CHUNK, font=None):
    """Encodes the video of main.py:1027-1087 to `path` with ffmpeg (ffmpeg_argv); raises if ffmpeg fails.  Returns the frame count."""
    exe = ffmpeg or find_ffmpeg()
    comp = Composer(layout, sources, device, font)
    out_dir = os.path.dirname(path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    proc = subprocess.Popen(ffmpeg_argv(exe, path, layout.width, layout.height), stdin=subprocess.PIPE)
    failure = None
    try:
        stream_frames(comp, proc.stdin, chunk)
    except BrokenPipeError as e:
        failure = e
    finally:
        try:
            proc.stdin.close()
        except BrokenPipeError:
            pass
    rc = proc.wait()
    if rc != 0 or failure is not None:
        raise RuntimeError(f"ffmpeg exited with status {rc} while writing {path}" + (f" ({failure})" if failure else ""))
    return comp.n
