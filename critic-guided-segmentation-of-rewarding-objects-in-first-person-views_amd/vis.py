"""The -viscritic / -vismasker videos (Handler.visualize, main.py:702-884): every test frame, with -vismasker the masked frame under it,
then two scrolling value curves (ground-truth reward, critic prediction); one video in time order, one sorted by the prediction and,
with --sortidx != 0, one sorted by the ground truth.

The reference composes every frame in a Python loop on the host, once per video, and stacks a whole video in host memory before ffmpeg
sees a byte.  Here the frames, masks and tables are uploaded once, ``cgs_vis_compose`` (csrc/vis.hip) builds the frames of a chunk in
one launch -- the permuted gather, the x4 upscale, the plot windows and the label blend -- and ``video.stream_frames`` feeds the
encoder through its two pinned buffers.  What stays on the host is N numbers per curve (the plot rows, float64 as the reference), the
sort (the reference's numpy call) and PIL's rendering of each DISTINCT label string: that image is the coverage the kernel blends."""
import os
import subprocess
from collections import namedtuple

import numpy as np
import torch

from . import _lib, video

TILE, SCALE, PLOT_H = 64, 4, 32                      # 64 x 64 tiles, x4 nearest (scale), 32 source rows per curve (ph)
VALUES = _lib.VIS_VALUES                             # the two curves: ground truth, prediction
CELL_W, CELL_H = _lib.VIS_CELL_W, _lib.VIS_CELL_H    # atlas cell of one label
FRAMERATE = 4                                        # main.py:874
CHUNK = 128                                          # frames per composition launch / pinned buffer (75 MB at 256 x 768)
NONTEMPORAL = True                                   # store policy: DESIGN.md section 4, tools/time_vis.py

Plan = namedtuple("Plan", "R V width height")
Tables = namedtuple("Tables", "rows ids atlas")      # device tensors shared by the videos of one run


def plan(vismasker):
    """Image rows R (1: the frame; 2: the masked frame under it), value rows V, and the frame size 4 x (64, 64 R + 32 V)."""
    R = 2 if vismasker else 1
    return Plan(R, VALUES, SCALE * TILE, SCALE * (TILE * R + PLOT_H * VALUES))


def refuse_unbuilt(args):
    """What of Handler.visualize stays outside this build, and the one state the reference cannot survive either."""
    if args.purevis:
        raise NotImplementedError("--purevis is outside this build's scope (the reference indexes frames where it means value rows, "
                                  "main.py:764-767)")
    if not args.train:
        raise ValueError("-viscritic / -vismasker show the test split that -train loads (self.XX, main.py:744-746): without -train "
                         "the reference fails on the missing attribute; add -train (with -critic '' -masker '' to load the checkpoints "
                         "instead of training)")


def plot_rows(values):
    """make_plotbar's pixel row of every value (main.py:31-37), float64 on the host: uint8 [V, N] in 0..31 (a constant curve: 31)."""
    values = np.asarray(values, dtype=np.float64)
    out = []
    for v in np.atleast_2d(values):
        shifted = v - np.min(v)
        top = shifted.max()
        shifted = shifted / ((top * 1.01) if top else 1)
        out.append(PLOT_H - 1 - np.floor(shifted * PLOT_H).astype(np.int64))
    out = np.stack(out)
    assert out.min() >= 0 and out.max() < PLOT_H
    return out.astype(np.uint8).reshape(values.shape)


def label_strings(values, n):
    """Per source frame p the three strings main.py:858-862 draw: str(p), then str(round(value, 3)) of each curve."""
    values = np.asarray(values, dtype=np.float64)
    return [[str(p)] + [str(round(values[v, p].item(), 3)) for v in range(VALUES)] for p in range(n)]


def render_label(text):
    """uint8 [CELL_H, CELL_W]: the coverage of `text` as ImageDraw.text draws it at (0, 0) with PIL's default font.  White on black:
    PIL's blend of 255 over 0 through a gives back a, so the image is the mask."""
    from PIL import Image, ImageDraw
    img = Image.new("RGB", (CELL_W, CELL_H))
    draw = ImageDraw.Draw(img)
    left, top, right, bottom = draw.textbbox((0, 0), text)
    if left < 0 or top < 0 or right > CELL_W or bottom > CELL_H:
        raise ValueError(f"label {text!r} covers {(left, top, right, bottom)}, outside its {CELL_W} x {CELL_H} atlas cell")
    draw.text((0, 0), text, fill=(255, 255, 255))
    return np.array(img)[:, :, 0]


def labels(values, n):
    """(atlas uint8 [L, CELL_H, CELL_W], ids int32 [n, 3], strings): one cell per DISTINCT string, and per source frame the cells of
    its index label and its two value labels.  All three are functions of the source frame, so one table serves every sorting."""
    return pack_labels(label_strings(values, n))


def pack_labels(strings):
    """labels() for given strings: strings[p] = (index label, value label 0, value label 1) of source frame p."""
    cell_of = {}
    ids = np.array([[cell_of.setdefault(s, len(cell_of)) for s in row] for row in strings], dtype=np.int32).reshape(-1, 1 + VALUES)
    atlas = np.stack([render_label(s) for s in cell_of])
    return atlas, ids, list(cell_of)


def label_positions(height):
    """(x, y) of the index label and the value labels (main.py:857-862), in ids' column order."""
    return [(_lib.VIS_INDEX_X, height - 12 - SCALE * PLOT_H * VALUES - 1)] + \
           [(_lib.VIS_VALUE_X, _lib.VIS_VALUE_Y + _lib.VIS_VALUE_DY * v) for v in range(VALUES)]


def sortings(values, sortidx):
    """[(file-name suffix, perm or None)] in the reference's order (main.py:879-884); the sort is the reference's numpy call."""
    values = np.asarray(values)
    out = [("", None), ("-pred-sorted", np.argsort(values[sortidx])[::-1])]
    if sortidx:
        out.append(("-GT-sorted", np.argsort(values[0])[::-1]))
    return out


def _device_tensor(a, dtype, shape_tail, device, what):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if t.dtype != dtype:
        if dtype == torch.uint8:
            raise ValueError(f"{what} must be uint8, got {t.dtype}")
        t = t.to(dtype)
    t = t.to(device).contiguous()
    if t.ndim == len(shape_tail) + 2 and t.shape[1] == 1:              # masks as [N,1,64,64]
        t = t[:, 0]
    if tuple(t.shape[1:]) != shape_tail:
        raise ValueError(f"{what} must be [N, {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t.contiguous()


def upload_tables(values, n, device):
    atlas, ids, _ = labels(values, n)
    rows = plot_rows(values)
    return Tables(*(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (rows, ids, atlas)))


class Composer:
    """One video on the device: ``compose(f0, n)`` gives its frames f0 .. f0 + n - 1.  X uint8 [N,64,64,3]; masks fp32 [N,64,64] or
    [N,1,64,64], or None (-viscritic); values float64 [2, N]; perm None (time order) or the video's sorting.  Sources are numpy arrays
    or device tensors (shared between the videos of a run, like `tables`)."""

    def __init__(self, X, masks, values, perm=None, device="cuda", tables=None):
        if not torch.cuda.is_available():
            raise _lib.CgsError("the video frames are composed on the GPU (cgs_vis_compose); no GPU is visible and there is no CPU fallback")
        device = torch.device(device)
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._X = _device_tensor(X, torch.uint8, (TILE, TILE, 3), self.device, "X")
        self.n = len(self._X)
        self._masks = None if masks is None else _device_tensor(masks, torch.float32, (TILE, TILE), self.device, "masks")
        values = np.asarray(values.cpu() if torch.is_tensor(values) else values, dtype=np.float64)
        if self.n < 1 or values.shape != (VALUES, self.n) or (self._masks is not None and len(self._masks) != self.n):
            raise ValueError(f"X [{self.n},...], masks and values {values.shape} must describe the same N >= 1 frames")
        self._perm = None
        if perm is not None:
            perm = np.asarray(perm.cpu() if torch.is_tensor(perm) else perm).astype(np.int64)
            if perm.shape != (self.n,) or not np.array_equal(np.sort(perm), np.arange(self.n)):
                raise ValueError("perm must be a permutation of the N frames")
            self._perm = torch.from_numpy(perm.astype(np.int32)).to(self.device)
        self._tables = tables if tables is not None else upload_tables(values, self.n, self.device)
        self.plan = plan(self._masks is not None)
        self.frame_shape = (self.plan.height, self.plan.width, 3)

    def compose(self, f0, n, out=None, nontemporal=NONTEMPORAL):
        """Frames f0 .. f0 + n - 1 as device uint8 [n, H, 256, 3] (into `out` when given), on the current stream."""
        if not (0 <= f0 and 1 <= n and f0 + n <= self.n):
            raise ValueError(f"frames {f0}..{f0 + n} outside the {self.n} frames of this video")
        if out is None:
            out = torch.empty((n,) + self.frame_shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape[1:]) != self.frame_shape or len(out) < n \
                or out.device != self.device:
            raise ValueError(f"out must be contiguous uint8 [>={n}, {self.frame_shape}] on {self.device}")
        t = self._tables
        ptr = lambda x: None if x is None else x.data_ptr()
        with torch.cuda.device(self.device):
            _lib.call("cgs_vis_compose", self._X.data_ptr(), ptr(self._masks), ptr(self._perm), t.rows.data_ptr(), t.ids.data_ptr(),
                      t.atlas.data_ptr(), len(t.atlas), self.n, self.plan.R, f0, n, _lib.VIS_NONTEMPORAL if nontemporal else 0,
                      out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out[:n]


def _encode(path, comp, exe, chunk):
    proc = subprocess.Popen(video.ffmpeg_argv(exe, path, comp.plan.width, comp.plan.height, framerate=FRAMERATE), stdin=subprocess.PIPE)
    failure = None
    try:
        video.stream_frames(comp, proc.stdin, chunk)
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


def write_videos(resultdir, visname, sortidx, X, masks, values, device="cuda", ffmpeg=None, chunk=CHUNK):
    """Encodes {resultdir}{visname}.mp4, {visname}-pred-sorted.mp4 and, with sortidx != 0, {visname}-GT-sorted.mp4 (main.py:878-884)
    with ffmpeg at 4 frames/s; the sources and tables go to the device once.  Returns the paths written."""
    exe = ffmpeg or video.find_ffmpeg()
    if resultdir:
        os.makedirs(resultdir, exist_ok=True)
    first = Composer(X, masks, values, None, device)
    paths = []
    for suffix, perm in sortings(values, sortidx):
        comp = first if perm is None else Composer(first._X, first._masks, values, perm, first.device, tables=first._tables)
        paths.append(f"{resultdir}{visname}{suffix}.mp4")
        _encode(paths[-1], comp, exe, chunk)
    return paths
