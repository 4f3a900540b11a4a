"""The PNG sheets the training loops leave behind (main.py:203-226, 465-530): ``{model}/segment/e{epoch}_b{b}.png`` every --visevery
steps of the mask training -- a 7-row grid of 64 x 64 tiles, one column per image: two black rows that carry the value labels, then A, B,
replaced, injected and the mask Z -- and ``{model}/critic/e{epoch}_b{b}.png`` every 100th batch of the critic training: the batch's
frames side by side with the target and the prediction drawn over each.

The reference pulls A, B and Z to the host, mixes in numpy and encodes the PNG inline, which at this build's step rate would cost
several hundred steps per sheet.  Here the pixels of the segment sheet are made on the GPU from the tensors of the step that are
resident anyway (``cgs_sheet_compose``, csrc/sheet.hip), the sheet and the small label vectors are copied asynchronously into a
pinned slot of a ring, and a writer thread waits for the slot's event, draws the labels with PIL -- so they are PIL's own pixels, and
no string ever has to exist while the loop runs -- and encodes the file.  The loop never synchronises with the host for a sheet; it
waits only when every slot of the ring is still being encoded (back-pressure)."""
import contextlib
import queue
import threading

import numpy as np
import torch

from . import _lib, video

TILE, ROWS = 64, _lib.SHEET_ROWS
FONT_SIZE = 10                                       # main.py:70
LABEL_DY = 12                                        # `adder`, main.py:498
SEGMENT_LABELS = ("Y", "pred", "negpred", "replacevalue", "injectvalue")      # drawn in this order at y = 0, 12, 24, 36, 48
CRITIC_EVERY = 100                                   # main.py:204
COMPRESS_LEVEL = 1                                   # zlib level of the PNGs (lossless at every level): DESIGN.md section 4


def sheet_shape(n):
    return (ROWS * TILE, TILE * n, 3)


def segment_path(train_path, epoch, b_idx):
    return f"{train_path}e{epoch}_b{b_idx}.png"      # main.py:530 (and :226 for the critic's)


def wanted(visevery, b_idx):
    """main.py:466, with this build's own meaning of --visevery 0: no sheets (the reference divides by zero there)."""
    return visevery > 0 and b_idx % visevery == 0


def compose(A, B, Z, out=None):
    """The pixels of the segment sheet as device uint8 [7 * 64, 64 n, 3] (into `out` when given), on the current stream.
    A, B uint8 [n,64,64,3], Z fp32 [n,64,64] or [n,1,64,64], all contiguous on one GPU."""
    if not (torch.is_tensor(A) and torch.is_tensor(B) and torch.is_tensor(Z)):
        raise ValueError("A, B and Z must be device tensors")
    if not A.is_cuda:
        raise _lib.CgsError("the sheet is composed on the GPU (cgs_sheet_compose); the tensors are not on one and there is no CPU fallback")
    if Z.ndim == 4 and Z.shape[1] == 1:
        Z = Z[:, 0]
    n = len(A)
    for t, dtype, tail, what in ((A, torch.uint8, (TILE, TILE, 3), "A"), (B, torch.uint8, (TILE, TILE, 3), "B"),
                                 (Z, torch.float32, (TILE, TILE), "Z")):
        if t.dtype != dtype or tuple(t.shape) != (n,) + tail or not t.is_contiguous() or t.device != A.device:
            raise ValueError(f"{what} must be contiguous {dtype} [{n}, {', '.join(map(str, tail))}] on {A.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if not 1 <= n <= _lib.SHEET_MAX_N:
        raise ValueError(f"a sheet shows 1 .. {_lib.SHEET_MAX_N} images, got {n}")
    if out is None:
        out = torch.empty(sheet_shape(n), dtype=torch.uint8, device=A.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != sheet_shape(n) or not out.is_contiguous() or out.device != A.device:
        raise ValueError(f"out must be contiguous uint8 {sheet_shape(n)} on {A.device}")
    with torch.cuda.device(A.device):
        _lib.call("cgs_sheet_compose", A.data_ptr(), B.data_ptr(), Z.data_ptr(), n, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out


def label_text(value):
    return str(round(value, 3))


def draw_rows(img, rows, n, font):
    """draw.text of main.py:500-515 / 218-223 on a PIL image: per (y, values) row the value of image i at x = int(i * width / n),
    white, rows in the given order."""
    from PIL import ImageDraw
    draw = ImageDraw.Draw(img)
    for y, values in rows:
        for i, value in enumerate(values):
            draw.text((int(i * img.width / n), y), label_text(value), fill=(255, 255, 255), font=font)
    return img


def segment_rows(Y, pred, negpred, replacevalue, injectvalue=None):
    """[(y, values)] of the segment sheet: Y, pred, negpred, replacevalue and, with inject, injectvalue, 12 pixels apart."""
    rows = [Y, pred, negpred, replacevalue] + ([injectvalue] if injectvalue is not None else [])
    return [(LABEL_DY * k, list(v)) for k, v in enumerate(rows)]


def critic_rows(Y, pred, height=TILE):
    return [(1, list(Y)), (int(1 + height / 2), list(pred))]


def save_png(img, path):
    img.save(path, format="PNG", compress_level=COMPRESS_LEVEL)


class _Slot:
    def __init__(self, k):
        self.k, self.pixels, self.labels = k, None, None

    def fit(self, shape, n, pin):
        """Host buffers of this slot for a sheet of `shape` (None: no pixels come from the device) and four label rows of n values,
        pinned when the sources are on a GPU."""
        stale = self.pixels is None or tuple(self.pixels.shape) != tuple(shape or ()) or self.pixels.is_pinned() != pin
        if shape is not None and stale:
            self.pixels = torch.empty(shape, dtype=torch.uint8, pin_memory=pin)
        if self.labels is None or self.labels.shape[1] != n or self.labels.is_pinned() != pin:
            self.labels = torch.empty((len(SEGMENT_LABELS) - 1, n), dtype=torch.float32, pin_memory=pin)


class SheetWriter:
    """A ring of `depth` host slots and one writer thread.  submit_* enqueue the device work on the caller's stream, hand the slot to
    the thread and return without synchronising; they block only while every slot is still being written.  close() drains the ring
    and re-raises the first exception the thread met.  compose / encode can be replaced (tests)."""

    def __init__(self, depth=4, compose=compose, encode=save_png, font=None):
        if depth < 1:
            raise ValueError("depth must be at least 1")
        self.depth = depth
        self._compose, self._encode = compose, encode
        self._font = font
        self._free, self._todo = queue.Queue(), queue.Queue()
        for k in range(depth):
            self._free.put(_Slot(k))
        self._dev = None                      # the composed sheet on the device; stream order keeps copy k ahead of compose k + 1
        self._err, self._closed = [], False
        self.written, self.encode_s = [], 0.0
        self._thread = threading.Thread(target=self._run, name="sheet-writer", daemon=True)
        self._thread.start()

    # ---- the thread
    def _run(self):
        import time
        from PIL import Image
        while True:
            job = self._todo.get()
            if job is None:
                return
            slot, event, path, pixels, rows, n = job
            try:
                if not self._err:
                    if event is not None:
                        event.synchronize()
                    t0 = time.perf_counter()
                    if self._font is None:
                        self._font = video.resolve_font(FONT_SIZE)[0]
                    img = draw_rows(Image.fromarray(pixels()), rows(), n, self._font)
                    self._encode(img, path)            # (the file is closed when this returns)
                    self.encode_s += time.perf_counter() - t0
                    self.written.append(path)
            except BaseException as e:
                self._err.append(e)
            finally:
                self._free.put(slot)

    def _take(self):
        if self._closed:
            raise RuntimeError("the SheetWriter is closed")
        return self._free.get()               # back-pressure: blocks while all slots are with the thread

    @staticmethod
    def _event(device):
        if device.type != "cuda":
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        return ev

    # ---- the two sheets
    def submit_segment(self, path, A, B, Z, labels_host, labels_dev, inject):
        """The sheet of one mask-training step.  A, B, Z: the step's device tensors; labels_host: Y (host floats, as the reference's
        float64 targets); labels_dev: (pred, negpred, replacevalue, injectvalue) fp32 [n] device tensors (injectvalue unused without
        inject).  Everything is enqueued on the current stream; the sources may be overwritten by later work on that stream."""
        n = len(A)
        labels_dev = list(labels_dev)[:4 if inject else 3]
        if len(labels_host) != n or any(v.numel() != n for v in labels_dev):
            raise ValueError(f"every label row must hold {n} values")
        slot = self._take()
        try:
            device = A.device
            slot.fit(sheet_shape(n), n, device.type == "cuda")
            with torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext():
                if self._dev is None or tuple(self._dev.shape) != sheet_shape(n) or self._dev.device != device:
                    self._dev = torch.empty(sheet_shape(n), dtype=torch.uint8, device=device)
                sheet = self._compose(A, B, Z, out=self._dev)
                slot.pixels.copy_(sheet, non_blocking=True)
                for k, v in enumerate(labels_dev):
                    slot.labels[k].copy_(v.reshape(-1), non_blocking=True)
                event = self._event(device)
        except BaseException:
            self._free.put(slot)
            raise
        Y, rows_dev = [float(v) for v in labels_host], len(labels_dev)
        rows = lambda: segment_rows(Y, *(slot.labels[k].tolist() for k in range(rows_dev)))
        self._todo.put((slot, event, path, lambda: slot.pixels.numpy(), rows, n))

    def submit_critic(self, path, X_host_u8, y_f32, pred_dev):
        """The sheet of one critic-training batch: the uint8 frames as the host holds them (not modified afterwards), the targets
        (fp32 values on the host) and the device vector of predictions, copied asynchronously."""
        X = X_host_u8.numpy() if torch.is_tensor(X_host_u8) else np.asarray(X_host_u8)
        n = len(X)
        if X.dtype != np.uint8 or X.ndim != 4 or X.shape[3] != 3 or n < 1 or pred_dev.numel() != n or len(y_f32) != n:
            raise ValueError("the critic sheet takes uint8 frames [n,h,w,3], n targets and n predictions")
        slot = self._take()
        try:
            device = pred_dev.device
            slot.fit(None, n, device.type == "cuda")
            with torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext():
                slot.labels[0].copy_(pred_dev.reshape(-1), non_blocking=True)
                event = self._event(device)
        except BaseException:
            self._free.put(slot)
            raise
        Y = y_f32.tolist() if hasattr(y_f32, "tolist") else [float(v) for v in y_f32]
        rows = lambda: critic_rows(Y, slot.labels[0].tolist(), X.shape[1])
        self._todo.put((slot, event, path, lambda: np.concatenate(X, axis=1), rows, n))

    def close(self):
        """Waits until every submitted sheet is on disk (or failed), stops the thread and raises the first exception it met.
        A second call does nothing."""
        if self._closed:
            return
        self._closed = True
        self._todo.put(None)
        self._thread.join()
        if self._err:
            raise self._err[0]

