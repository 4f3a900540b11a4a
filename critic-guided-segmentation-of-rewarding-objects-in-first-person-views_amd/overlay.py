"""The frames of the overlay video of ``-process --source-video`` (csrc/overlay.hip): ``compose`` tints every frame by its upsampled mask
(``fit.up``'s grey byte), draws the outline of the thresholded mask in the tint colour and lays the panels side by side -- the overlay
alone, frame | overlay, or frame | overlay | grey.  Integers throughout, so a result is reproducible bit for bit.  Runs on the GPU only;
``parse_color`` / ``to_alpha256`` / ``panels`` / ``check_outline`` are the pure host helpers.

The outline is the set of on pixels within Manhattan distance t - 1 of an off pixel, where a pixel OUTSIDE the frame counts as on: a
mask that the frame cuts draws no line along the frame's edge.  boundary.py scores with the opposite convention (there the frame's edge
belongs to an object's outline); a drawn line along the border of the picture would only be noise.

``compose_tracks`` (csrc/overlay_tracks.hip, ``--overlay-tracks``) is ``compose`` with a colour per tracked object, the objects' bounding
boxes and their track numbers; ``FONT`` holds the digits it draws, ``check_boxes`` / ``scale`` are its pure host helpers."""
import numpy as np
import torch

from . import _lib
from .fit import _frames, _need_gpu

LAYOUTS = {"overlay": _lib.OVERLAY_ONLY, "side": _lib.OVERLAY_SIDE, "triple": _lib.OVERLAY_TRIPLE}
MAX_OUTLINE = _lib.OVERLAY_MAX_OUTLINE
COLOR, ALPHA, OUTLINE, LAYOUT = (0, 255, 0), 0.5, 1, "overlay"
NONTEMPORAL = True
MAX_BOXES, MAX_TRACK_OBJECTS, BOXES = _lib.OVERLAY_MAX_BOXES, _lib.OVERLAY_MAX_TRACK_OBJECTS, 1


def _glyphs(*rows):
    return np.array([[int(r, 2) for r in g.split()] for g in rows], dtype=np.uint8)


# the digits 0..9 as 5 x 7 glyphs, a byte per glyph row from the top, bit 4 the leftmost pixel: the only copy of their shapes (the kernel
# reads them from this array)
FONT = _glyphs("01110 10001 10011 10101 11001 10001 01110", "00100 01100 00100 00100 00100 00100 01110",
               "01110 10001 00001 00010 00100 01000 11111", "11111 00010 00100 00010 00001 10001 01110",
               "00010 00110 01010 10010 11111 00010 00010", "11111 10000 11110 00001 00001 10001 01110",
               "00110 01000 10000 11110 10001 10001 01110", "11111 00001 00010 00100 01000 01000 01000",
               "01110 10001 10001 01110 10001 10001 01110", "01110 10001 10001 01111 00001 00010 01100")
FONT.setflags(write=False)
_font_on_device = {}            # (device, the font's bytes) -> its device copy: an upload per call would synchronise the stream


def panels(layout):
    """The number of panels of a layout name; ValueError for an unknown one."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {', '.join(LAYOUTS)}")
    return LAYOUTS[layout]


def parse_color(text):
    """"R,G,B" (or three numbers) -> (r, g, b), whole numbers 0..255; ValueError otherwise."""
    parts = text.split(",") if isinstance(text, str) else list(text) if isinstance(text, (tuple, list)) else None
    if parts is None or len(parts) != 3:
        raise ValueError(f"colour {text!r}: three integers R,G,B")
    out = []
    for p in parts:
        try:
            v = int(p.strip(), 10) if isinstance(p, str) else p
        except ValueError:
            raise ValueError(f"colour {text!r}: three integers R,G,B") from None
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255:
            raise ValueError(f"colour {text!r}: each of R,G,B is an integer 0..255")
        out.append(int(v))
    return tuple(out)


def to_alpha256(alpha):
    """An opacity in [0, 1] as the integer round(alpha * 256) in 0..256; ValueError outside the range."""
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"alpha must be a number, got {alpha!r}") from None
    if not 0.0 <= a <= 1.0:                      # (a NaN fails both comparisons)
        raise ValueError(f"alpha = {alpha!r}: an opacity is between 0 and 1")
    return int(round(a * 256))


def check_outline(t, name="outline"):
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t <= MAX_OUTLINE:
        raise ValueError(f"{name} = {t!r}: a thickness is an integer 0..{MAX_OUTLINE} pixels")
    return int(t)


def check_boxes(b, name="boxes"):
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b <= MAX_BOXES:
        raise ValueError(f"{name} = {b!r}: a box's thickness is an integer 0..{MAX_BOXES} pixels (0: no boxes, no numbers)")
    return int(b)


def scale(h, w):
    """The size of a font pixel on frames of h x w: max(1, min(h, w) // 256)."""
    return max(1, min(int(h), int(w)) // 256)


def _prepare(what, guide, grey, hard, color, alpha256, outline, layout, out, more=None):
    """What ``compose`` and ``compose_tracks`` do before the call: the checks of the arguments both take, the GPU check under the name
    `what`, contiguous inputs (a bool `hard` viewed as uint8) and `out`.  more(n): the caller's checks of its own tensors, run after those
    of grey and hard; it returns the tensors that the GPU check names after grey and those it names last.  Returns guide, grey, hard, out,
    (n, h, w), (r, g, b), outline and k."""
    n, h, w = _frames("guide", guide)
    k = panels(layout)
    rgb = parse_color(color)
    outline = check_outline(outline)
    if isinstance(alpha256, bool) or not isinstance(alpha256, (int, np.integer)) or not 0 <= alpha256 <= 256:
        raise ValueError(f"alpha256 = {alpha256!r}: an integer 0..256 (overlay.to_alpha256 maps an opacity to it)")
    if not isinstance(grey, torch.Tensor) or grey.dtype != torch.uint8 or tuple(grey.shape) != (n, h, w):
        raise ValueError(f"grey must be a uint8 tensor [{n},{h},{w}], got "
                         + (f"{grey.dtype} {tuple(grey.shape)}" if isinstance(grey, torch.Tensor) else type(grey).__name__))
    if hard is not None and (not isinstance(hard, torch.Tensor) or hard.dtype not in (torch.uint8, torch.bool) or tuple(hard.shape) != (n, h, w)):
        raise ValueError(f"hard must be a uint8 or bool tensor [{n},{h},{w}] or None, got "
                         + (f"{hard.dtype} {tuple(hard.shape)}" if isinstance(hard, torch.Tensor) else type(hard).__name__))
    own, own_last = more(n) if more is not None else ((), ())
    if n > 65535:
        raise ValueError(f"guide: at most 65535 frames a call, got {n}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_contiguous()
                            or tuple(out.shape) != (n, h, k * w, 3)):
        raise ValueError(f"out must be a contiguous uint8 tensor [{n},{h},{k * w},3]")
    _need_gpu(what, guide, grey, *own, *((hard,) if hard is not None else ()), *((out,) if out is not None else ()), *own_last)
    guide, grey = guide.contiguous(), grey.contiguous()
    if hard is not None:
        hard = hard.contiguous()
        if hard.dtype == torch.bool:
            hard = hard.view(torch.uint8)
    if out is None:
        out = torch.empty((n, h, k * w, 3), dtype=torch.uint8, device=guide.device)
    return guide, grey, hard, out, (n, h, w), rgb, outline, k


def compose(guide, grey, hard=None, color=COLOR, alpha256=128, outline=OUTLINE, layout=LAYOUT, out=None, nontemporal=NONTEMPORAL):
    """guide: device tensor uint8 [n,H,W,3], the frames, 64 <= H, W <= 4096.  grey: uint8 [n,H,W] (fit.up's grey).  hard: uint8 / bool
    [n,H,W], zero / non-zero, or None (no outline).  color (r, g, b); alpha256: the opacity as an integer 0..256; outline: thickness 0..4;
    layout "overlay", "side" or "triple" (k = 1, 2, 3 panels).  Returns uint8 [n,H,k W,3] (`out` when given) on the inputs' device:
    overlay_c = (frame_c (65280 - q) + color_c q + 32640) // 65280 with q = alpha256 grey, outline pixels the colour itself; "side" puts
    the frame to its left, "triple" also the grey byte as RGB to its right.  No CPU path: raises CgsError without a GPU."""
    guide, grey, hard, out, (n, h, w), (r, g, b), outline, k = _prepare("overlay.compose (cgs_overlay_compose)", guide, grey, hard, color,
                                                                        alpha256, outline, layout, out)
    with torch.cuda.device(guide.device):
        _lib.call("cgs_overlay_compose", guide.data_ptr(), grey.data_ptr(), hard.data_ptr() if hard is not None else None, n, h, w, r, g, b,
                  int(alpha256), outline, k, _lib.OVERLAY_NONTEMPORAL if nontemporal else 0, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out


def _device_font(font, device):
    if isinstance(font, torch.Tensor):
        if font.dtype != torch.uint8 or tuple(font.shape) != FONT.shape:
            raise ValueError(f"font must be uint8 {list(FONT.shape)}, got {font.dtype} {tuple(font.shape)}")
        return font.contiguous()
    font = np.asarray(font)
    if font.dtype != np.uint8 or font.shape != FONT.shape:
        raise ValueError(f"font must be uint8 {list(FONT.shape)}, got {font.dtype} {font.shape}")
    key = (str(device), font.tobytes())
    if key not in _font_on_device:
        _font_on_device[key] = torch.from_numpy(np.array(font)).to(device)
    return _font_on_device[key]


def compose_tracks(guide, grey, hard, labels, ids, table, font=FONT, color=COLOR, alpha256=128, outline=OUTLINE, boxes=BOXES, layout=LAYOUT,
                   out=None, nontemporal=NONTEMPORAL, age=None):
    """``compose`` with the tracked objects drawn: guide, grey, hard, color, alpha256, outline, layout, out, nontemporal as there (hard may
    be None).  labels: int32 [n,64,64], ``objects.label``'s labels of the 64 x 64 masks; ids: int32 [n,K], K <= 64, the track number of
    every object (``objects.TrackStream.push``; 0: none); table: int32 [n,K,8], ``objects.label``'s table (area and bounding box are
    read; a row with area 0 is no object); font: uint8 [10,7] (array or device tensor), a byte per glyph row, bit 4 leftmost; boxes: the
    thickness of a bounding box 0..4 (0: no boxes and no numbers).  Returns uint8 [n,H,k W,3].
    A pixel takes the colour of its object's track, 64 + ((t 2654435761 mod 2^32) >> 8 c & 255) 191 // 255 (``objects.track``'s rgb),
    its object being the label of its home cell (fit.home_cells) or, when that is 0, of the nearest labelled cell of the 5 x 5 cells
    around it; `color` where there is none.  Every object with a track gets its box on the cells' pixel tiling and, at the box's top left
    corner, a plate with the track number in digits scale(H, W) font pixels big.  Plates lie over borders, borders over the outline.
    age: None, or int32 [n,K], ``objects.fill``'s age: an object with age > 0 is a carried one and is drawn hatched
    (cgs_overlay_compose_tracks_carried) -- on the stripes ((x + y) // (2 scale(H, W))) & 1 == 0 as above, between them without tint and
    without its box's border; plate, digits and outline stay whole.  All ages <= 0 give the bytes of age=None.
    Integers throughout (include/cgs_hip.h has every formula).  No CPU path: raises CgsError without a GPU."""
    boxes = check_boxes(boxes)

    def tracked(n):
        for name, t in (("labels", labels), ("ids", ids), ("table", table)) + ((("age", age),) if age is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise ValueError(f"{name} must be an int32 tensor, got " + (str(t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
        side = _lib.FIT_SIDE
        if tuple(labels.shape) != (n, side, side):
            raise ValueError(f"labels must be [{n},{side},{side}] for {n} frames, got {tuple(labels.shape)}")
        if ids.dim() != 2 or ids.shape[0] != n or not 1 <= ids.shape[1] <= MAX_TRACK_OBJECTS:
            raise ValueError(f"ids must be [{n},K] with K in 1..{MAX_TRACK_OBJECTS}, got {tuple(ids.shape)}")
        if tuple(table.shape) != (n, ids.shape[1], _lib.OBJ_FIELDS):
            raise ValueError(f"table must be [{n},{ids.shape[1]},{_lib.OBJ_FIELDS}] beside ids {tuple(ids.shape)}, got {tuple(table.shape)}")
        if age is not None and tuple(age.shape) != tuple(ids.shape):
            raise ValueError(f"age must be [{n},{ids.shape[1]}] as ids, got {tuple(age.shape)}")
        return (labels, ids, table) + ((age,) if age is not None else ()), ((font,) if isinstance(font, torch.Tensor) else ())

    entry = "cgs_overlay_compose_tracks" if age is None else "cgs_overlay_compose_tracks_carried"
    guide, grey, hard, out, (n, h, w), (r, g, b), outline, k = _prepare(f"overlay.compose_tracks ({entry})", guide, grey,
                                                                        hard, color, alpha256, outline, layout, out, more=tracked)
    K = int(ids.shape[1])
    font = _device_font(font, guide.device)
    labels, ids, table = labels.contiguous(), ids.contiguous(), table.contiguous()
    with torch.cuda.device(guide.device):
        if age is not None:
            age = age.contiguous()
            _lib.call(entry, guide.data_ptr(), grey.data_ptr(), hard.data_ptr() if hard is not None else None, labels.data_ptr(),
                      ids.data_ptr(), table.data_ptr(), age.data_ptr(), font.data_ptr(), n, h, w, K, r, g, b, int(alpha256), outline, boxes, k,
                      _lib.OVERLAY_NONTEMPORAL if nontemporal else 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return out
        _lib.call("cgs_overlay_compose_tracks", guide.data_ptr(), grey.data_ptr(), hard.data_ptr() if hard is not None else None,
                  labels.data_ptr(), ids.data_ptr(), table.data_ptr(), font.data_ptr(), n, h, w, K, r, g, b, int(alpha256), outline, boxes, k,
                  _lib.OVERLAY_NONTEMPORAL if nontemporal else 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out
