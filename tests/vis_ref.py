"""Numpy + PIL restatement of the -viscritic / -vismasker frames (Handler.visualize's make_video, main.py:818-874) for the vis tests;
independent of cgs_amd.vis.  Labels are drawn by PIL itself (ImageDraw.text with its default font), as the reference does.

A frame of video position j shows source frame p = sorting[j] (p = j without a sorting):
  the RGB frame X[p]; with masks the frame times its mask under it, uint8(float32(x) * m) truncated;
  two plot strips of 32 x 64 (ground truth, prediction): column c holds value index k = j + c - 32 of the sorted sequence; when it
  exists, a white pixel sits at row 31 - floor(32 (x - min) / (1.01 max or 1)); column 32 keeps its red channel only;
  everything x4 nearest; then the index label str(p) at (230, H - 269) and the value labels str(round(value, 3)) at (1, 1 + 15 v)."""
import numpy as np

SCALE, PLOT_H, TILE = 4, 32, 64
CELL_W, CELL_H = 64, 16                      # the rectangle a label may cover (the tests blank it when PIL / FreeType differ)


def plot_rows(values):
    """make_plotbar's row of every value (main.py:31-37): float64 [N] -> int [N] in 0..31."""
    v = np.asarray(values, dtype=np.float64)
    v = v - v.min()
    top = v.max()
    v = v / ((top * 1.01) if top else 1)
    return PLOT_H - 1 - np.floor(v * PLOT_H).astype(int)


def label_positions(height):
    """(x, y) of the index label and the two value labels in a frame of `height` rows."""
    return [(TILE * SCALE - 26, height - 12 - 2 * PLOT_H * SCALE - 1), (1, 1), (1, 16)]


def label_strings(values, p):
    """The three strings of source frame p, in the order of label_positions."""
    return [str(int(p))] + [str(round(values[v, p].item(), 3)) for v in range(2)]


def canvas(X, masks, values, sorting=None):
    """uint8 [N, H, 256, 3]: the frames before any label is drawn."""
    X = np.asarray(X)
    n = len(X)
    values = np.asarray(values, dtype=np.float64)
    perm = np.arange(n) if sorting is None else np.asarray(sorting)
    tiles = [X.astype(np.float32)]
    if masks is not None:
        m = np.asarray(masks, dtype=np.float32).reshape(n, TILE, TILE, 1)
        tiles.append(X.astype(np.float32) * m)
    tiles = [t[perm] for t in tiles]
    rows = [plot_rows(values[v, perm]) for v in range(2)]
    out = []
    for j in range(n):
        strips = []
        for v in range(2):
            strip = np.zeros((PLOT_H, TILE, 3))
            for c in range(TILE):
                k = j + c - TILE // 2
                if 0 <= k < n:
                    strip[rows[v][k], c] = 255
            strip[:, TILE // 2] *= np.array((1, 0, 0))
            strips.append(strip)
        pic = np.concatenate([t[j] for t in tiles] + strips, axis=0)
        out.append(np.repeat(np.repeat(np.uint8(pic), SCALE, axis=0), SCALE, axis=1))
    return np.stack(out)


def frames(X, masks, values, sorting=None, strings=None):
    """uint8 [N, H, 256, 3]: the finished frames of one video, labels drawn by PIL.  strings[p] (optional) replaces the three label
    strings of source frame p."""
    from PIL import Image, ImageDraw
    values = np.asarray(values, dtype=np.float64)
    base = canvas(X, masks, values, sorting)
    perm = np.arange(len(base)) if sorting is None else np.asarray(sorting)
    out = []
    for j, pic in enumerate(base):
        img = Image.fromarray(pic)
        draw = ImageDraw.Draw(img)
        for (x, y), text in zip(label_positions(pic.shape[0]), strings[perm[j]] if strings is not None else label_strings(values, perm[j])):
            draw.text((x, y), text, fill=(255, 255, 255))
        out.append(np.array(img))
    return np.stack(out)


def blank_labels(a):
    """A copy of frames [N, H, 256, 3] with the three label rectangles zeroed."""
    a = np.array(a, copy=True)
    for x, y in label_positions(a.shape[1]):
        a[:, y:y + CELL_H, x:x + CELL_W] = 0
    return a


def blend(dst, alpha):
    """PIL's paste of white through a coverage mask, per byte: ((v >> 8) + v) >> 8 with v = dst (255 - a) + 255 a + 128."""
    d, a = np.asarray(dst, dtype=np.int64), np.asarray(alpha, dtype=np.int64)
    v = d * (255 - a) + 255 * a + 128
    return (((v >> 8) + v) >> 8).astype(np.uint8)
