"""Numpy restatement of the reference's evaluation-video frames (main.py:1028-1083) for the video tests; independent of cgs_amd.video.

The two layouts the reference can render are written out below as tables (main.py:1028-1035 reorder the columns, main.py:1050-1051
colour-code the allM entries 0, 2, 3, 5, 6 and fill every other one with a constant 0.1 tile).  Each tile is built in float64 as the
reference holds it (RGB / 255, masks 0 / 1, fp32 maps promoted, codes TP (0,1,0) FN (1,0,0) FP (.5,.5,.5) TN 0), quantised with
uint8(255 v) truncation, and shown x3 nearest between the title and legend bands."""
import numpy as np

# column tables: row 1 (grey tiles), row 2 ("code:<name>" = colour-coded against Y, "const" = the 0.1 tile), titles by allM position
LAYOUTS = {
    False: {"row1": ["X", "Y", "hardM", "M", "salhardM"],
            "row2": ["X", "code:Y", "code:hardM", "const", "const"],
            "titles": [0, 1, 3, 2, 5], "h_top": 120, "h_bottom": 120},
    True: {"row1": ["X", "Y", "crfM", "hardM", "M", "salcrfM", "salhardM", "salM"],
           "row2": ["X", "code:Y", "code:crfM", "code:hardM", "const", "code:salcrfM", "code:salhardM", "const"],
           "titles": [0, 1, 4, 3, 2, 7, 6, 5], "h_top": 120, "h_bottom": 60},
}


def _grey(a):
    """[n,64,64] or [n,64,64,3] source -> float64 [n,64,64,3] as the reference concatenates it."""
    a = np.asarray(a)
    if a.ndim == 4 and a.shape[-1] == 3:
        return a / 255.0
    v = a.astype(np.float64)
    return np.repeat(v[..., None], 3, axis=-1)


def _code(y, m):
    y, m = np.asarray(y).astype(bool), np.asarray(m).astype(bool)
    out = np.zeros(y.shape + (3,))
    out[y & m] = (0.0, 1.0, 0.0)
    out[y & ~m] = (1.0, 0.0, 0.0)
    out[~y & m] = (0.5, 0.5, 0.5)
    return out


def middle(sources, crf):
    """uint8 [n, 2 * 192, 192 cols, 3]: the two tile rows, quantised and upscaled x3 nearest.  sources: name -> [n,64,64] stacks (X
    uint8 [n,64,64,3]; Y / masks bool or 0/1; M fp32; salM fp64)."""
    lay = LAYOUTS[crf]
    n = len(sources["X"])
    row1 = [_grey(sources[nm]) for nm in lay["row1"]]
    row2 = []
    for nm in lay["row2"]:
        if nm == "const":
            row2.append(np.full((n, 64, 64, 3), 0.1))
        elif nm.startswith("code:"):
            row2.append(_code(sources["Y"], sources[nm[5:]]))
        else:
            row2.append(_grey(sources[nm]))
    tiles = np.concatenate([np.concatenate(row1, axis=2), np.concatenate(row2, axis=2)], axis=1)
    q = (tiles * 255).astype(np.uint8)
    return np.repeat(np.repeat(q, 3, axis=1), 3, axis=2)


def frames(sources, crf, top, bottom):
    """Whole frames uint8 [n, H, W, 3] with the given band images on top and bottom."""
    mid = middle(sources, crf)
    n = len(mid)
    return np.concatenate([np.broadcast_to(top, (n,) + top.shape), mid, np.broadcast_to(bottom, (n,) + bottom.shape)], axis=1)
