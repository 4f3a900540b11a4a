"""The rule of cgs_objects_ablate / cgs_objects_select and of objects.value's chunking (the header comment in include/cgs_hip.h and the
docstrings of cgs_amd.objects) in Python integers and numpy: no torch, no GPU, written from the rule and not from the kernels.  The
ablated set is made the other way round from the kernel: every labelled cell stamps its clipped square into its object's set."""
import numpy as np

SIDE, K_MAX = 64, 64


def mean_fill(frame, labels):
    """(r, g, b) of the mean fill of one frame: c = (2 S + N) // (2 N) over the cells of label 0, over all cells when there are none."""
    bg = np.asarray(labels) == 0
    if not bg.any():
        bg = np.ones_like(bg)
    N = int(bg.sum())
    return tuple((2 * int(np.asarray(frame)[..., ch][bg].astype(np.int64).sum()) + N) // (2 * N) for ch in range(3))


def row_counts(kept, K=K_MAX):
    return [min(max(int(k), 0), K) for k in kept]


def ablate(frames, labels, kept, fill, grow, K=K_MAX, frames_range=None):
    """frames uint8 [n,64,64,3], labels int [n,64,64], kept [n]; fill: "mean", (r, g, b) or a uint8 array [64,64,3].
    Returns (images uint8 [rows,64,64,3], row_frame int32 [rows], row_label int32 [rows], offsets int32 [n + 1]) for the frames of
    frames_range (all of them by default); offsets are always the whole stack's."""
    frames, labels = np.asarray(frames), np.asarray(labels)
    n, R = len(frames), int(grow)
    counts = row_counts(kept, K)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    f0, f1 = (0, n) if frames_range is None else frames_range
    images, row_frame, row_label = [], [], []
    for f in range(f0, f1):
        if isinstance(fill, str):
            assert fill == "mean"
            F = np.empty((SIDE, SIDE, 3), dtype=np.uint8)
            F[:] = mean_fill(frames[f], labels[f])
        elif isinstance(fill, np.ndarray):
            assert fill.shape == (SIDE, SIDE, 3) and fill.dtype == np.uint8
            F = fill
        else:
            F = np.empty((SIDE, SIDE, 3), dtype=np.uint8)
            F[:] = tuple(int(v) for v in fill)
        A = np.zeros((counts[f] + 1, SIDE, SIDE), dtype=bool)
        for y in range(SIDE):
            for x in range(SIDE):
                k = int(labels[f, y, x])
                if 1 <= k <= counts[f]:
                    A[k, max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = True
        for k in range(1, counts[f] + 1):
            img = frames[f].copy()
            img[A[k]] = F[A[k]]
            images.append(img)
            row_frame.append(f)
            row_label.append(k)
    images = np.stack(images) if images else np.zeros((0, SIDE, SIDE, 3), dtype=np.uint8)
    return images, np.array(row_frame, dtype=np.int32), np.array(row_label, dtype=np.int32), offsets


def chunks(rows, chunk_rows):
    """[(f0, f1, rows)]: consecutive ranges of frames, a frame joins the range while the row total stays at most chunk_rows; ranges
    without rows are left out."""
    out, f0, total = [], 0, 0
    for f, r in enumerate(rows):
        r = int(r)
        assert r <= chunk_rows
        if total + r > chunk_rows:
            out.append((f0, f, total))
            f0, total = f, 0
        total += r
    out.append((f0, len(rows), total))
    return [c for c in out if c[2] > 0]


def selected(drop, kept, V, K=K_MAX):
    """The keep table of a threshold: drop >= V in float32 for the objects that have a row; a NaN is not selected."""
    drop = np.asarray(drop, dtype=np.float32)
    keep = np.zeros((len(kept), K), dtype=bool)
    for f, c in enumerate(row_counts(kept, K)):
        for k in range(c):
            keep[f, k] = bool(drop[f, k] >= np.float32(V))
    return keep


def select(labels, table, kept, keep, K=K_MAX):
    """labels int [n,h,w], table int [n,>=K,8], kept [n], keep [n,K].  Returns (labels, table [n,K,8], kept', mask uint8, unscored)."""
    labels, table, keep = np.asarray(labels), np.asarray(table), np.asarray(keep)
    n = len(labels)
    out, out_table = np.zeros_like(labels, dtype=np.int32), np.zeros((n, K, 8), dtype=np.int32)
    out_kept, unscored = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for f in range(n):
        have = max(int(kept[f]), 0)
        limit, new, count = min(have, K), {}, 0
        for k in range(1, limit + 1):
            if keep[f, k - 1]:
                count += 1
                new[k] = count
                out_table[f, count - 1] = table[f, k - 1]
        out_kept[f], unscored[f] = count, have - limit
        for y in range(labels.shape[1]):
            for x in range(labels.shape[2]):
                out[f, y, x] = new.get(int(labels[f, y, x]), 0)
    return out, out_table, out_kept, (out != 0).astype(np.uint8), unscored
