"""The direct form of what cgs_objects_track_fill computes (include/cgs_hip.h), the checker of tests/test_objects_track_fill_host.py,
tests/test_gpu_objects_track_fill.py and tests/test_gpu_objects_track_fill_cli.py.  ``fill_plain`` is the rule as it is written, cell by
cell in Python integers: the spanning sets from loops over gap / prev, every cell walked back with objects_track_mc_ref.offset, the
claims, the numbering and the table rows from Python sets and sums.  ``fill`` is the same with objects_track_mc_ref.carried's whole
frames in int64 arrays (the host test holds the two against each other): the GPU tests fill thousands of frames.  Nothing of the
kernel's words, LDS staging, run detection or popcounts.  The tracks come from objects_track_gap_ref / objects_track_mc_ref (``tracked``)."""
import numpy as np

import objects_track_gap_ref as gap_ref
import objects_track_mc_ref as mc_ref
import objects_track_ref as base

FIELDS = ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "first")
TOTALS = ("objects", "cells", "dropped", "vanished")


def tracked(labels, bwd, milli, K=64, G=8):
    """The tracker's dict for a stack: objects_track_mc_ref.track with a field, objects_track_gap_ref.track without."""
    return gap_ref.track(labels, milli, K, G) if bwd is None else mc_ref.track(labels, bwd, milli, K, G)


def spanning(prev, gap, m, j, K, G):
    """S(m, j): the labels p in 1..K of frame a = m - j that a link (a -> f), f > m, f - a <= G + 1, starts from."""
    n, a, out = len(prev), m - j, set()
    for f in range(m + 1, min(n - 1, a + G + 1) + 1):
        for l in range(1, K + 1):
            if int(gap[f][l - 1]) == f - a and 1 <= int(prev[f][l - 1]) <= K:
                out.add(int(prev[f][l - 1]))
    return out


def _carried_cell(labels, bwd, a, m, y, x, K):
    h, w = labels.shape[1:]
    my, mx = (0, 0) if bwd is None else mc_ref.offset(bwd, a, m, y, x)
    sy, sx = y + my, x + mx
    if not (0 <= sy < h and 0 <= sx < w):
        return 0
    v = int(labels[a][sy][sx])
    return v if 1 <= v <= K else 0


def _finish(labels, track, K, frames):
    """frames: per frame (claims {(y, x): (j, p)}, vanished).  The numbering, the outputs and the totals."""
    n, h, w = labels.shape
    out = np.array(labels, dtype=np.int32)
    out_track, age = np.zeros((n, K), dtype=np.int32), np.zeros((n, K), dtype=np.int32)
    table, totals = np.zeros((n, K, len(FIELDS)), dtype=np.int32), np.zeros(4, dtype=np.int64)
    for m, (claims, vanished) in enumerate(frames):
        top = max(int(labels[m].max()), 0)
        for l in {int(v) for v in np.unique(labels[m]) if 1 <= v <= K}:
            out_track[m, l - 1] = track[m][l - 1]
        totals[3] += vanished
        for rank, (j, p) in enumerate(sorted(set(claims.values()))):
            l = top + rank + 1
            if l > K:
                totals[2] += 1
                continue
            cells = sorted(q for q, c in claims.items() if c == (j, p))
            for y, x in cells:
                out[m, y, x] = l
            out_track[m, l - 1], age[m, l - 1] = track[m - j][p - 1], j
            ys, xs = [q[0] for q in cells], [q[1] for q in cells]
            table[m, l - 1] = [len(cells), min(xs), min(ys), max(xs), max(ys), sum(xs), sum(ys), cells[0][0] * w + cells[0][1]]
            totals[0] += 1
            totals[1] += len(cells)
    return {"labels": out, "track": out_track, "age": age, "table": table, "totals": totals.astype(np.int32)}


def fill_plain(labels, bwd, prev, gap, track, K=64, G=8):
    """The definition: labels integer [n,h,w]; bwd integer [n - 1,8,8,2] (then 64 x 64) or None; prev, gap, track integer [n,K].
    Returns {"labels", "track", "age" int32, "table" int32 [n,K,8], "totals" int32 [4]}."""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    frames = []
    for m in range(n):
        claims, vanished = {}, 0
        for j in range(1, min(G, m) + 1):
            S = spanning(prev, gap, m, j, K, G)
            hit = set()
            for y in range(h):
                for x in range(w):
                    if S and int(labels[m][y][x]) <= 0 and (y, x) not in claims:
                        p = _carried_cell(labels, bwd, m - j, m, y, x, K)
                        if p in S:
                            claims[(y, x)] = (j, p)
                            hit.add(p)
            vanished += len(S - hit)
        frames.append((claims, vanished))
    return _finish(labels, track, K, frames)


def fill(labels, bwd, prev, gap, track, K=64, G=8):
    """``fill_plain`` with whole frames at a time."""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    frames = []
    for m in range(n):
        claims, vanished = {}, 0
        taken = np.asarray(labels[m]) > 0
        for j in range(1, min(G, m) + 1):
            S = spanning(prev, gap, m, j, K, G)
            if not S:
                continue
            W = base._clip(labels[m - j], K) if bwd is None else mc_ref.carried(labels[m - j], bwd, m - j, m, K)
            hit = ~taken & np.isin(W, sorted(S))
            for y, x in zip(*np.nonzero(hit)):
                claims[(int(y), int(x))] = (j, int(W[y, x]))
            taken = taken | hit
            vanished += len(S - {int(v) for v in np.unique(W[hit])})
        frames.append((claims, vanished))
    return _finish(labels, track, K, frames)


def paint(out_labels, out_track, K):
    """(track number per pixel int64 [n,h,w], rgb uint8 [n,h,w,3]): the tracker's colours over the filled labels."""
    out_labels, out_track = np.asarray(out_labels).astype(np.int64), np.asarray(out_track).astype(np.int64)
    inside = (out_labels >= 1) & (out_labels <= K)
    number = np.where(inside, np.take_along_axis(out_track, np.clip(out_labels - 1, 0, K - 1).reshape(len(out_labels), -1), axis=1)
                      .reshape(out_labels.shape), 0)
    hsh = ((number & 0xFFFFFFFF) * 2654435761) & 0xFFFFFFFF
    rgb = np.stack([64 + ((hsh >> (8 * c)) & 255) * 191 // 255 for c in range(3)], axis=-1)
    return number, np.where((number != 0)[..., None], rgb, 0).astype(np.uint8)
