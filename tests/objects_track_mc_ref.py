"""The direct form of what cgs_objects_track_mc computes (include/cgs_hip.h), the checker of tests/test_objects_track_mc_host.py and
tests/test_gpu_objects_track_mc.py: a plain walk over the frame pairs in integers.  For a pair (a, f) every cell of frame f is
walked back along the block vectors one step at a time, frame a's label is read where the walk ends (0 outside the grid), and the
carried map goes to objects_track_ref.links in place of frame a: its pair counts then hold the carried areas.  The level order, the
masking of closed ends and the walk over the frames for numbers, tables and spans are objects_track_gap_ref's, written out again with
the carried maps.  Nothing of the kernels' LDS staging, ballots, 64-bit masks or `best` rows."""
import numpy as np

import objects_track_gap_ref as gap_ref
import objects_track_ref as base

FIELDS = base.FIELDS
SIDE, BLOCK = 64, 8


def _clamp(v):
    return 0 if v < 0 else SIDE - 1 if v > SIDE - 1 else v


def offset(bwd, a, f, y, x):
    """m_g of cell (y, x) of frame f walked back to frame a, g = f - a: (my, mx) in Python ints."""
    my = mx = 0
    for j in range(f - a):
        cy, cx = _clamp(y + my), _clamp(x + mx)
        v = bwd[f - j - 1][cy >> 3][cx >> 3]
        my += int(v[0])
        mx += int(v[1])
    return my, mx


def carried_plain(frame_a, bwd, a, f, K):
    """W_{a -> f}: int64 [64,64], frame a's labels (outside 1..K read as 0) gathered along the path of every cell of frame f, cell by
    cell with ``offset``: the definition."""
    src = base._clip(frame_a, K)
    out = np.zeros((SIDE, SIDE), dtype=np.int64)
    for y in range(SIDE):
        for x in range(SIDE):
            my, mx = offset(bwd, a, f, y, x)
            sy, sx = y + my, x + mx
            if 0 <= sy < SIDE and 0 <= sx < SIDE:
                out[y, x] = src[sy, sx]
    return out


def carried(frame_a, bwd, a, f, K):
    """``carried_plain`` with all cells walked at once in int64 arrays (the host test holds the two against each other): the tests walk
    thousands of frame pairs."""
    bwd = np.asarray(bwd).astype(np.int64)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    my, mx = np.zeros_like(y), np.zeros_like(x)
    for j in range(f - a):
        v = bwd[f - j - 1][np.clip(y + my, 0, SIDE - 1) >> 3, np.clip(x + mx, 0, SIDE - 1) >> 3]
        my, mx = my + v[..., 0], mx + v[..., 1]
    sy, sx = y + my, x + mx
    inside = (sy >= 0) & (sy < SIDE) & (sx >= 0) & (sx < SIDE)
    return np.where(inside, base._clip(frame_a, K)[np.clip(sy, 0, SIDE - 1), np.clip(sx, 0, SIDE - 1)], 0)


def all_links(labels, bwd, milli, K, G):
    """labels integer [n,64,64], bwd integer [n - 1,8,8,2] -> {(f, q): (p, g, inter, union)}: object q of frame f continues object p
    of frame f - g; union holds the carried area of p."""
    labels = np.asarray(labels)
    bwd = np.asarray(bwd).astype(np.int64).reshape(-1, SIDE // BLOCK, SIDE // BLOCK, 2)
    n = labels.shape[0]
    assert labels.shape[1:] == (SIDE, SIDE) and len(bwd) == max(n - 1, 0)
    objs = [gap_ref._objects(labels[f], K) for f in range(n)]
    has_next, has_prev, out = [set() for _ in range(n)], [set() for _ in range(n)], {}
    for g in range(1, G + 2):
        made = []
        for f in range(g, n):                                               # the f's of a level do not see each other's links
            if g == 1:
                a, b = labels[f - 1], labels[f]
            else:
                a, b = gap_ref._masked(labels[f - g], objs[f - g] - has_next[f - g]), gap_ref._masked(labels[f], objs[f] - has_prev[f])
            if g > 1 and (not (objs[f - g] - has_next[f - g]) or not (objs[f] - has_prev[f])):
                continue                                                     # (nothing open: nothing to carry)
            for q, (p, inter, union) in base.links(carried(a, bwd, f - g, f, K), b, milli, K).items():
                made.append((f, q, p, inter, union))
        for f, q, p, inter, union in made:
            assert q not in has_prev[f] and p not in has_next[f - g]
            has_prev[f].add(q)
            has_next[f - g].add(p)
            out[(f, q)] = (p, g, inter, union)
    return out


def track(labels, bwd, milli, K=64, G=0, max_tracks=None, want_paint=False):
    """objects_track_gap_ref.track's dict (prev, gap, track, totals, gap_links, table, extra, heads, spans, track_labels) with the links
    of ``all_links``; the areas of the table are the objects' own."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    max_tracks = n * K if max_tracks is None else max_tracks
    link = all_links(labels, bwd, milli, K, G)
    prev, gap, trk = (np.zeros((n, K), dtype=np.int32) for _ in range(3))
    rows, heads, last, n_objects = [], [], [], 0
    gap_links = np.zeros(G + 1, dtype=np.int32)
    for f in range(n):
        area = np.bincount(base._clip(labels[f], K).ravel(), minlength=65)
        for l in range(1, K + 1):                                            # by frame, then by label: the numbering order
            if area[l] == 0:
                continue
            n_objects += 1
            a = int(area[l])
            if (f, l) in link:
                p, g, inter, union = link[(f, l)]
                prev[f, l - 1], gap[f, l - 1], t = p, g, int(trk[f - g, p - 1])
                assert t > 0
                row = rows[t - 1]
                row["length"] += 1
                row["area_sum"] += a
                row["area_min"], row["area_max"] = min(row["area_min"], a), max(row["area_max"], a)
                row["inter_sum"] += inter
                row["union_sum"] += union
                row["bridges"] += g > 1
                row["missed"] += g - 1
                gap_links[g - 1] += 1
                last[t - 1] = f
            else:
                heads.append((f, l))
                rows.append({"first_frame": f, "first_label": l, "length": 1, "area_sum": a, "area_min": a, "area_max": a, "inter_sum": 0,
                             "union_sum": 0, "bridges": 0, "missed": 0})
                last.append(f)
                t = len(rows)
            trk[f, l - 1] = t
    table, extra = np.zeros((max_tracks, len(FIELDS)), dtype=np.int32), np.zeros((max_tracks, 2), dtype=np.int32)
    for t, row in enumerate(rows[:max_tracks]):
        table[t] = [row[k] for k in FIELDS]
        extra[t] = [row["bridges"], row["missed"]]
    spans = [last[t] - row["first_frame"] + 1 for t, row in enumerate(rows)]
    assert all(s == row["length"] + row["missed"] for s, row in zip(spans, rows))
    totals = np.array([len(rows), int(gap_links.sum()), n_objects, max(spans, default=0)], dtype=np.int32)
    out = {"prev": prev, "gap": gap, "track": trk, "totals": totals, "gap_links": gap_links, "table": table, "extra": extra, "heads": heads,
           "spans": spans}
    if want_paint:
        painted = np.zeros(labels.shape, dtype=np.int32)
        for f in range(n):
            for l in range(1, K + 1):
                painted[f][labels[f] == l] = trk[f, l - 1]
        out["track_labels"] = painted
    return out
