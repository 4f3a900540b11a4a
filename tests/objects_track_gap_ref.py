"""The direct form of what cgs_objects_track_gap computes (include/cgs_hip.h), the checker of tests/test_objects_track_gap_host.py and
tests/test_gpu_objects_track_gap.py: the level-order walk as it is defined.  For level g the two frames are masked in numpy (every
label that is not an open tail, or not an open head, becomes 0) and handed to objects_track_ref.links; the numbers, the tables,
gap_links, the extras and the span come from a plain walk over the frames.  ``fragments`` is built from Python sets.  Nothing of the
kernels' 64-bit masks, match tables, pointer doubling, scans or atomics."""
from fractions import Fraction

import numpy as np

import objects_track_ref as base

FIELDS = base.FIELDS


def _objects(frame, K):
    frame = np.asarray(frame)
    return {int(l) for l in np.unique(frame) if 1 <= l <= K}


def _masked(frame, keep):
    frame = np.asarray(frame)
    return np.where(np.isin(frame, sorted(keep)), frame, 0)


def all_links(labels, milli, K, G):
    """labels integer [n,h,w] -> {(f, q): (p, g, inter, union)}: object q of frame f continues object p of frame f - g."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    objs = [_objects(labels[f], K) for f in range(n)]
    has_next, has_prev, out = [set() for _ in range(n)], [set() for _ in range(n)], {}
    for g in range(1, G + 2):
        made = []
        for f in range(g, n):                                               # the f's of a level do not see each other's links
            if g == 1:
                a, b = labels[f - 1], labels[f]
            else:
                a, b = _masked(labels[f - g], objs[f - g] - has_next[f - g]), _masked(labels[f], objs[f] - has_prev[f])
            for q, (p, inter, union) in base.links(a, b, milli, K).items():
                made.append((f, q, p, inter, union))
        for f, q, p, inter, union in made:
            assert q not in has_prev[f] and p not in has_next[f - g]
            has_prev[f].add(q)
            has_next[f - g].add(p)
            out[(f, q)] = (p, g, inter, union)
    return out


def track(labels, milli, K=64, G=0, max_tracks=None, want_paint=False):
    """labels integer [n,h,w].  Returns a dict: prev, gap, track int32 [n,K]; totals int32 [4] (tracks, links, objects, longest span);
    gap_links int32 [G + 1]; table int32 [max_tracks,8]; extra int32 [max_tracks,2] (bridges, missed); heads; spans: per track; and
    with want_paint track_labels int32 [n,h,w]."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    max_tracks = n * K if max_tracks is None else max_tracks
    link = all_links(labels, milli, K, G)
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


def _reach(partners, m):
    return lambda f, q: q in partners[f] and Fraction(partners[f][q][1], partners[f][q][2]) >= Fraction(int(m), 1000)


def switches(pred, truth, track_milli, match_milli, K=64, G=0):
    """objects_track_ref.switches with both stacks tracked at gap G: only the truth's adjacent links (gap 1) are followed."""
    pt, tt = track(pred, track_milli, K, G), track(truth, track_milli, K, G)
    partners = base.truth_partners(pred, truth, K)
    counts = np.zeros((len(match_milli), 3), dtype=np.int32)
    for k, m in enumerate(match_milli):
        reach = _reach(partners, m)
        for f in range(len(partners)):
            for q in range(1, K + 1):
                if not reach(f, q):
                    continue
                counts[k, 0] += 1
                q0 = int(tt["prev"][f, q - 1]) if tt["gap"][f, q - 1] == 1 else 0
                if q0 and reach(f - 1, q0):
                    counts[k, 1] += 1
                    counts[k, 2] += pt["track"][f, partners[f][q][0] - 1] != pt["track"][f - 1, partners[f - 1][q0][0] - 1]
    return counts


def fragments(pred, truth, track_milli, match_milli, K=64, G=0):
    """Per matching threshold, over the covered truth objects: distinct (truth track, predicted track) pairs - distinct truth tracks."""
    pt, tt = track(pred, track_milli, K, G), track(truth, track_milli, K, G)
    partners = base.truth_partners(pred, truth, K)
    out = []
    for m in match_milli:
        reach = _reach(partners, m)
        pairs, truths = set(), set()
        for f in range(len(partners)):
            for q in range(1, K + 1):
                if reach(f, q):
                    t = int(tt["track"][f, q - 1])
                    pairs.add((t, int(pt["track"][f, partners[f][q][0] - 1])))
                    truths.add(t)
        out.append(len(pairs) - len(truths))
    return np.array(out, dtype=np.int64)
