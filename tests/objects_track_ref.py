"""The direct form of what cgs_objects_track and cgs_objects_track_switches compute (include/cgs_hip.h), the checker of
tests/test_objects_track_host.py and tests/test_gpu_objects_track.py: pair counts by one np.bincount of p * 65 + q per pair of frames,
best partners by exact fractions.Fraction compares (ties to the smallest number), a plain walk over the frames for the tracks, Python
sums for the table and loops for the switch counts -- nothing of the kernels' match tables, pointer doubling, scans or atomics."""
from fractions import Fraction

import numpy as np

FIELDS = ("first_frame", "first_label", "length", "area_sum", "area_min", "area_max", "inter_sum", "union_sum")


def _clip(frame, K):
    frame = np.asarray(frame).astype(np.int64)
    return np.where((frame >= 1) & (frame <= K), frame, 0)


def pair_counts(a, b, K):
    """a, b integer [h,w] -> (inter [65,65] over labels 0..64 clipped to 1..K, area_a [65], area_b [65])."""
    a, b = _clip(a, K), _clip(b, K)
    table = np.bincount((a * 65 + b).ravel(), minlength=65 * 65).reshape(65, 65)
    return table, table.sum(axis=1), table.sum(axis=0)


def best_partner(inter_row, own, other_areas, K):
    """(partner, inter) of largest IoU among 1..K with inter > 0, the smallest number on a tie; (0, 0) without overlap."""
    top, pick = Fraction(0), (0, 0)
    for j in range(1, K + 1):
        inter = int(inter_row[j])
        if inter > 0:
            value = Fraction(inter, int(own) + int(other_areas[j]) - inter)
            if value > top:
                top, pick = value, (j, inter)
    return pick


def links(a, b, milli, K):
    """Frames f and f + 1 -> {q: (p, inter, union)} for every linked pair."""
    table, area_a, area_b = pair_counts(a, b, K)
    out = {}
    for q in range(1, K + 1):
        if area_b[q] == 0:
            continue
        p, inter = best_partner(table[:, q], area_b[q], area_a, K)
        if p == 0 or best_partner(table[p, :], area_a[p], area_b, K)[0] != q:
            continue
        union = int(area_a[p] + area_b[q]) - inter
        if Fraction(inter, union) >= Fraction(int(milli), 1000):
            out[q] = (p, inter, union)
    return out


def track(labels, milli, K=64, max_tracks=None, want_paint=False):
    """labels integer [n,h,w].  Returns a dict: prev, track int32 [n,K]; totals int32 [4]; table int32 [max_tracks,8] (max_tracks
    defaults to n K); heads: the list of (frame, label) in numbering order; and with want_paint track_labels int32 [n,h,w]."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    max_tracks = n * K if max_tracks is None else max_tracks
    prev, trk = np.zeros((n, K), dtype=np.int32), np.zeros((n, K), dtype=np.int32)
    rows, heads, n_links, n_objects = [], [], 0, 0
    for f in range(n):
        area = np.bincount(_clip(labels[f], K).ravel(), minlength=65)
        link = links(labels[f - 1], labels[f], milli, K) if f else {}
        for l in range(1, K + 1):                                            # by frame, then by label: the numbering order
            if area[l] == 0:
                continue
            n_objects += 1
            a = int(area[l])
            if l in link:
                p, inter, union = link[l]
                prev[f, l - 1], t = p, int(trk[f - 1, p - 1])
                row = rows[t - 1]
                row["length"] += 1
                row["area_sum"] += a
                row["area_min"], row["area_max"] = min(row["area_min"], a), max(row["area_max"], a)
                row["inter_sum"] += inter
                row["union_sum"] += union
                n_links += 1
            else:
                heads.append((f, l))
                rows.append({"first_frame": f, "first_label": l, "length": 1, "area_sum": a, "area_min": a, "area_max": a, "inter_sum": 0,
                             "union_sum": 0})
                t = len(rows)
            trk[f, l - 1] = t
    table = np.zeros((max_tracks, len(FIELDS)), dtype=np.int32)
    for t, row in enumerate(rows[:max_tracks]):
        table[t] = [row[k] for k in FIELDS]
    totals = np.array([len(rows), n_links, n_objects, max([r["length"] for r in rows], default=0)], dtype=np.int32)
    out = {"prev": prev, "track": trk, "totals": totals, "table": table, "heads": heads}
    if want_paint:
        painted = np.zeros(labels.shape, dtype=np.int32)
        for f in range(n):
            for l in range(1, K + 1):
                painted[f][labels[f] == l] = trk[f, l - 1]
        out["track_labels"] = painted
    return out


def colours(track_labels):
    """The rgb of include/cgs_hip.h applied to a map of track numbers: uint8 [..., 3]."""
    t = np.asarray(track_labels).astype(np.uint64)
    hsh = (t * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    out = np.zeros(t.shape + (3,), dtype=np.uint8)
    for c in range(3):
        out[..., c] = np.where(t > 0, 64 + ((hsh >> np.uint64(8 * c)) & np.uint64(255)) * np.uint64(191) // np.uint64(255), 0).astype(np.uint8)
    return out


def truth_partners(pred, truth, K):
    """Per frame {q: (p, inter, union)}: every truth object's best predicted object (cgs_objects_match's side 1)."""
    out = []
    for a, b in zip(np.asarray(pred), np.asarray(truth)):
        table, area_p, area_t = pair_counts(a, b, K)
        frame = {}
        for q in range(1, K + 1):
            if area_t[q]:
                p, inter = best_partner(table[:, q], area_t[q], area_p, K)
                if p:
                    frame[q] = (p, inter, int(area_t[q] + area_p[p]) - inter)
        out.append(frame)
    return out


def switches(pred, truth, track_milli, match_milli, K=64):
    """pred, truth integer [n,h,w]: both tracked at track_milli; int32 [T,3] = (covered, continued, switches) per matching threshold."""
    pt, tt = track(pred, track_milli, K), track(truth, track_milli, K)
    partners = truth_partners(pred, truth, K)
    counts = np.zeros((len(match_milli), 3), dtype=np.int32)
    for k, m in enumerate(match_milli):
        reach = lambda f, q: q in partners[f] and Fraction(partners[f][q][1], partners[f][q][2]) >= Fraction(int(m), 1000)
        for f in range(len(partners)):
            for q in range(1, K + 1):
                if not reach(f, q):
                    continue
                counts[k, 0] += 1
                q0 = int(tt["prev"][f, q - 1])
                if q0 and reach(f - 1, q0):
                    counts[k, 1] += 1
                    counts[k, 2] += pt["track"][f, partners[f][q][0] - 1] != pt["track"][f - 1, partners[f - 1][q0][0] - 1]
    return counts
