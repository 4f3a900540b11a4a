"""The direct form of what cgs_objects_match computes (include/cgs_hip.h), the checker of tests/test_objects_match_host.py and
tests/test_gpu_objects_match.py: per frame a loop over the pixels fills a dict of pair counts and two dicts of areas, and every IoU is
a fractions.Fraction -- nothing of the kernel's runs, ballots or cross-multiplication.  Also the frame generator of the tests."""
from fractions import Fraction

import numpy as np


def match_frame(pred, truth, milli, max_objects=64):
    """pred, truth: integer [h,w]; milli: thresholds in thousandths.  Returns (counts int32 [2 + 2 T], best int32 [2,K,4],
    sums: per threshold the list of Fractions the frame adds to sum_iou)."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    h, w = pred.shape
    K = max_objects
    areas, pairs, largest = ({}, {}), {}, [0, 0]
    for y in range(h):
        for x in range(w):
            p, t = int(pred[y, x]), int(truth[y, x])
            largest[0], largest[1] = max(largest[0], p), max(largest[1], t)
            p, t = (p if 1 <= p <= K else 0), (t if 1 <= t <= K else 0)
            if p:
                areas[0][p] = areas[0].get(p, 0) + 1
            if t:
                areas[1][t] = areas[1].get(t, 0) + 1
            if p and t:
                pairs[(p, t)] = pairs.get((p, t), 0) + 1
    counts = np.zeros(2 + 2 * len(milli), dtype=np.int32)
    counts[:2] = largest
    best = np.zeros((2, K, 4), dtype=np.int32)
    sums = [[] for _ in milli]
    for side in (0, 1):
        for a in range(1, min(largest[side], K) + 1):
            own = areas[side].get(a, 0)
            top, row = Fraction(0), (0, 0, own, 0)
            for b in range(1, min(largest[1 - side], K) + 1):                  # ascending: a tie stays with the smaller number
                inter = pairs.get((a, b) if side == 0 else (b, a), 0)
                if inter == 0:
                    continue
                other = areas[1 - side][b]
                value = Fraction(inter, own + other - inter)
                if value > top:
                    top, row = value, (b, inter, own, other)
            best[side, a - 1] = row
            for k, m in enumerate(milli):
                if top > 0 and top >= Fraction(int(m), 1000):
                    counts[2 + 2 * k + side] += 1
                    if side == 0:
                        sums[k].append(top)
    return counts, best, sums


def match(pred, truth, milli, max_objects=64):
    """pred, truth: integer [n,h,w].  Returns (counts int32 [n, 2 + 2 T], best int32 [n,2,K,4], sum_iou float64 [T]: the exact sum of
    Fractions over the stack, rounded once)."""
    frames = [match_frame(p, t, milli, max_objects) for p, t in zip(np.asarray(pred), np.asarray(truth))]
    total = [sum((v for f in frames for v in f[2][k]), Fraction(0)) for k in range(len(milli))]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.array([float(v) for v in total], dtype=np.float64)


def split_counts(counts):
    """counts [n, 2 + 2 T] -> pred_max [n], truth_max [n], matched_pred [n,T], matched_truth [n,T]."""
    counts = np.asarray(counts)
    pairs = counts[:, 2:].reshape(counts.shape[0], -1, 2)
    return counts[:, 0], counts[:, 1], pairs[:, :, 0], pairs[:, :, 1]


# ---------------------------------------------------------------------------------------------------------------- the generator
KINDS = ("exact", "shifted", "left_half", "column_short", "poor", "missing", "spurious")


def generator_frame(seed):
    """(pred, truth) bool [64,64]: a 4 x 4 grid of 16 x 16 cells; per cell a truth rectangle at least 6 x 6 that keeps two pixels
    clear of the cell's border (so neighbouring cells never touch, at either connectivity), and a prediction of one of KINDS: the
    rectangle itself; shifted by (1, 1); its left half; all but its last column; one corner pixel of it plus a block outside it
    (IoU far below 1/2); none; or a rectangle with no truth under it."""
    rs = np.random.RandomState(seed)
    pred, truth = np.zeros((64, 64), dtype=bool), np.zeros((64, 64), dtype=bool)
    for cell in range(16):
        cy, cx = 16 * (cell // 4), 16 * (cell % 4)
        bh, bw = rs.randint(6, 10), rs.randint(6, 10)
        y0, x0 = cy + rs.randint(2, 14 - bh - 1), cx + rs.randint(2, 14 - bw - 1)
        kind = KINDS[rs.randint(len(KINDS))]
        if kind != "spurious":
            truth[y0:y0 + bh, x0:x0 + bw] = True
        if kind in ("exact", "spurious"):
            pred[y0:y0 + bh, x0:x0 + bw] = True
        elif kind == "shifted":
            pred[y0 + 1:y0 + bh + 1, x0 + 1:x0 + bw + 1] = True
        elif kind == "left_half":
            pred[y0:y0 + bh, x0:x0 + bw // 2] = True
        elif kind == "column_short":
            pred[y0:y0 + bh, x0:x0 + bw - 1] = True
        elif kind == "poor":
            pred[y0 + bh - 1:y0 + bh + 2, x0 + bw - 1:x0 + bw + 2] = True
    return pred, truth
