"""The direct form of the rule of cgs_graph_cut (include/cgs_hip.h), the checker of tests/test_graph_cut_host.py and
tests/test_gpu_graph_cut.py: Python integers and numpy for the trimap, the n-links and the colour histograms, the capacities from
``graphcut.tables``, the maximum flow from ``scipy.sparse.csgraph.maximum_flow(method="dinic")`` on the whole graph (source, sink and
every t-link, nothing folded away), and the cut from a backward breadth-first search from the sink in capacity - flow.  Nothing of the
kernel's schedule: no push-relabel, no rounds -- which is why the `rounds` column is the one figure this file cannot give (it is
reported as 0)."""
from collections import namedtuple

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_flow

from cgs_amd import graphcut

EMPTY, EARLY, NOT_CONVERGED = 1, 2, 4
STATUS, ITERATIONS, ROUNDS, ENERGY, SEED_ON, ON, UNKNOWN, CHANGED = range(8)
AXIAL, DIAGONAL = ((0, 1), (1, 0)), ((1, 1), (1, -1))
Cut = namedtuple("Cut", ["mask", "stats"])


def trimap(z, thresh, inclusive, lo, hi):
    """(seed bool, hard background bool, hard foreground bool) of one float32 mask, compared in float32."""
    z = np.asarray(z, dtype=np.float32)
    t, a, b = np.float32(thresh), np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        seed = (z >= t) if inclusive else (z > t)
        return seed, (z < a) | np.isnan(z), z > b


def pairs(frame, connectivity):
    """The unordered neighbour pairs of a frame: (p, q, d2, diagonal) with p, q flat cell indices and d2 the integer squared RGB distance."""
    h, w = frame.shape[:2]
    f = frame.astype(np.int64)
    out = []
    for y in range(h):
        for x in range(w):
            for diagonal, steps in ((False, AXIAL), (True, DIAGONAL)):
                if diagonal and connectivity != 8:
                    continue
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w:
                        out.append((y * w + x, yy * w + xx, int(((f[y, x] - f[yy, xx]) ** 2).sum()), diagonal))
    return out


def n_links(frame, connectivity, WA, WD):
    """[(p, q, capacity)] of the frame's pairs, and m."""
    ps = pairs(frame, connectivity)
    m = max(1, sum(d2 for _, _, d2, _ in ps) // len(ps)) if ps else 1
    return [(p, q, int((WD if diag else WA)[min(1023, 64 * d2 // m)])) for p, q, d2, diag in ps], m


def t_links(frame, label, hard_bg, hard_fg, bins, L, big):
    """(source -> cell, cell -> sink) int arrays [h*w] for the labelling `label`, or None when a side is empty."""
    s = {4: 6, 8: 5}[bins]
    f = frame.astype(np.int64) >> s
    bin_ = ((f[..., 0] * bins + f[..., 1]) * bins + f[..., 2]).ravel()
    lab = label.ravel()
    B = bins ** 3
    H1, H0 = np.bincount(bin_[lab], minlength=B), np.bincount(bin_[~lab], minlength=B)
    N1, N0 = int(lab.sum()), int((~lab).sum())
    if N1 == 0 or N0 == 0:
        return None
    cost_fg = L[N1 + B] - L[H1[bin_] + 1]
    cost_bg = L[N0 + B] - L[H0[bin_] + 1]
    cs = np.where(hard_fg.ravel(), big, np.where(hard_bg.ravel(), 0, cost_bg)).astype(np.int64)
    ct = np.where(hard_fg.ravel(), 0, np.where(hard_bg.ravel(), big, cost_fg)).astype(np.int64)
    return cs, ct


def min_cut(P, links, cs, ct):
    """(flow value, bool [P]: the cells that cannot reach the sink in the residual graph) of the graph with nodes 0..P-1, source P, sink
    P + 1: scipy's Dinic on the whole graph, then a backward search from the sink over arcs with capacity - flow > 0."""
    S, T = P, P + 1
    cap = {}
    for p, q, c in links:
        if c > 0:
            cap[(p, q)] = cap.get((p, q), 0) + c
            cap[(q, p)] = cap.get((q, p), 0) + c
    for p in range(P):
        if cs[p] > 0:
            cap[(S, p)] = int(cs[p])
        if ct[p] > 0:
            cap[(p, T)] = int(ct[p])
    if not cap:
        return 0, np.ones(P, dtype=bool)
    rows, cols = (np.array(v, dtype=np.int32) for v in zip(*cap.keys()))
    graph = csr_matrix((np.array(list(cap.values()), dtype=np.int32), (rows, cols)), shape=(P + 2, P + 2))
    res = maximum_flow(graph, S, T, method="dinic")
    flow = res.flow.tocoo()
    resid = dict(cap)                                     # capacity - flow (flow is antisymmetric, so an arc without capacity can have residual)
    for u, v, f in zip(flow.row, flow.col, flow.data):
        if f:
            resid[(int(u), int(v))] = resid.get((int(u), int(v)), 0) - int(f)
    into = {}
    for (u, v), r in resid.items():
        assert r >= 0
        if r > 0:
            into.setdefault(v, []).append(u)
    reach = np.zeros(P + 2, dtype=bool)
    reach[T] = True
    stack = [T]
    while stack:
        v = stack.pop()
        for u in into.get(v, ()):
            if not reach[u]:
                reach[u] = True
                stack.append(u)
    assert not reach[S]
    return int(res.flow_value), ~reach[:P]


def cut_frame(frame, z, thresh, inclusive=False, lo=None, hi=None, lam=50, iters=3, bins=8, connectivity=8):
    """One frame: (mask bool [h,w], stats int64 [8], rounds reported as 0)."""
    frame = np.asarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    d_lo, d_hi = graphcut.default_band(float(thresh))
    lo, hi = d_lo if lo is None else lo, d_hi if hi is None else hi
    WA, WD, L = (t.astype(np.int64) for t in graphcut.tables(lam))
    big = 8 * int(WA[0]) + 1
    seed, hard_bg, hard_fg = trimap(z, thresh, inclusive, lo, hi)
    assert not (hard_bg & seed).any() and (seed | ~hard_fg).all()
    links, _m = n_links(frame, connectivity, WA, WD)
    label, status, run, energy = seed.copy(), 0, 0, 0
    for _ in range(iters):
        t = t_links(frame, label, hard_bg, hard_fg, bins, L, big)
        if t is None:
            status |= EMPTY
            break
        energy, fg = min_cut(h * w, links, *t)
        run += 1
        new = fg.reshape(h, w)
        same = bool((new == label).all())
        label = new
        if same:
            if run < iters:
                status |= EARLY
            break
    stats = np.array([status, run, 0, energy, seed.sum(), label.sum(), (~hard_bg & ~hard_fg).sum(), (label != seed).sum()], dtype=np.int64)
    return label, stats


def cut(frames, masks, thresh, **kw):
    """A stack: frames uint8 [n,h,w,3], masks float32 [n,h,w] -> Cut(mask bool [n,h,w], stats int64 [n,8])."""
    res = [cut_frame(f, z, thresh, **kw) for f, z in zip(frames, masks)]
    return Cut(np.stack([m for m, _ in res]), np.stack([s for _, s in res]))
