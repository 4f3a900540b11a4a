"""The rule of cgs_objects_appearance / cgs_objects_reid (the header comment in include/cgs_hip.h) in Python integers and numpy: no torch,
nothing taken from the kernels.  ``appearance`` gives the object and track histograms, ``reid`` the links and identities."""
import numpy as np

BINS, SCALE = 64, 4096


def bins_of(frames):
    """frames uint8 [..., 3] -> the bin of every pixel, ((R >> 6) << 4) | ((G >> 6) << 2) | (B >> 6)."""
    f = np.asarray(frames).astype(np.int64)
    return ((f[..., 0] >> 6) << 4) | ((f[..., 1] >> 6) << 2) | (f[..., 2] >> 6)


def appearance(frames, labels, track, K, rows=None):
    """frames uint8 [n,h,w,3], labels int [n,h,w], track int [n,K] or None.  Returns (S int64 [rows,64] or None, H int64 [n,K,64]);
    rows defaults to n * K."""
    labels = np.asarray(labels).astype(np.int64)
    n = labels.shape[0]
    b = bins_of(frames)
    H = np.zeros((n, K, BINS), dtype=np.int64)
    for f in range(n):
        inside = (labels[f] >= 1) & (labels[f] <= K)
        np.add.at(H[f], (labels[f][inside] - 1, b[f][inside]), 1)
    if track is None:
        return None, H
    rows = n * K if rows is None else rows
    track = np.asarray(track).astype(np.int64)
    S = np.zeros((rows, BINS), dtype=np.int64)
    for f in range(n):
        for l in range(K):
            t = int(track[f, l])
            if 1 <= t <= rows:
                S[t - 1] += H[f, l]
    return S, H


def signatures(S, n_tracks, min_area):
    """(Q int64 [rows,64], D list) of the first n_tracks rows of S; the others stay zero."""
    S = np.asarray(S).astype(np.int64)
    Q = np.zeros_like(S)
    D = [0] * S.shape[0]
    for t in range(n_tracks):
        A = int(S[t].sum())
        if A >= min_area:
            Q[t] = [int(v) * SCALE // A for v in S[t]]
            D[t] = int(Q[t].sum())
    return Q, D


def reid(table, extra, S, n_tracks, milli, W, min_area):
    """table int [rows,8], extra int [rows,2] or None, S int [rows,64].  Returns a dict: prev, next, sim, identity (int64 [rows], by t - 1),
    Q int64 [rows,64], totals [identities, links, eligible, longest], and for the tests' own conditions: admissible (the list of
    admissible pairs (t, u, s)), succ, pred (dicts), ties (how many succ / pred choices had a second candidate of the same s)."""
    table = np.asarray(table).astype(np.int64)
    rows = table.shape[0]
    N = max(0, min(int(n_tracks), rows))
    Q, D = signatures(S, N, min_area)
    F = [int(table[t, 0]) for t in range(N)]
    L = [int(table[t, 0]) + int(table[t, 2]) + (int(extra[t][1]) if extra is not None else 0) - 1 for t in range(N)]
    admissible = []
    for t in range(N):
        if not D[t]:
            continue
        for u in range(N):
            if D[u] and L[t] < F[u] <= L[t] + W:
                s = int(np.minimum(Q[t], Q[u]).sum())
                if 1000 * s >= milli * min(D[t], D[u]):
                    admissible.append((t + 1, u + 1, s))
    succ, pred, ties = {}, {}, 0
    for t, u, s in admissible:                                           # ascending t, then u: strictly larger keeps the smallest number
        if t not in succ or s > succ[t][1]:
            succ[t] = (u, s)
        if u not in pred or s > pred[u][1]:
            pred[u] = (t, s)
    for t, u, s in admissible:
        ties += (succ[t][1] == s and succ[t][0] != u) + (pred[u][1] == s and pred[u][0] != t)
    prev, nxt, sim, identity = (np.zeros(rows, dtype=np.int64) for _ in range(4))
    for t, (u, s) in succ.items():
        if pred[u][0] == t:
            nxt[t - 1], prev[u - 1], sim[u - 1] = u, t, s
    count, sizes = 0, {}
    for t in range(1, N + 1):                                            # a link runs to a larger number: prev is numbered already
        if prev[t - 1]:
            identity[t - 1] = identity[prev[t - 1] - 1]
        else:
            count += 1
            identity[t - 1] = count
        sizes[int(identity[t - 1])] = sizes.get(int(identity[t - 1]), 0) + 1
    totals = [count, int(np.count_nonzero(prev)), sum(1 for d in D[:N] if d), max(sizes.values()) if sizes else 0]
    return {"prev": prev, "next": nxt, "sim": sim, "identity": identity, "Q": Q, "totals": totals, "admissible": admissible,
            "succ": succ, "pred": pred, "ties": ties}


def object_identities(track, identity):
    """track int [n,K], identity int [rows] -> the identity of every object, 0 where there is none."""
    track, identity = np.asarray(track).astype(np.int64), np.asarray(identity).astype(np.int64)
    inside = (track >= 1) & (track <= identity.shape[0])
    return np.where(inside, identity[np.clip(track - 1, 0, max(identity.shape[0] - 1, 0))] if identity.shape[0] else 0, 0)
