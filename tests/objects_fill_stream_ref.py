"""What tests/test_gpu_objects_fill_stream.py needs beside tests/objects_track_fill_ref.py, in numpy and Python integers: the flickering
stacks, the per-frame form of the four totals (a frame range's totals are sums of these), and the facts about a whole-stack result that
the stream test asserts so that nothing passes vacuously."""
import numpy as np

import objects_track_fill_ref as ref


def stack(n, h, w, seed):
    """int32 [n,h,w].  One blob per lane of rows (lanes of 8 rows at h = 64, else 5), each drifting right by 0 or 1 cell a frame and
    wrapping; a blob is on or off by a two-state chain (on -> off with p = 0.25, off -> on with p = 0.35).  In lane 0, in half of its off
    frames (the first, the third, ... of them), a bar over the lane's full width takes the blob's place: a mask carried there finds no
    free cell.  The blobs (and the bar)
    of a frame are numbered from the top, as objects.label numbers them."""
    rs = np.random.RandomState(seed)
    lane, bh, bw = (8, 6, 16) if h == 64 else (5, 3, 6)      # (a bar is over 3 blobs wide: at IoU 0.3 it never links to one)
    lanes = h // lane
    out = np.zeros((n, h, w), dtype=np.int32)
    x = rs.randint(0, w - bw + 1, lanes)
    on = rs.rand(lanes) < 0.6
    offs = 0
    for f in range(n):
        if f:
            x = x + rs.randint(0, 2, lanes)
            flip = rs.rand(lanes)
            on = np.where(on, flip >= 0.25, flip < 0.35)
        offs += int(not on[0])
        bar = (not on[0]) and offs % 2 == 1
        k = 0
        for i in range(lanes):
            y0 = i * lane + 1
            if on[i]:
                k += 1
                x0 = int(x[i]) % (w - bw + 1)
                out[f, y0:y0 + bh, x0:x0 + bw] = k
            elif i == 0 and bar:
                k += 1
                out[f, y0:y0 + bh, :] = k
    out.setflags(write=False)
    return out


def frame_totals(labels, bwd, prev, gap, track, K=64, G=8):
    """int64 [n,4]: what frame m adds to cgs_objects_track_fill's totals (objects, cells, dropped, vanished) -- objects_track_fill_ref.fill's
    claims frame by frame, the numbering of its _finish counted instead of written."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((n, 4), dtype=np.int64)
    for m in range(n):
        claims, vanished = {}, 0
        taken = labels[m] > 0
        for j in range(1, min(G, m) + 1):
            S = ref.spanning(prev, gap, m, j, K, G)
            if not S:
                continue
            W = ref.base._clip(labels[m - j], K) if bwd is None else ref.mc_ref.carried(labels[m - j], bwd, m - j, m, K)
            hit = ~taken & np.isin(W, sorted(S))
            for y, x in zip(*np.nonzero(hit)):
                claims[(int(y), int(x))] = (j, int(W[y, x]))
            taken = taken | hit
            vanished += len(S - {int(v) for v in np.unique(W[hit])})
        top = max(int(labels[m].max()), 0)
        cands = sorted(set(claims.values()))
        made = min(len(cands), max(K - top, 0))
        out[m] = [made, sum(1 for c in claims.values() if cands.index(c) < made), len(cands) - made, vanished]
    return out


def heads_in_later_chunks(age, gap, track, sizes):
    """The number of filled objects (age > 0) whose link's head lies in a later chunk of the split `sizes` than the filled frame: the
    frames a stream can only fill by looking ahead.  The head of the link that jumps over frame m from the tail (m - j, p) is the frame
    f > m with gap[f][l] == f - (m - j) in the tail's track: `track` is the filled stack's, where the filled object carries that number."""
    age, gap = np.asarray(age), np.asarray(gap)
    n, K = age.shape
    chunk = np.repeat(np.arange(len(sizes)), sizes)
    assert len(chunk) == n
    count = 0
    for m, l in zip(*np.nonzero(age > 0)):
        a = int(m) - int(age[m, l])
        heads = [f for f in range(int(m) + 1, min(n, a + gap.max() + 1)) for q in range(K)
                 if int(gap[f, q]) == f - a and int(track[f][q]) == int(track[m][l])]
        assert len(heads) == 1, (m, l, heads)
        count += int(chunk[heads[0]] > chunk[m])
    return count
