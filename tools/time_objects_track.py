"""Times the object tracker (csrc/objects_track.hip) on the -eval stack size, 2450 frames of 64 x 64 with K = 64, for three label stacks:

  blobs    a few discs per frame that drift a pixel or two per frame, appear and vanish, plus a little speckle, labelled by
           objects.label: what -eval -objects --track-iou sees;
  full     one full-frame object in every frame: the longest chain (every round of the pointer doubling has work to do) and every
           atomic of the table on one row;
  strips   64 row-objects in every frame: 64 tracks through the whole stack.

For each: objects.track as a whole (which also allocates the outputs and the scratch), the same with track_labels and rgb, and on its
own the inner matching (cgs_objects_match on the n - 1 pairs of neighbouring frames plus the self-pair, into preallocated buffers).
Median of 5 timed calls after a warm-up, device events.  Beside each the host alternative: the pairs' `best` copied to the host and a
numpy / Python walk over the frames that forms prev, the track numbers and the table (wall clock, --host-frames frames scaled to the
stack).  full_to_blobs is the ratio of the two objects.track times.  One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_objects_track.py [--out profiles/objects_track_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cgs_amd import _lib, objects  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402

IOU, K = 0.3, 64


def blob_stack(n, rs):
    """bool [n,64,64]: discs that live for a while and drift."""
    ys, xs = np.mgrid[0:64, 0:64]
    out = rs.rand(n, 64, 64) < 0.002
    for _ in range(n // 12):
        f0, life = rs.randint(0, n), rs.randint(2, 120)
        cy, cx, r = rs.uniform(0, 64), rs.uniform(0, 64), rs.uniform(3, 12)
        for f in range(f0, min(f0 + life, n)):
            cy, cx = cy + rs.uniform(-2, 2), cx + rs.uniform(-2, 2)
            out[f] |= np.hypot(ys - cy, xs - cx) < r
    return out


def pairs(labels, buffers=None):
    """The tracker's inner matching on its own: best [n,2,K,4] (slot f is the pair (f, f + 1), the last slot the last frame with itself)."""
    n = labels.shape[0]
    if buffers is None:
        buffers = (torch.tensor([round(IOU * 1000)], dtype=torch.int32).to(labels.device),
                   torch.empty((n, 4), dtype=torch.int32, device=labels.device), torch.empty((n, 2, K, 4), dtype=torch.int32, device=labels.device))
    thr, counts, best = buffers
    stream = torch.cuda.current_stream().cuda_stream
    if n > 1:
        _lib.call("cgs_objects_match", labels.data_ptr(), labels[1:].data_ptr(), n - 1, 64, 64, K, thr.data_ptr(), 1, counts.data_ptr(),
                  best.data_ptr(), stream)
    _lib.call("cgs_objects_match", labels[n - 1:].data_ptr(), labels[n - 1:].data_ptr(), 1, 64, 64, K, thr.data_ptr(), 1,
              counts[n - 1:].data_ptr(), best[n - 1:].data_ptr(), stream)
    return buffers


def host_walk(best, milli):
    """best [n,2,K,4] on the host -> (prev, track, table rows): the frames walked one after the other."""
    n = best.shape[0]
    prev, track, rows = np.zeros((n, K), dtype=np.int32), np.zeros((n, K), dtype=np.int32), []
    for f in range(n):
        area = best[f, 0, :, 2]
        if f:
            back, fwd = best[f - 1, 1], best[f - 1, 0]
            q, inter, union = back[:, 0], back[:, 1], back[:, 2] + back[:, 3] - back[:, 1]
            ok = (q > 0) & (inter > 0) & (1000 * inter >= milli * union) & (fwd[np.maximum(q, 1) - 1, 0] == np.arange(1, K + 1))
            prev[f] = np.where(ok & (area > 0), q, 0)
        for l in np.flatnonzero(area):
            a = int(area[l])
            if prev[f, l]:
                t = track[f - 1, prev[f, l] - 1]
                r = rows[t - 1]
                r[2] += 1
                r[3] += a
                r[4], r[5] = min(r[4], a), max(r[5], a)
                r[6] += int(best[f - 1, 1, l, 1])
                r[7] += int(best[f - 1, 1, l, 2] + best[f - 1, 1, l, 3] - best[f - 1, 1, l, 1])
            else:
                rows.append([f, l + 1, 1, a, a, a, 0, 0])
                t = len(rows)
            track[f, l] = t
    return prev, track, rows


def host_ms_per_stack(best, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = best[:frames].cpu().numpy()
    copied = time.perf_counter()
    out = host_walk(host, round(IOU * 1000))
    t1 = time.perf_counter()
    scale = best.shape[0] / frames
    return (copied - t0) * 1e3 * scale, (t1 - t0) * 1e3 * scale, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--host-frames", type=int, default=2450)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    tile = lambda frame: up(np.broadcast_to(frame, (n, 64, 64)).astype(np.int32))
    strips = (np.arange(4096, dtype=np.int32) // 64 + 1).reshape(64, 64)
    stacks = (("blobs", objects.label(up(blob_stack(n, rs))).labels), ("full", tile(np.ones((64, 64)))), ("strips", tile(strips)))
    rows, med = [], {}
    for name, labels in stacks:
        res = objects.track(labels, iou=IOU)
        ms = device_ms(lambda: objects.track(labels, iou=IOU))
        painted = device_ms(lambda: objects.track(labels, iou=IOU, want_labels=True, want_rgb=True))
        buffers = pairs(labels)
        inner = device_ms(lambda: pairs(labels, buffers))
        frames = min(a.host_frames, n)
        copy_ms, host_ms, (prev, track, table) = host_ms_per_stack(buffers[2], frames)
        if frames == n:                                                     # the walk and the kernels agree
            assert np.array_equal(prev, res.prev.cpu().numpy()) and np.array_equal(track, res.track.cpu().numpy())
            assert np.array_equal(np.array(table, dtype=np.int32).reshape(-1, 8), res.table[:len(table)].cpu().numpy())
        med[name] = float(np.median(ms))
        rows.append({"case": name, "n": n, "max_objects": K, "track_iou": IOU, "tracks": int(res.n_tracks), "links": int(res.n_links),
                     "objects": int(res.n_objects), "longest": int(res.longest), "ms_median": round(med[name], 4), "ms_min": round(min(ms), 4),
                     "ms_max": round(max(ms), 4), "with_paint_ms_median": round(float(np.median(painted)), 4),
                     "inner_match_ms_median": round(float(np.median(inner)), 4), "us_per_frame": round(med[name] * 1e3 / n, 4),
                     "host_copy_best_ms": round(copy_ms, 2), "host_copy_walk_ms": round(host_ms, 2)})
    stamp = {"full_to_blobs": round(med["full"] / med["blobs"], 3), "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0),
             "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
