"""Times the object matching kernel (csrc/objects_match.hip) on the -eval stack size, 2450 frames of 64 x 64, with K = 64 objects per
side and T = 10 thresholds (0.5:0.95:10), for three pairs of label stacks:

  blobs    a few discs per frame plus a little speckle as the truth, the same discs moved and resized a little as the prediction, both
           labelled by objects.label: what -eval -objects --match-iou sees;
  full     one full-frame object on both sides: every pixel of a frame goes to the same three LDS words, the worst case for
           contention (one add per row and target, thanks to the run-based adds);
  strips   64 objects on both sides (one row each, the truth shifted by 10 pixels): the longest scans of the matching step;

each with `best` written.  Median of 5 timed calls after a warm-up, device events around objects.match (which also uploads the ten
thresholds and allocates the outputs).  Beside each the host alternative: both stacks copied to the host, then per frame one
np.bincount of pred * 65 + truth (wall clock over --host-frames frames, scaled to the stack; the pair counts only, no matching).
full_to_blobs is the ratio of the two kernel times.  One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_objects_match.py [--out profiles/objects_match_time.jsonl]
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
from cgs_amd import objects  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402

IOU = [m / 1000 for m in range(500, 951, 50)]


def blob_pair(n, rs):
    """(prediction, truth) bool [n,64,64]."""
    ys, xs = np.mgrid[0:64, 0:64]
    pred, truth = np.zeros((n, 64, 64), dtype=bool), np.zeros((n, 64, 64), dtype=bool)
    for f in range(n):
        for _ in range(rs.randint(1, 5)):
            cy, cx, r = rs.uniform(0, 64), rs.uniform(0, 64), rs.uniform(3, 14)
            truth[f] |= np.hypot(ys - cy, xs - cx) < r
            if rs.rand() < 0.85:                                           # a missed object now and then
                pred[f] |= np.hypot(ys - cy - rs.normal(0, 1.5), xs - cx - rs.normal(0, 1.5)) < r * rs.uniform(0.75, 1.2)
    return pred | (rs.rand(n, 64, 64) < 0.004), truth | (rs.rand(n, 64, 64) < 0.002)


def host_ms_per_stack(pred, truth, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, t = pred[:frames].cpu().numpy(), truth[:frames].cpu().numpy()
    for a, b in zip(p, t):
        np.bincount((np.clip(a, 0, 64) * 65 + np.clip(b, 0, 64)).ravel(), minlength=65 * 65)
    return (time.perf_counter() - t0) * 1e3 * len(pred) / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--host-frames", type=int, default=2450)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    bp, bt = blob_pair(n, rs)
    strips = (np.arange(4096, dtype=np.int32) // 64 + 1).reshape(64, 64)
    tile = lambda frame: up(np.broadcast_to(frame, (n, 64, 64)).astype(np.int32))
    stacks = (("blobs", objects.label(up(bp)).labels, objects.label(up(bt)).labels),
              ("full", tile(np.ones((64, 64))), tile(np.ones((64, 64)))),
              ("strips", tile(strips), tile(np.roll(strips, 10))))
    rows, med = [], {}
    for name, pred, truth in stacks:
        res = objects.match(pred, truth, iou=IOU)
        ms = device_ms(lambda: objects.match(pred, truth, iou=IOU))
        bare = device_ms(lambda: objects.match(pred, truth, iou=IOU, want_best=False))
        host = host_ms_per_stack(pred, truth, min(a.host_frames, n))
        med[name] = float(np.median(ms))
        rows.append({"case": name, "n": n, "max_objects": 64, "thresholds": len(IOU),
                     "pred_objects_per_frame_mean": round(float(res.pred_max.float().mean()), 2),
                     "truth_objects_per_frame_mean": round(float(res.truth_max.float().mean()), 2),
                     "matched_at_0.5_per_frame_mean": round(float(res.matched_pred[:, 0].float().mean()), 2),
                     "ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "counts_only_ms_median": round(float(np.median(bare)), 4), "us_per_frame": round(med[name] * 1e3 / n, 4),
                     "host_copy_bincount_ms": round(host, 2)})
    stamp = {"full_to_blobs": round(med["full"] / med["blobs"], 3), "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0),
             "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
