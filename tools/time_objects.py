"""Times the object labelling kernel (csrc/objects.hip) on the -eval stack size, 2450 frames of 64 x 64, for four stacks:

  blobs         blob-like masks (a few discs per frame plus a little speckle), what a trained masker gives;
  random45      every pixel on with probability 0.45 (hundreds of small components per frame);
  spiral        the one-pixel 64 x 64 spiral in every frame: one component, the longest path a frame can hold;
  checkerboard  at connectivity 4: 2048 components per frame, the most a frame can hold (the others run at connectivity 8);

each with labels, the kept mask and a 256-row table written (as -process -objects) and with the kept mask alone and a 1-row table (as
-eval -objects).  Median of 5 timed calls after a warm-up, device events around objects.label (which also allocates the outputs).
Beside each, where scipy is importable, the host alternative: the stack copied to the host and one scipy.ndimage.label call per
frame (wall clock over --host-frames frames, scaled to the stack; labelling only, no table).  spiral_to_blobs is the ratio of the two
kernel times.  One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_objects.py [--out profiles/objects_time.jsonl]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import objects_ref  # noqa: E402  (the spiral and the checkerboard)
from cgs_amd import objects  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402


def blobs(n, rs):
    ys, xs = np.mgrid[0:64, 0:64]
    out = np.zeros((n, 64, 64), dtype=bool)
    for f in range(n):
        for _ in range(rs.randint(1, 5)):
            cy, cx, r = rs.uniform(0, 64), rs.uniform(0, 64), rs.uniform(3, 14)
            out[f] |= np.hypot(ys - cy, xs - cx) < r
    return out | (rs.rand(n, 64, 64) < 0.004)


def host_ms_per_stack(stack, connectivity, frames):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else None
    dev = torch.from_numpy(stack[:frames]).to("cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for frame in dev.cpu().numpy():
        ndimage.label(frame, structure=structure)
    return (time.perf_counter() - t0) * 1e3 * len(stack) / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--host-frames", type=int, default=245)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n = a.n
    tile = lambda frame: np.broadcast_to(frame, (n, 64, 64)).copy()
    stacks = (("blobs", blobs(n, rs), 8), ("random45", rs.rand(n, 64, 64) < 0.45, 8), ("spiral", tile(objects_ref.spiral()), 8),
              ("checkerboard", tile(objects_ref.checkerboard()), 4))
    rows, full = [], {}
    for name, stack, conn in stacks:
        dev = torch.from_numpy(stack).to("cuda")
        res = objects.label(dev, connectivity=conn, max_objects=256)
        found = res.found.cpu().numpy()
        all_ms = device_ms(lambda: objects.label(dev, connectivity=conn, max_objects=256, want_labels=True, want_mask=True))
        mask_ms = device_ms(lambda: objects.label(dev, connectivity=conn, max_objects=1, want_labels=False, want_mask=True))
        host = host_ms_per_stack(stack, conn, min(a.host_frames, n))
        full[name] = float(np.median(all_ms))
        rows.append({"case": name, "n": n, "connectivity": conn, "found_per_frame_mean": round(float(found.mean()), 2),
                     "ms_median": round(full[name], 4), "ms_min": round(min(all_ms), 4), "ms_max": round(max(all_ms), 4),
                     "mask_only_ms_median": round(float(np.median(mask_ms)), 4),
                     "us_per_frame": round(full[name] * 1e3 / n, 4),
                     "host_scipy_loop_ms": None if host is None else round(host, 2)})
    stamp = {"spiral_to_blobs": round(full["spiral"] / full["blobs"], 3), "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0),
             "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
