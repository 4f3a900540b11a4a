"""Times the mask clean-up kernel (csrc/clean.hip) on the -eval stack size, 2450 frames of 64 x 64, on two soft stacks read at 0.5:

  blobs     blob-like masks (a few soft discs per frame plus a little speckle), what a trained masker gives;
  speckled  the same discs under heavy speckle and with pinholes: many small components and many small holes;

for each single operation (hysteresis, opening, closing at radius 1 and 4, square and cross, hole filling at 16 and 4096 pixels) and
for a full spec, with and without `gated`.  Every case is timed beside cgs_objects_label on the same stack in the same run, in turns:
the ratio of the two is what the line is for, a time alone says little on a shared machine.  A warm-up call, then 5 timed calls by
device events around clean.clean / objects.label (which also allocate their outputs) and a window of 50 back-to-back calls per kernel.
No time here is a pass or fail condition.  One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_clean.py [--out profiles/clean_time.jsonl]
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
from cgs_amd import clean, objects  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402

REPEATS, WINDOW = 5, 50
CASES = (("threshold", dict()), ("hyst", dict(strong=0.8)), ("open1", dict(open=1)), ("open4", dict(open=4)),
         ("open4_cross", dict(open=4, shape="cross")), ("close1", dict(close=1)), ("close4", dict(close=4)),
         ("fill16", dict(fill=16)), ("fill4096", dict(fill=4096)), ("fill4096_conn4", dict(fill=4096, connectivity=4)),
         ("full", dict(strong=0.8, open=1, close=2, fill=16)), ("full_gated", dict(strong=0.8, open=1, close=2, fill=16, want_gated=True)))


def soft_blobs(n, rs, speckle, pinholes):
    ys, xs = np.mgrid[0:64, 0:64]
    out = np.full((n, 64, 64), 0.1, dtype=np.float32)
    for f in range(n):
        for _ in range(rs.randint(1, 5)):
            cy, cx, r = rs.uniform(0, 64), rs.uniform(0, 64), rs.uniform(3, 14)
            d = np.hypot(ys - cy, xs - cx)
            out[f] = np.maximum(out[f], np.where(d < r, np.where(d < r / 2, 0.9, 0.6), 0.1).astype(np.float32))
    out[rs.rand(n, 64, 64) < speckle] = 0.6
    out[rs.rand(n, 64, 64) < pinholes] = 0.1
    return out


def in_turns(fa, fb):
    """(ms of fa, ms of fb): REPEATS timed calls each, alternating, after one warm-up call of each."""
    fa(), fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(REPEATS):
        for ms, fn in zip(out, (fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    return out


def window_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(WINDOW):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / WINDOW


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_clean.py measures on the GPU; no GPU is visible")
    rs = np.random.RandomState(0)
    n = a.n
    stacks = (("blobs", soft_blobs(n, rs, 0.004, 0.0)), ("speckled", soft_blobs(n, rs, 0.08, 0.05)))
    stamp = {"n": n, "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = []
    for name, stack in stacks:
        dev = torch.from_numpy(stack).to("cuda")
        label = lambda: objects.label(dev, thresh=0.5, inclusive=True, max_objects=1, want_labels=False, want_mask=True)
        for case, kw in CASES:
            run = lambda: clean.clean(dev, thresh=0.5, inclusive=True, **kw)
            counts = run().counts.sum(dim=0).tolist()
            ms, label_ms = in_turns(run, label)
            win, label_win = window_ms(run), window_ms(label)
            med, label_med = float(np.median(ms)), float(np.median(label_ms))
            lines.append(json.dumps({"stack": name, "case": case, "spec": {k: v for k, v in kw.items() if k != "want_gated"},
                                     "gated": bool(kw.get("want_gated")), "counts": dict(zip(clean.COUNTS, counts)),
                                     "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                     "window_ms_per_call": round(win, 4), "us_per_frame": round(win * 1e3 / n, 4),
                                     "label_ms_median": round(label_med, 4), "label_window_ms_per_call": round(label_win, 4),
                                     "to_label": round(win / label_win, 3), **stamp}))
            print(lines[-1])
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
