"""Times motion-compensated tracking (cgs_objects_track_mc, csrc/objects_track.hip) against the uncompensated tracker of the same build
on the -eval stack size, 2450 frames of 64 x 64 with K = 64, on the blob stack of tools/time_objects_track.py and the flickering stack of
tools/time_objects_track_gap.py.

In one run, on the same stack, on preallocated outputs and scratch (the C entries themselves, no allocation inside the timed window):
cgs_objects_track (G = 0) or cgs_objects_track_gap (G = 8) without motion, and cgs_objects_track_mc at the same G along an all-zero field
(the same links, so the same work after the counting: the difference is the staging and the gather) and along a random field within
+-4 cells.  A timing is one window of --calls calls between two device events; the variants alternate within a round and the median over
--rounds rounds is kept, after a warm-up call of every variant.  The zero field's outputs are checked against the uncompensated entry
bit for bit before anything is timed.  No ratio is fixed in advance: mc_to_plain = ms of the motion entry / ms of the plain one.  The
vectors' own time is stated separately: cgs_temporal_flow at search 4 over 2450 random frames, in microseconds per frame pair.

  pan   a synthetic panning, flickering stack: blobs of 5 x 5 cells on a wide canvas, 16 cells apart, seen through a window that moves 3
        cells a frame (10 / 40 between neighbouring frames, below the link IoU), each blob absent from about a third of its frames.  The number of tracks without motion and along the true field
        (0, -3), at G = 0 and G = 8.

One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_objects_track_mc.py [--out profiles/objects_track_mc_time.jsonl]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cgs_amd import _lib, objects, temporal  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402
from time_objects_track import IOU, K, blob_stack  # noqa: E402
from time_objects_track_gap import Entry, flicker_stack, window_ms  # noqa: E402

GAPS = (0, 8)
SEARCH = 4


class MotionEntry(Entry):
    """cgs_objects_track_mc on its own buffers."""

    def __init__(self, labels, gap, bwd):
        super().__init__(labels, gap)
        self.bwd = bwd

    def __call__(self):
        o, n = self.out, self.n
        _lib.call("cgs_objects_track_mc", self.labels.data_ptr(), self.bwd.data_ptr(), n, 64, 64, K, round(IOU * 1000), self.gap, n * K,
                  o["prev"].data_ptr(), o["gap"].data_ptr(), o["track"].data_ptr(), o["totals"].data_ptr(), o["gap_links"].data_ptr(),
                  o["table"].data_ptr(), o["extra"].data_ptr(), None, None, self.scratch.data_ptr(), self.scratch.numel() * 8,
                  torch.cuda.current_stream().cuda_stream)


def pan_stack(n, rs, step=3, pitch=16, cell=5):
    """int32 [n,64,64]: blobs on a canvas 64 + step (n - 1) cells wide, one per cell of a grid of `pitch`, seen through a window that
    moves so that the content moves `step` cells a frame along x; a blob is absent from about a third of its frames.  A blob's label
    is (its column mod 8) * 4 + its row + 1: the window holds at most 5 columns, so the labels of a frame are distinct."""
    width = 64 + step * (n - 1)
    cols, rows = width // pitch + 1, 64 // pitch
    there = rs.rand(n, rows, cols) >= 1 / 3
    s = np.zeros((n, 64, 64), dtype=np.int32)
    for f in range(n):
        off = step * (n - 1 - f)                                           # the window's first canvas column
        for c in range(off // pitch - 1, (off + 64) // pitch + 1):
            x = c * pitch + 4 - off
            if c < 0 or c >= cols or x + cell <= 0 or x >= 64:
                continue
            for r in range(rows):
                if there[f, r, c]:
                    s[f, r * pitch + 4:r * pitch + 4 + cell, max(x, 0):min(x + cell, 64)] = (c % 8) * rows + r + 1
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects_track_mc.py measures on the GPU; none is visible")
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    zero = torch.zeros((n - 1, 8, 8, 2), dtype=torch.int8, device="cuda")
    within = up(rs.randint(-SEARCH, SEARCH + 1, (n - 1, 8, 8, 2)).astype(np.int8))
    rows = []
    for name, labels in (("blobs", objects.label(up(blob_stack(n, rs))).labels), ("flicker", up(flicker_stack(n, rs)))):
        variants = {}
        for g in GAPS:
            variants[f"plain{g}"] = Entry(labels, g if g else None)
            variants[f"mc{g}_zero"] = MotionEntry(labels, g, zero)
            variants[f"mc{g}_within{SEARCH}"] = MotionEntry(labels, g, within)
        for fn in variants.values():                                        # warm-up of every variant
            fn()
        torch.cuda.synchronize()
        for g in GAPS:                                                      # a zero field is the uncompensated tracker
            for key in variants[f"plain{g}"].out:
                assert torch.equal(variants[f"mc{g}_zero"].out[key], variants[f"plain{g}"].out[key]), (g, key)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window_ms(fn, a.calls))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = {"case": name, "n": n, "max_objects": K, "track_iou": IOU, "calls_per_window": a.calls, "rounds": a.rounds,
               "objects": int(variants["plain0"].out["totals"][2]),
               "tracks": {k: int(v.out["totals"][0]) for k, v in variants.items()},
               "ms": {k: round(v, 4) for k, v in med.items()}, "ms_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
        for g in GAPS:
            row[f"mc_to_plain_g{g}_zero"] = round(med[f"mc{g}_zero"] / med[f"plain{g}"], 3)
            row[f"mc_to_plain_g{g}_within{SEARCH}"] = round(med[f"mc{g}_within{SEARCH}"] / med[f"plain{g}"], 3)
        rows.append(row)

    low = up(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8))
    fwd, bwd = temporal.flow(low, SEARCH)
    flow = lambda: _lib.call("cgs_temporal_flow", low.data_ptr(), n, SEARCH, fwd.data_ptr(), bwd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    flow()
    torch.cuda.synchronize()
    flow_ms = [window_ms(flow, a.calls) for _ in range(a.rounds)]
    rows.append({"case": "flow", "n": n, "search": SEARCH, "ms": round(float(np.median(flow_ms)), 4),
                 "us_per_pair": round(1000 * float(np.median(flow_ms)) / (n - 1), 4)})

    pan = up(pan_stack(n, rs))
    true = torch.zeros((n - 1, 8, 8, 2), dtype=torch.int8, device="cuda")
    true[..., 1] = -3
    counts = {}
    for g in GAPS:
        counts[f"plain{g}"] = int(objects.track(pan, iou=IOU, max_objects=K, max_gap=g).n_tracks)
        counts[f"mc{g}"] = int(objects.track(pan, iou=IOU, max_objects=K, max_gap=g, motion=true).n_tracks)
    rows.append({"case": "pan", "n": n, "step": 3, "track_iou": IOU, "objects": int(objects.track(pan, iou=IOU, max_objects=K).n_objects),
                 "tracks": counts})

    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
