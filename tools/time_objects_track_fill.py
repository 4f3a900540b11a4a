"""Times the fill of bridged tracks (cgs_objects_track_fill, csrc/objects_fill.hip) beside the tracker call whose links it fills, on the
-eval stack size, 2450 frames of 64 x 64 with K = 64.  The tracker's kernels are not touched by the fill, so the tracker is the
yardstick: fill_to_track = ms of the fill / ms of the tracker with the same G and field, on the same stack, in the same run.

  flicker  tools/time_objects_track_gap.py's flickering stack, each frame renumbered 1..count in raster order as objects.label numbers
           a frame (with the grid's own numbers a frame's largest label is nearly always 64 and the fill has no label left to give).
           Without a field (cgs_objects_track_gap and the fill with bwd NULL) and along an all-zero field (cgs_objects_track_mc and the
           fill's staged path: the same links and the same masks, so the difference is the staging and the walk).
  pan      tools/time_objects_track_mc.py's panning, flickering stack along its true field (0, -3).

G = 1 and 8.  Everything runs on preallocated outputs (the C entries themselves, no allocation inside the timed window).  A timing is one
window of --calls calls between two device events; the variants alternate within a round and the median over --rounds rounds is kept,
after a warm-up call of every variant.  The fill along the zero field is checked against the fill without a field bit for bit before
anything is timed.  Per stack and G the line also holds the objects before and after the fill, the fill's four counts, and filled_share
= new objects / the tracks' missed frames (every new object is one missed frame of one track that got a mask).  No ratio is fixed in
advance.  One JSON line per stack on stdout and, with --out FILE, in FILE.

    python tools/time_objects_track_fill.py [--out profiles/objects_track_fill_time.jsonl]
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
from cgs_amd import _lib  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402
from time_objects_track import IOU, K  # noqa: E402
from time_objects_track_gap import Entry, flicker_stack, window_ms  # noqa: E402
from time_objects_track_mc import MotionEntry, pan_stack  # noqa: E402

GAPS = (1, 8)


class FillEntry:
    """cgs_objects_track_fill on its own buffers, reading the outputs of a tracker entry."""

    def __init__(self, tracker, bwd=None):
        labels = tracker.labels
        n, dev = labels.shape[0], labels.device
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        self.labels, self.tracker, self.bwd, self.n = labels, tracker, bwd, n
        self.out = {"labels": new(n, 64, 64), "track": new(n, K), "age": new(n, K), "table": new(n, K, 8), "totals": new(4)}

    def __call__(self):
        o, t = self.out, self.tracker.out
        _lib.call("cgs_objects_track_fill", self.labels.data_ptr(), None if self.bwd is None else self.bwd.data_ptr(), self.n, 64, 64, K,
                  self.tracker.gap, t["prev"].data_ptr(), t["gap"].data_ptr(), t["track"].data_ptr(), o["labels"].data_ptr(),
                  o["track"].data_ptr(), o["age"].data_ptr(), o["table"].data_ptr(), o["totals"].data_ptr(),
                  torch.cuda.current_stream().cuda_stream)


def renumber(stack):
    """Every frame's labels replaced by their rank among the labels the frame holds: 1..count."""
    out = np.zeros_like(stack)
    for f, frame in enumerate(stack):
        present = np.unique(frame[frame > 0])
        lut = np.zeros(int(stack.max()) + 1, dtype=stack.dtype)
        lut[present] = np.arange(1, len(present) + 1)
        out[f] = lut[frame]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects_track_fill.py measures on the GPU; none is visible")
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    zero = torch.zeros((n - 1, 8, 8, 2), dtype=torch.int8, device="cuda")
    true = torch.zeros((n - 1, 8, 8, 2), dtype=torch.int8, device="cuda")
    true[..., 1] = -3
    rows = []
    for name, labels, fields in (("flicker", up(renumber(flicker_stack(n, rs))), {"none": None, "zero": zero}),
                                 ("pan", up(pan_stack(n, rs)), {"true": true})):
        variants = {}
        for g in GAPS:
            for fname, field in fields.items():
                tracker = Entry(labels, g) if field is None else MotionEntry(labels, g, field)
                variants[f"track{g}_{fname}"] = tracker
                variants[f"fill{g}_{fname}"] = FillEntry(tracker, field)
        for fn in variants.values():                                        # warm-up of every variant; a fill runs behind its tracker
            fn()
        torch.cuda.synchronize()
        if "zero" in fields:                                                # a zero field is no field
            for g in GAPS:
                for key, t in variants[f"fill{g}_none"].out.items():
                    assert torch.equal(variants[f"fill{g}_zero"].out[key], t), (g, key)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window_ms(fn, a.calls))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = {"case": name, "n": n, "max_objects": K, "track_iou": IOU, "calls_per_window": a.calls, "rounds": a.rounds,
               "ms": {k: round(v, 4) for k, v in med.items()}, "ms_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
        first = next(iter(fields))
        for g in GAPS:
            t, f = variants[f"track{g}_{first}"].out, variants[f"fill{g}_{first}"].out
            made, cells, dropped, vanished = f["totals"].tolist()
            missed = int(t["extra"][:, 1].sum())
            row[f"g{g}"] = {"tracks": int(t["totals"][0]), "objects_before": int(t["totals"][2]), "objects_after": int(t["totals"][2]) + made,
                            "missed_frames": missed, "filled_objects": made, "filled_cells": cells, "dropped": dropped, "vanished": vanished,
                            "filled_share": round(made / missed, 4) if missed else None}
            for fname in fields:
                row[f"fill_to_track_g{g}_{fname}"] = round(med[f"fill{g}_{fname}"] / med[f"track{g}_{fname}"], 3)
        rows.append(row)
        print(f"{name}: " + "; ".join(f"G={g}: {row[f'g{g}']['objects_before']} objects -> {row[f'g{g}']['objects_after']}, "
                                       f"{row[f'g{g}']['filled_objects']} of {row[f'g{g}']['missed_frames']} missed frames filled "
                                       f"({row[f'g{g}']['filled_share']})" for g in GAPS), file=sys.stderr)
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
