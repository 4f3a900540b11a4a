"""Times the identity layer on top of the tracks (cgs_objects_appearance and cgs_objects_reid, csrc/objects_reid.hip) beside the tracker
call whose tracks it chains, on the -eval stack size, 2450 frames of 64 x 64 with K = 64.  The tracker's kernels are not touched, so the
tracker is the yardstick: appearance_to_track and reid_to_track = ms of the entry / ms of the tracker with the same G on the same stack
in the same run.

  flicker  tools/time_objects_track_gap.py's flickering stack; a blob's colour is a palette colour chosen by its grid cell, +-20 noise.
  blob     tools/time_objects_track.py's drifting discs, labelled by objects.label; every pixel a random palette colour.
  pan      tools/time_objects_track_mc.py's panning, flickering stack; a blob's colour is a palette colour chosen by its label.

G = 0 and 8; W = 16, 64 and 256 at the default threshold 0.8 and area 64.  Everything runs on preallocated outputs (the C entries
themselves, no allocation inside the timed window).  A timing is one window of --calls calls between two device events; the variants
alternate within a round and the median over --rounds rounds is kept, after a warm-up call of every variant.  Per stack and G the line
also holds the tracks before and the eligible tracks, links, identities and the longest chain after, per W.  No ratio is fixed in advance.
One JSON line per stack on stdout and, with --out FILE, in FILE.

    python tools/time_objects_reid.py [--out profiles/objects_reid_time.jsonl]
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
from cgs_amd import _lib, objects  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402
from time_objects_track import IOU, K, blob_stack  # noqa: E402
from time_objects_track_gap import Entry, flicker_stack, window_ms  # noqa: E402
from time_objects_track_mc import pan_stack  # noqa: E402

GAPS = (0, 8)
WINDOWS = (16, 64, 256)
SIM, AREA = 0.8, 64
PALETTE = np.array([(32 + 64 * r, 32 + 64 * g, 32 + 64 * b) for r in (0, 3) for g in (0, 2, 3) for b in (0, 1, 3)], dtype=np.int64)


class AppearanceEntry:
    """cgs_objects_appearance (track histograms only) on its own buffer, reading the track numbers of a tracker entry."""

    def __init__(self, tracker, frames):
        self.tracker, self.frames, self.n = tracker, frames, tracker.n
        self.S = torch.empty((self.n * K, 64), dtype=torch.int32, device=frames.device)

    def __call__(self):
        _lib.call("cgs_objects_appearance", self.frames.data_ptr(), self.tracker.labels.data_ptr(), self.tracker.out["track"].data_ptr(),
                  self.n, 64, 64, K, self.n * K, self.S.data_ptr(), None, torch.cuda.current_stream().cuda_stream)


class ReidEntry:
    """cgs_objects_reid on its own buffers, reading an appearance entry's histograms and its tracker's table."""

    def __init__(self, appearance, window):
        t = appearance.tracker
        n, dev = t.n, appearance.S.device
        rows = n * K
        self.appearance, self.window, self.n, self.rows = appearance, window, n, rows
        self.out = torch.empty((4, rows), dtype=torch.int32, device=dev)
        self.totals = torch.empty(4, dtype=torch.int32, device=dev)
        self.Q = torch.empty((rows, 64), dtype=torch.int16, device=dev)
        need = int(_lib.load().cgs_objects_reid_scratch_bytes(n, rows))
        self.scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)

    def __call__(self):
        t, o = self.appearance.tracker.out, self.out
        extra = t.get("extra")
        _lib.call("cgs_objects_reid", self.appearance.S.data_ptr(), t["table"].data_ptr(), None if extra is None else extra.data_ptr(),
                  t["totals"].data_ptr(), self.n, self.rows, round(SIM * 1000), self.window, AREA, o[0].data_ptr(), o[1].data_ptr(),
                  o[2].data_ptr(), o[3].data_ptr(), self.totals.data_ptr(), self.Q.data_ptr(), self.scratch.data_ptr(),
                  self.scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)


def coloured(labels, rs, by_label=True):
    """uint8 [n,64,64,3] for an int32 label stack: a palette colour per label with +-20 noise, or a random palette colour per pixel."""
    pick = labels % len(PALETTE) if by_label else rs.randint(0, len(PALETTE), labels.shape)
    noise = rs.randint(-20, 21, labels.shape + (3,)) if by_label else 0
    return (PALETTE[pick] + noise).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects_reid.py measures on the GPU; none is visible")
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    blobs = objects.label(up(blob_stack(n, rs)), max_objects=K).labels.cpu().numpy()
    rows = []
    for name, labels, by_label in (("flicker", flicker_stack(n, rs), True), ("blob", blobs, False), ("pan", pan_stack(n, rs), True)):
        frames, labels = up(coloured(labels, rs, by_label)), up(labels)
        variants = {}
        for g in GAPS:
            tracker = Entry(labels, g)
            variants[f"track{g}"] = tracker
            variants[f"appearance{g}"] = shared = AppearanceEntry(tracker, frames)
            for w in WINDOWS:
                variants[f"reid{g}_w{w}"] = ReidEntry(shared, w)
        for fn in variants.values():                                        # warm-up of every variant, each behind what it reads
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window_ms(fn, a.calls))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = {"case": name, "n": n, "max_objects": K, "track_iou": IOU, "sim": SIM, "min_area": AREA, "pair_pass": "lane per candidate",
               "calls_per_window": a.calls, "rounds": a.rounds, "ms": {k: round(v, 4) for k, v in med.items()},
               "ms_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
        for g in GAPS:
            tracks = int(variants[f"track{g}"].out["totals"][0])
            row[f"g{g}"] = {"tracks": tracks, "appearance_to_track": round(med[f"appearance{g}"] / med[f"track{g}"], 3)}
            for w in WINDOWS:
                identities, links, eligible, longest = variants[f"reid{g}_w{w}"].totals.tolist()
                row[f"g{g}"][f"w{w}"] = {"eligible": eligible, "links": links, "identities": identities, "longest": longest,
                                         "reid_to_track": round(med[f"reid{g}_w{w}"] / med[f"track{g}"], 3)}
        rows.append(row)
        print(f"{name}: " + "; ".join(f"G={g}: {row[f'g{g}']['tracks']} tracks -> " + ", ".join(
            f"{row[f'g{g}'][f'w{w}']['identities']} identities at W={w}" for w in WINDOWS) for g in GAPS), file=sys.stderr)
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
