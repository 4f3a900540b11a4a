"""Times tracking across gaps (cgs_objects_track_gap, csrc/objects_track.hip) against the adjacent tracker on the -eval stack size,
2450 frames of 64 x 64 with K = 64: the three stacks of tools/time_objects_track.py (blobs, full, strips) and

  flicker  an 8 x 8 grid of blobs, each shifted by -1..1 pixels a frame and absent from about a third of its frames: every level has
           open tails and open heads in nearly every frame pair, which is what the level kernel is for.

In one run, on preallocated outputs and scratch (the C entries themselves, no allocation inside the timed window): cgs_objects_match
on the n - 1 neighbouring pairs plus the self-pair (the counting of the adjacent pass; its link kernel cannot be launched alone),
cgs_objects_track, and cgs_objects_track_gap at G = 0, 1, 2, 4, 8.  A timing is one window of --calls calls between two device events;
the variants alternate within a round and the median over --rounds rounds is kept, after a warm-up call of every variant.  Per stack:
ms per call of each, per_level_ms = (gap_G - gap_0) / G and level_to_match = per_level_ms / match_ms.  G = 0 through the new entry is
checked against cgs_objects_track bit for bit before anything is timed.  One JSON line per stack on stdout and, with --out FILE, in
FILE.

    python tools/time_objects_track_gap.py [--out profiles/objects_track_gap_time.jsonl]
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
from time_objects_track import IOU, K, blob_stack, pairs  # noqa: E402

GAPS = (0, 1, 2, 4, 8)


def flicker_stack(n, rs, cell=8):
    """int32 [n,64,64]: label i + 1 is the blob of grid cell i wherever it shows."""
    per = 64 // cell
    s = np.zeros((n, 64 + 2, 64 + 2), dtype=np.int32)
    there = rs.rand(n, per * per) >= 1 / 3
    dy, dx = rs.randint(-1, 2, (n, per * per)), rs.randint(-1, 2, (n, per * per))
    for f in range(n):
        for i in np.flatnonzero(there[f]):
            y, x = 1 + (i // per) * cell + dy[f, i], 1 + (i % per) * cell + dx[f, i]
            s[f, y:y + cell, x:x + cell] = i + 1
    return np.ascontiguousarray(s[:, 1:-1, 1:-1])


class Entry:
    """One of the two C entries on its own buffers."""

    def __init__(self, labels, gap=None):
        n, dev = labels.shape[0], labels.device
        lib = _lib.load()
        need = lib.cgs_objects_track_scratch_bytes(n, K) if gap is None else lib.cgs_objects_track_gap_scratch_bytes(n, K, gap)
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        self.labels, self.gap, self.n = labels, gap, n
        self.out = {"prev": new(n, K), "track": new(n, K), "totals": new(4), "table": new(n * K, 8)}
        if gap is not None:
            self.out.update(gap=new(n, K), gap_links=new(gap + 1), extra=new(n * K, 2))
        self.scratch = torch.empty((int(need) + 7) // 8, dtype=torch.int64, device=dev)

    def __call__(self):
        o, n = self.out, self.n
        tail = (None, None, self.scratch.data_ptr(), self.scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
        if self.gap is None:
            _lib.call("cgs_objects_track", self.labels.data_ptr(), n, 64, 64, K, round(IOU * 1000), n * K, o["prev"].data_ptr(),
                      o["track"].data_ptr(), o["totals"].data_ptr(), o["table"].data_ptr(), *tail)
        else:
            _lib.call("cgs_objects_track_gap", self.labels.data_ptr(), n, 64, 64, K, round(IOU * 1000), self.gap, n * K, o["prev"].data_ptr(),
                      o["gap"].data_ptr(), o["track"].data_ptr(), o["totals"].data_ptr(), o["gap_links"].data_ptr(), o["table"].data_ptr(),
                      o["extra"].data_ptr(), *tail)


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects_track_gap.py measures on the GPU; none is visible")
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    tile = lambda frame: up(np.broadcast_to(frame, (n, 64, 64)).astype(np.int32))
    strips = (np.arange(4096, dtype=np.int32) // 64 + 1).reshape(64, 64)
    stacks = (("blobs", objects.label(up(blob_stack(n, rs))).labels), ("full", tile(np.ones((64, 64)))), ("strips", tile(strips)),
              ("flicker", up(flicker_stack(n, rs))))
    rows = []
    for name, labels in stacks:
        buffers = pairs(labels)
        variants = {"match": lambda: pairs(labels, buffers), "track": Entry(labels)}
        variants.update({f"gap{g}": Entry(labels, g) for g in GAPS})
        for fn in variants.values():                                        # warm-up of every variant
            fn()
        torch.cuda.synchronize()
        for key in ("prev", "track", "totals", "table"):                    # G = 0 is the adjacent tracker
            assert torch.equal(variants["gap0"].out[key], variants["track"].out[key]), key
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window_ms(fn, a.calls))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        top = variants[f"gap{GAPS[-1]}"].out
        row = {"case": name, "n": n, "max_objects": K, "track_iou": IOU, "calls_per_window": a.calls, "rounds": a.rounds,
               "tracks_by_gap": {str(g): int(variants[f"gap{g}"].out["totals"][0]) for g in GAPS},
               "links_by_gap_at_8": top["gap_links"].tolist(), "objects": int(top["totals"][2]),
               "ms": {k: round(v, 4) for k, v in med.items()}, "ms_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
        for g in GAPS[1:]:
            per_level = (med[f"gap{g}"] - med["gap0"]) / g
            row[f"per_level_ms_g{g}"] = round(per_level, 4)
            row[f"level_to_match_g{g}"] = round(per_level / med["match"], 3)
        rows.append(row)
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
