"""Times the value of an object (cgs_objects_ablate and cgs_objects_select, csrc/objects_value.hip, and objects.value as a whole) on the
-eval stack size, 2450 frames of 64 x 64 with K = 64: tools/time_objects_track.py's drifting discs, labelled by objects.label, under
random frames.  Every figure stands beside a yardstick measured in the same run:

  ablate   the whole stack in one call of the C entry on a preallocated output, per fill and grow: ms, ns a row and bytes written a
           second -- beside a device-to-device copy of the same number of bytes (copy_ of a uint8 tensor: it also reads them).
  select   the C entry with every other object kept -- beside cgs_objects_label on the same stack.
  value    objects.value (fill low, grow 0, chunk_rows 2048) with the critic of fixture G1, host clock around a synchronise: the base
           pass, the host argmin, an ablate and a critic forward per chunk, the scatter -- beside the critic forward alone over the same
           rows in the same batches.

The kernel timings are one window of --calls calls between two device events; the variants alternate within a round and the median over
--rounds rounds is kept, after a warm-up call of every variant.  No target is fixed in advance.  One JSON line on stdout and, with --out
FILE, in FILE.

    python tools/time_objects_value.py [--out profiles/objects_value_time.jsonl]
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
import bench  # noqa: E402
from cgs_amd import _lib, engine, objects  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402
from time_objects_track import K, blob_stack  # noqa: E402
from time_objects_track_gap import window_ms  # noqa: E402

ROW_BYTES = 64 * 64 * 3
ABLATES = (("mean_g0", 2, 0), ("frame_g0", 1, 0), ("frame_g4", 1, 4))       # name, fill mode, grow
CHUNK_ROWS = 2048


def host_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects_value.py measures on the GPU; none is visible")
    rs = np.random.RandomState(0)
    n, dev = a.n, "cuda"
    masks = torch.from_numpy(np.ascontiguousarray(blob_stack(n, rs))).to(dev).view(torch.uint8)
    frames = torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).to(dev)
    res = objects.label(masks, max_objects=K, want_labels=True, want_mask=True)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(res.kept.clamp(0, K), 0)
    rows = int(offsets[-1])
    images = torch.empty((rows, 64, 64, 3), dtype=torch.uint8, device=dev)
    other = torch.empty_like(images)
    row_frame, row_label = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
    fill = frames[0].contiguous()

    def ablate(mode, grow):
        return lambda: _lib.call("cgs_objects_ablate", frames.data_ptr(), res.labels.data_ptr(), offsets.data_ptr(), n, 0, n, K, grow, mode,
                                 0, fill.data_ptr() if mode == 1 else None, 0, rows, images.data_ptr(), row_frame.data_ptr(),
                                 row_label.data_ptr(), stream())

    keep = torch.zeros((n, K), dtype=torch.uint8, device=dev)
    keep[:, ::2] = 1
    sel = {"labels": torch.empty_like(res.labels), "table": torch.empty_like(res.table), "kept": torch.empty_like(res.kept),
           "mask": torch.empty((n, 64, 64), dtype=torch.uint8, device=dev), "unscored": torch.empty(n, dtype=torch.int32, device=dev)}
    lab = {"labels": torch.empty_like(res.labels), "count": torch.empty((n, 2), dtype=torch.int32, device=dev), "table": torch.empty_like(res.table)}
    variants = {name: ablate(mode, grow) for name, mode, grow in ABLATES}
    variants["copy"] = lambda: other.copy_(images)
    variants["select"] = lambda: _lib.call(
        "cgs_objects_select", res.labels.data_ptr(), res.table.data_ptr(), res.kept.data_ptr(), keep.data_ptr(), n, 64, 64, K,
        sel["labels"].data_ptr(), sel["table"].data_ptr(), sel["kept"].data_ptr(), sel["mask"].data_ptr(), sel["unscored"].data_ptr(), stream())
    variants["label"] = lambda: _lib.call(
        "cgs_objects_label", masks.data_ptr(), _lib.OBJ_U8, 0.0, n, 64, 64, 8, 1, K, lab["labels"].data_ptr(), None, lab["count"].data_ptr(),
        lab["table"].data_ptr(), stream())
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(window_ms(fn, a.calls))
    med = {k: float(np.median(v)) for k, v in ms.items()}

    eng = engine.HourglassEngine(64, device=torch.device("cuda:0"), dropout=0.0)
    eng.load_state(*bench.g1_weights())
    infer = lambda X: eng.infer(X, want_mask=False)[0]
    holder = {}

    def whole():
        holder["val"] = objects.value(infer, frames, res.labels, res.kept, fill="low", grow=0, max_objects=K, chunk_rows=CHUNK_ROWS)

    whole()
    chunks = holder["val"].chunks
    spans = [(int(offsets[f0]), int(offsets[f1])) for f0, f1, _ in chunks]

    def critic_alone():
        for lo in range(0, n, CHUNK_ROWS):
            infer(frames[lo:lo + CHUNK_ROWS])
        for lo, hi in spans:
            infer(images[lo:hi])

    critic_alone()
    value_ms, critic_ms = [], []
    for _ in range(a.rounds):
        value_ms += host_ms(whole, 1)
        critic_ms += host_ms(critic_alone, 1)
    v, c = float(np.median(value_ms)), float(np.median(critic_ms))
    gbs = lambda t: round(rows * ROW_BYTES / (t * 1e-3) / 1e9, 1)
    row = {"case": "blob", "n": n, "max_objects": K, "rows": rows, "bytes_written": rows * ROW_BYTES, "calls_per_window": a.calls,
           "rounds": a.rounds, "ms": {k: round(x, 4) for k, x in med.items()},
           "ms_spread": {k: [round(min(x), 4), round(max(x), 4)] for k, x in ms.items()},
           "ablate": {name: {"ns_per_row": round(med[name] * 1e6 / rows, 1), "gb_written_per_s": gbs(med[name]),
                             "to_copy": round(med[name] / med["copy"], 3)} for name, _, _ in ABLATES},
           "copy_gb_written_per_s": gbs(med["copy"]), "select_to_label": round(med["select"] / med["label"], 3),
           "value": {"chunk_rows": CHUNK_ROWS, "chunks": len(chunks), "ms": round(v, 3), "ms_spread": [round(min(value_ms), 3), round(max(value_ms), 3)],
                     "critic_alone_ms": round(c, 3), "critic_alone_spread": [round(min(critic_ms), 3), round(max(critic_ms), 3)],
                     "to_critic_alone": round(v / c, 3), "images_per_s": round((rows + n) / (v * 1e-3))},
           "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
