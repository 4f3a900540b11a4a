"""Times the graph-cut kernel (csrc/graph_cut.hip) on the -eval stack size, 2450 frames of 64 x 64: blob-like soft masks (a few soft
discs per frame, what a trained masker gives) on textured frames whose objects have their own colour, read at 0.5 with the default
band.  Cases: it = 1 and it = 3 at conn 4 and conn 8, each at 16, 32 and 64 sweeps a round (cgs_graph_cut_sweeps: the result is the
same, `rounds` and the time are not).  Every case is timed beside cgs_dense_crf2 at the reference's parameters on the same stack in the
same run, in turns: the ratio of the two is what a line is for, a time alone says little on a shared machine.  A warm-up call, then 5
timed calls by device events around graphcut.cut / crf.dense_crf (which also allocate their outputs), and a window of back-to-back
calls per kernel.  scipy's Dinic (tests/graph_cut_ref.py, the whole rule on the host) is timed on a sample of the frames; where scipy
is missing that figure is "not measured".  Each line also holds the most rounds any frame took: the default max_rounds
(graphcut.MAX_ROUNDS) has to stay at least 8 times that.  No time here is a pass or fail condition.  One JSON line per case on stdout
and, with --out FILE, appended to FILE.

    python tools/time_graph_cut.py [--out profiles/graph_cut_time.jsonl] [--n 2450] [--host-sample 8]
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
from cgs_amd import crf, graphcut  # noqa: E402
from time_clean import in_turns, soft_blobs  # noqa: E402
from time_metrics import csrc_hash  # noqa: E402

WINDOW = 5
CASES = [(it, conn) for it in (1, 3) for conn in (4, 8)]
SWEEPS = (16, 32, 64)


def textured_frames(masks, rs):
    """uint8 [n,64,64,3]: a background colour and an object colour per frame, mixed by the soft mask, under texture noise."""
    n = len(masks)
    bg, fg = rs.randint(0, 256, (n, 1, 1, 3)), rs.randint(0, 256, (n, 1, 1, 3))
    m = (masks[..., None] > 0.5)
    return np.clip(np.where(m, fg, bg) + rs.randint(-35, 36, (n, 64, 64, 3)), 0, 255).astype(np.uint8)


def window_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(WINDOW):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / WINDOW


def host_ms_per_frame(frames, masks, sample, **kw):
    try:
        import graph_cut_ref
    except ImportError:
        return "not measured"
    t0 = time.perf_counter()
    for f, z in zip(frames[:sample], masks[:sample]):
        graph_cut_ref.cut_frame(f, z, 0.5, **kw)
    return round((time.perf_counter() - t0) * 1e3 / max(1, min(sample, len(frames))), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--host-sample", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_graph_cut.py measures on the GPU; no GPU is visible")
    rs = np.random.RandomState(0)
    n = a.n
    masks = soft_blobs(n, rs, 0.004, 0.0)
    masks = np.clip(masks + rs.normal(0, 0.12, masks.shape), 0, 1).astype(np.float32)       # soft edges: a band of unknown cells
    frames = textured_frames(masks, rs)
    dev_f, dev_z = torch.from_numpy(frames).to("cuda"), torch.from_numpy(masks).to("cuda")
    stamp = {"n": n, "csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    dense = lambda: crf.dense_crf(dev_f, dev_z)
    lines = []
    for it, conn in CASES:
        host = host_ms_per_frame(frames, masks, a.host_sample, iters=it, connectivity=conn) if a.host_sample else "not measured"
        for sweeps in SWEEPS:
            run = lambda: graphcut.cut(dev_f, dev_z, 0.5, iters=it, connectivity=conn, sweeps=sweeps)
            stats = run().stats.cpu().numpy().astype(np.int64)
            ms, crf_ms = in_turns(run, dense)
            win, crf_win = window_ms(run), window_ms(dense)
            lines.append(json.dumps({"case": f"it{it}_conn{conn}", "it": it, "conn": conn, "sweeps": sweeps,
                                     "report": {k: v for k, v in graphcut.cut_report(stats, {}).items() if k != "spec"},
                                     "rounds_max": int(stats[:, 2].max()), "rounds_mean": round(float(stats[:, 2].mean()), 3),
                                     "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                     "window_ms_per_call": round(win, 4), "us_per_frame": round(win * 1e3 / n, 4),
                                     "crf_ms_median": round(float(np.median(crf_ms)), 4), "crf_window_ms_per_call": round(crf_win, 4),
                                     "to_crf": round(win / crf_win, 3), "host_dinic_ms_per_frame": host,
                                     "host_to_gpu_per_frame": round(host * n / win, 1) if isinstance(host, float) else "not measured", **stamp}))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
