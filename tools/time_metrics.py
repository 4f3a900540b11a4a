"""Times the evaluation scoring kernels (csrc/metrics.hip) on the -eval stack size, 2450 frames of 64 x 64:

  cgs_iou_curve at T = 1, 99 and 1024 thresholds, on uniform values and on bimodal ones (most pixels exactly 0 or 1);
  cgs_iou_counts for K = 1 and 8 label stacks;
  a 4-point CRF grid end to end through Handler.crf (upload, four cgs_dense_crf2 runs, four scores, the best labels back);

and beside each the same scoring the way Handler.get_iou does it: the stack copied to the host (.cpu().numpy()) and one numpy compare,
`&` and `|` per threshold / stack (wall clock; the stack is on the device when it is produced).  Median of 5 timed calls after a warm-up,
device events around the entry point's call (wrapper_ms_median: around metrics.iou_curve, which also sorts and uploads the thresholds).  bytes_read: 5 B per pixel for the curve (fp32 value + truth byte), (K + 1) B for the counts;
peak_fraction is bytes_read / time over 8 TB/s.  One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_metrics.py [--out profiles/metrics_time.jsonl]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cgs_amd import _lib, cli, handler, metrics  # noqa: E402

PEAK_BYTES_PER_S = 8e12
REPEATS = 5


def csrc_hash():
    d = os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fp:
            h.update(f.encode() + fp.read())
    return h.hexdigest()[:12]


def device_ms(fn):
    fn()                                            # warm-up (module load, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def wall_ms(fn):
    fn()
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def row(case, ms, host_ms, bytes_read=None, **extra):
    med = float(np.median(ms))
    r = {"case": case, **extra, "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
         "host_numpy_ms_median": round(float(np.median(host_ms)), 3)}
    if bytes_read is not None:
        r["bytes_read"] = int(bytes_read)
        r["peak_fraction"] = round(bytes_read / (med * 1e-3) / PEAK_BYTES_PER_S, 4)
    return r


def host_curve(dev_v, truth, thr):
    v = dev_v.cpu().numpy()
    return [(np.count_nonzero(truth & (v > t)), np.count_nonzero(truth | (v > t))) for t in thr]


def host_counts(dev_labels, truth):
    lab = dev_labels.cpu().numpy()
    return [(np.count_nonzero(truth & (m != 0)), np.count_nonzero(truth | (m != 0))) for m in lab]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n, dev = a.n, "cuda"
    px = n * 64 * 64
    truth = np.zeros((n, 64, 64), dtype=bool)
    truth[:, 16:48, 8:40] = True
    dev_truth = torch.from_numpy(truth).to(dev)
    uniform = rs.uniform(0, 1, (n, 64, 64)).astype(np.float32)
    bimodal = (rs.rand(n, 64, 64) < 0.2).astype(np.float32)
    soft = rs.rand(n, 64, 64) < 0.02                               # a thin band of in-between values, as a trained mask's edges
    bimodal[soft] = rs.uniform(0, 1, int(soft.sum())).astype(np.float32)
    rows = []
    for name, v in (("uniform", uniform), ("bimodal", bimodal)):
        dev_v = torch.from_numpy(v).to(dev)
        for T in (1, 99, 1024):
            thr = np.array([0.05], dtype=np.float32) if T == 1 else np.linspace(0.001, 0.999, T).astype(np.float32)
            dev_thr = torch.from_numpy(thr).to(dev)                # ascending already: the entry point itself, without the wrapper
            counts = torch.empty((T, 2), dtype=torch.int64, device=dev)
            raw = lambda: _lib.call("cgs_iou_curve", dev_v.data_ptr(), dev_truth.data_ptr(), dev_thr.data_ptr(), T, 0, px,
                                    counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            wrapped = device_ms(lambda: metrics.iou_curve(dev_v, dev_truth, thr))      # + threshold sort / upload, result reorder
            rows.append(row(f"iou_curve_{name}_T{T}", device_ms(raw), wall_ms(lambda: host_curve(dev_v, truth, thr)),
                            bytes_read=5 * px, n=n, T=T, wrapper_ms_median=round(float(np.median(wrapped)), 4)))
    for K in (1, 8):
        dev_labels = torch.from_numpy((rs.rand(K, n, 64, 64) < 0.3).astype(np.uint8)).to(dev)
        rows.append(row(f"iou_counts_K{K}", device_ms(lambda: metrics.iou_counts(dev_labels, dev_truth)),
                        wall_ms(lambda: host_counts(dev_labels, truth)), bytes_read=(K + 1) * px, n=n, K=K))

    # the 4-point grid end to end (wall clock on both sides: uploads, four CRF runs, scoring, labels back); the host side scores the
    # same four label stacks the way the reference does, each pulled to the host first
    frames = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    H = handler.Handler(cli.parse_args(["--model", "unused", "-eval", "-crf", "--crf-grid", "w1=5,22;it=2,10"]))
    H.rank = 1                                                     # no debug PNGs
    grid_ms = wall_ms(lambda: H.crf(frames, uniform[:, None], truth))
    H0 = handler.Handler(cli.parse_args(["--model", "unused"]))
    H0.rank = 1
    one_ms = wall_ms(lambda: H0.crf(frames, uniform[:, None], truth))
    dev_labels = torch.from_numpy((rs.rand(4, n, 64, 64) < 0.3).astype(np.uint8)).to(dev)
    rows.append(row("crf_grid_4_points_end_to_end", grid_ms, wall_ms(lambda: host_counts(dev_labels, truth)), n=n, points=4,
                    one_point_ms_median=round(float(np.median(one_ms)), 3)))
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
