"""Times the saliency sweep kernel (csrc/saliency.hip) on the -eval stack size, 2450 frames of 64 x 64, at T = 1, 64 and 1024 thresholds
in both modes (global: -salglobal's default; frame: -salglobal ''), with counts (truth given) and no mask (which = -1); the one-threshold
case also as saliency.post (mask, no counts).  Median of 5 timed calls after a warm-up, device events around the entry point's call
(wrapper_ms_median: around saliency.sweep, which also checks the stack for negative values, builds and uploads the per-threshold arrays).

Beside each, the host path it replaces: Handler._saliency_post on the host copy and numpy `&` / `|` counts, once per threshold (wall
clock).  That path is linear in T, so it is timed on at most 4 thresholds of the grid and reported per threshold
(host_ms_per_threshold) and scaled to the grid (host_ms_for_T, marked extrapolated when T > 4).  The two paths are checked to give
the same counts on the thresholds that were run on the host.  One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_saliency.py [--out profiles/saliency_time.jsonl]
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
from cgs_amd import _lib, handler, saliency  # noqa: E402

REPEATS = 5
HOST_THRESHOLDS = 4


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


def host_counts(sal, preds, truth, thr, salglobal):
    out = []
    for t in thr:
        hard = handler.Handler._saliency_post(sal[:, None], preds, float(t), salglobal)[1][:, 0].astype(bool)
        out.append((np.count_nonzero(truth & hard), np.count_nonzero(truth | hard)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n, dev = a.n, "cuda"
    truth = np.zeros((n, 64, 64), dtype=bool)
    truth[:, 16:48, 8:40] = True
    sal = (rs.exponential(1e-4, (n, 64, 64)) * rs.lognormal(0.0, 0.5, (n, 1, 1))).astype(np.float32)      # as |gradient| sums are
    preds = rs.uniform(0.05, 1.0, n).astype(np.float32)
    mean = np.where(sal >= 0, sal, 0.0).mean()
    d_sal, d_preds, d_truth = torch.from_numpy(sal).to(dev), torch.from_numpy(preds).to(dev), torch.from_numpy(truth).to(dev)
    d_truth8 = d_truth.view(torch.uint8)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    rows = []
    for mode, salglobal in (("global", True), ("frame", False)):
        for T in (1, 64, 1024):
            thr = np.array([0.5]) if T == 1 else np.linspace(0.01, 0.99, T)
            d_thr = torch.from_numpy(thr).to(dev)
            d_g = torch.from_numpy((mean * thr.astype(np.float32)).astype(np.float32)).to(dev) if salglobal else None
            d_k = None if salglobal else torch.from_numpy(saliency.frame_k(thr).astype(np.int32)).to(dev)
            counts = torch.empty((T, 2), dtype=torch.int64, device=dev)
            scale = torch.empty((n, T), dtype=torch.float32, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None else None
            raw = lambda: _lib.call("cgs_saliency_sweep", d_sal.data_ptr(), d_preds.data_ptr(), d_truth8.data_ptr(), d_thr.data_ptr(),
                                    ptr(d_g), ptr(d_k), T, n, 64, 64, -1, counts.data_ptr(), scale.data_ptr(), None, stream())
            ms = device_ms(raw)
            wrapped = device_ms(lambda: saliency.sweep(d_sal, d_preds, d_truth, thr, salglobal, mean=mean if salglobal else None))
            some = np.unique(np.linspace(0, T - 1, min(T, HOST_THRESHOLDS)).astype(int))
            host_ms, want = [], None
            for _ in range(3):
                t0 = time.perf_counter()
                want = host_counts(sal, preds, truth, thr[some], salglobal)
                host_ms.append((time.perf_counter() - t0) * 1e3 / len(some))
            got = counts.cpu().numpy()[some]
            if got.tolist() != [list(w) for w in want]:
                raise SystemExit(f"{mode} T={T}: the kernel's counts differ from the host path's")
            per = float(np.median(host_ms))
            r = {"case": f"saliency_sweep_{mode}_T{T}", "n": n, "T": T, "ms_median": round(float(np.median(ms)), 4),
                 "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "wrapper_ms_median": round(float(np.median(wrapped)), 4),
                 "host_ms_per_threshold": round(per, 3), "host_ms_for_T": round(per * T, 1), "host_extrapolated": bool(T > len(some))}
            if T == 1:
                post = device_ms(lambda: saliency.post(d_sal, d_preds, 0.5, salglobal, mean=mean if salglobal else None))
                r["post_wrapper_ms_median"] = round(float(np.median(post)), 4)
            rows.append(r)
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
