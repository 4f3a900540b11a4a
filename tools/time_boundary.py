"""Times the boundary kernel (csrc/boundary.hip) on the -eval stack size, 2450 frames of 64 x 64, for three pairs of mask stacks:

  blobs    a few discs per frame plus a little speckle as the truth, the same discs moved and resized a little as the prediction: what
           -eval --boundary-tol sees;
  empty    nothing on either side: no boundary pixel anywhere (every distance is the "none" value);
  checker  the checkerboard against its complement: every on pixel is a boundary pixel;

each at T = 1 (tolerance 1) and T = 16 (0, 0.5, ..., 7.5) tolerances, with and without `dist2` written.  Per case: the median of 5 timed
calls after a warm-up, device events around boundary.score (which also uploads the tolerances and allocates the outputs), and a window
of 50 back-to-back calls between two events divided by 50.  Beside each what a user does without the kernel: both stacks copied to the
host, then per frame and side one scipy.ndimage.distance_transform_edt of the complement of the boundary plus the numpy counts (wall
clock over --host-frames frames, scaled to the stack); without scipy, the checker of tests/boundary_ref.py takes its place (and says
so in "host").  host_to_kernel is the ratio of the two.  The blobs case is also compared with the checker on its first 8 frames.
One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_boundary.py [--out profiles/boundary_time.jsonl]
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
import boundary_ref  # noqa: E402
from cgs_amd import boundary  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402
from time_objects_match import blob_pair  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

TOLS = {1: (1,), 16: tuple(0.5 * k for k in range(16))}
WINDOW = 50


def host_counts(pred, truth, tol2):
    """One frame on the host: counts [4 + 4 T] as the kernel's, the distances from scipy's exact transform (or the checker's lists)."""
    if ndimage is None:
        return boundary_ref.score_frame(pred, truth, tol2)[0]
    bp, bt = boundary_ref.boundary(pred), boundary_ref.boundary(truth)
    none = np.full(pred.shape, -1, dtype=np.int64)
    dp = np.rint(ndimage.distance_transform_edt(~bp) ** 2).astype(np.int64) if bp.any() else none
    dt = np.rint(ndimage.distance_transform_edt(~bt) ** 2).astype(np.int64) if bt.any() else none
    both = bp.any() and bt.any()
    out = [int(bp.sum()), int(bt.sum()), int(dt[bp].max()) if both else -1, int(dp[bt].max()) if both else -1]
    for q in tol2:
        near_p, near_t = (dp <= q) & (dp >= 0), (dt <= q) & (dt >= 0)
        P, G = pred & near_p, truth & near_t
        out += [int((bp & near_t).sum()), int((bt & near_p).sum()), int((P & G).sum()), int((P | G).sum())]
    return np.array(out, dtype=np.int32)


def host_ms_per_stack(pred, truth, tol2, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, t = pred[:frames].cpu().numpy(), truth[:frames].cpu().numpy()
    rows = [host_counts(a, b, tol2) for a, b in zip(p, t)]
    return (time.perf_counter() - t0) * 1e3 * len(pred) / frames, np.stack(rows)


def window_ms(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    ap.add_argument("--host-frames", type=int, default=200)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n = a.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    bp, bt = blob_pair(n, rs)
    ys, xs = np.mgrid[0:64, 0:64]
    checker = np.broadcast_to((ys + xs) % 2 == 0, (n, 64, 64))
    stacks = (("blobs", up(bp), up(bt)), ("empty", up(np.zeros((n, 64, 64), dtype=bool)), up(np.zeros((n, 64, 64), dtype=bool))),
              ("checker", up(checker), up(~checker)))
    rows = []
    for name, pred, truth in stacks:
        for T, tol in TOLS.items():
            tol2 = boundary.tol_squared(tol)
            res = boundary.score(pred, truth, tol=tol)
            frames = min(a.host_frames, n)
            host, want = host_ms_per_stack(pred, truth, tol2, frames)
            got = torch.cat([torch.stack(res[:4], dim=1), torch.stack(res[4:8], dim=2).reshape(n, 4 * T)], dim=1)[:frames].cpu().numpy()
            if not np.array_equal(got, want):
                raise SystemExit(f"{name} T={T}: the kernel's counts differ from the host's")
            if name == "blobs":
                chk = boundary_ref.score(bp[:8], bt[:8], tol2)[0]
                if not np.array_equal(got[:8], chk):
                    raise SystemExit(f"{name} T={T}: the kernel's counts differ from the checker's")
            for want_dist2 in (False, True):
                fn = lambda: boundary.score(pred, truth, tol=tol, want_dist2=want_dist2)
                ms = device_ms(fn)
                win = window_ms(fn)
                med = float(np.median(ms))
                rows.append({"case": name, "n": n, "tolerances": T, "dist2": want_dist2,
                             "boundary_px_per_frame_mean": round(float((res.pred_px + res.truth_px).float().mean()), 1),
                             "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                             "ms_per_call_in_window_of_50": round(win, 4), "us_per_frame": round(med * 1e3 / n, 4),
                             "host": "scipy.ndimage.distance_transform_edt" if ndimage is not None else "tests/boundary_ref.py",
                             "host_frames": frames, "host_copy_edt_counts_ms": round(host, 1), "host_to_kernel": round(host / med, 1)})
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
