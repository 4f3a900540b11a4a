"""Times the two kernels of -process --source-video --smooth R --smooth-motion S (csrc/temporal_motion.hip) beside the filter they extend
(csrc/temporal.hip), all in one run.

  flow        cgs_temporal_flow at search 1 / 2 / 4 over 4096 frames of 64 x 64, in microseconds per frame pair.  "bytes" is what the kernel
              moves, counted from the shapes: each frame's 12 KB read by the two pairs it belongs to, 256 bytes of vectors written a pair.
              "gsad_per_s" counts one packed absolute-difference sum per cell, candidate and direction, border candidates included.
  smooth      cgs_temporal_smooth at radius 1 / 3 / 8 over the same frames: the yardstick, unchanged.
  smooth_mc   cgs_temporal_smooth_mc at the same radii along the vectors of search 4, and, at radius 3, along an all-zero field (the taps
              of the plain filter: what the path look-ups and the bounded addresses cost on their own).  "ratio_to_smooth" is its time
              over the plain filter's of the same radius, from this run.

The C entry points are called on preallocated outputs, so a figure is the kernel and its launch, not the allocator.  Per case the median
of 5 timed calls after a warm-up, device events around each call, and a window of 50 back-to-back calls between two events divided by
50; the three kinds are timed in turns, radius by radius, so that a drift of the machine touches them alike.  Before timing, the vectors
are compared with tests/temporal_motion_ref.py on 4 frames, the filter with float64 on 8 frames, and the all-zero field with the plain
filter bit for bit.  One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_temporal_motion.py [--out profiles/temporal_motion_time.jsonl]
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
import temporal_motion_ref  # noqa: E402
from cgs_amd import _lib, temporal  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402
from time_overlay import window_ms  # noqa: E402


def panned(n, rs, step=3):
    """A blocky scene under a pan of `step` cells a frame along x, n frames long (the pan wraps every 64 frames), +-6 colour noise and
    +-0.05 noise on z: (z float32 [n,64,64], low uint8 [n,64,64,3])."""
    colour = np.repeat(np.repeat(rs.randint(0, 256, (8, 30, 3)), 9, axis=0), 9, axis=1)
    value = np.repeat(np.repeat(rs.rand(8, 30), 9, axis=0), 9, axis=1)
    at = [192 - step * (f % 64) for f in range(n)]
    low = np.stack([colour[3:67, x:x + 64] for x in at])
    z = np.stack([value[3:67, x:x + 64] for x in at])
    low = np.clip(low + rs.randint(-6, 7, low.shape), 0, 255).astype(np.uint8)
    return np.clip(z + rs.uniform(-0.05, 0.05, z.shape), 0.0, 1.0).astype(np.float32), low


def figures(case, ms, win, n, nbytes, **extra):
    return {"case": case, **extra, "n": n, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "ms_per_call_in_window": round(win, 4), "us_per_frame": round(win * 1e3 / n, 3),
            "bytes": int(nbytes), "tb_per_s": round(nbytes / win / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_temporal_motion.py measures on the GPU: none is visible")
    rs = np.random.RandomState(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n = a.frames
    zs, ls = panned(n, rs)
    zd, ld = torch.from_numpy(zs).to("cuda"), torch.from_numpy(ls).to("cuda")
    od = torch.empty_like(zd)
    fwd = torch.empty((n - 1, 8, 8, 2), dtype=torch.int8, device="cuda")
    bwd = torch.empty_like(fwd)
    zero = torch.zeros_like(fwd)

    # ---- the checks
    got = temporal.flow(ld[:4], 4)
    for g, w in zip(got, temporal_motion_ref.flow_ref(ls[:4], 4)):
        if not np.array_equal(g.cpu().numpy(), w):
            raise SystemExit("the vectors differ from the checker")
    m8 = temporal.flow(ld[:8], 4)
    want = temporal_motion_ref.smooth_mc_ref(zs[:8], ls[:8], m8[0].cpu().numpy(), m8[1].cpu().numpy(), 3, 16.0)
    err = float(np.abs(temporal.smooth(zd[:8], ld[:8], 3, motion=m8).cpu().numpy().astype(np.float64) - want).max())
    if err > 2.7e-5:
        raise SystemExit(f"the filter along the motion differs from float64 by {err:.2e}")
    if not torch.equal(temporal.smooth(zd[:64], ld[:64], 3, motion=(zero[:63], zero[:63])), temporal.smooth(zd[:64], ld[:64], 3)):
        raise SystemExit("an all-zero field does not give the plain filter bit for bit")

    rows = []
    # ---- the vectors
    for search in (1, 2, 4):
        fn = lambda: _lib.call("cgs_temporal_flow", ld.data_ptr(), n, search, fwd.data_ptr(), bwd.data_ptr(), stream())
        r = figures("flow", device_ms(fn), window_ms(fn), n - 1, (n - 1) * (2 * 64 * 64 * 3 + 2 * 128), search=search)
        r["gsad_per_s"] = round((n - 1) * 2 * 4096 * (2 * search + 1) ** 2 / r["ms_per_call_in_window"] / 1e6, 1)
        rows.append(r)
    sat = float((fwd.abs().amax(dim=-1) >= 4).double().mean())      # (of search 4, the last one timed: the field the filter follows below)
    found = float((fwd == torch.tensor([0, 3], dtype=torch.int8, device="cuda")).all(dim=-1).double().mean())

    # ---- the filter without and with the motion, in turns
    for radius in (1, 3, 8):
        plain = lambda: _lib.call("cgs_temporal_smooth", zd.data_ptr(), ld.data_ptr(), n, 0, n, radius, 16.0, od.data_ptr(), stream())
        along = lambda f, b: (lambda: _lib.call("cgs_temporal_smooth_mc", zd.data_ptr(), ld.data_ptr(), f.data_ptr(), b.data_ptr(), n, 0, n,
                                                radius, 16.0, od.data_ptr(), stream()))
        nbytes = n * 64 * 64 * (3 + 4 + 4)
        cases = [("smooth", plain, {}), ("smooth_mc", along(fwd, bwd), {"field": "search 4", "share_found": round(found, 4),
                                                                         "share_saturated": round(sat, 4)})]
        if radius == 3:
            cases.append(("smooth_mc", along(zero, zero), {"field": "zero"}))
        base = None
        for case, fn, extra in cases:
            r = figures(case, device_ms(fn), window_ms(fn), n, nbytes + (0 if case == "smooth" else 2 * radius * 128 * n), radius=radius, **extra)
            r["gtaps_per_s"] = round(n * 4096 * (18 * radius + 1) / r["ms_per_call_in_window"] / 1e6, 1)
            if case == "smooth":
                base = r["ms_per_call_in_window"]
            else:
                r["ratio_to_smooth"] = round(r["ms_per_call_in_window"] / base, 3)
                r["smooth_mc_vs_float64_max_err"] = err
            rows.append(r)

    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
