"""Times cgs_dense_crf2 (csrc/crf.hip) on the -eval stack size: n = 2450 frames of 64 x 64 at the reference's parameters (10 iterations),
on uniform-noise frames and on frame-like ones (flat blocks, repeated rows), 5 timed repeats after a warm-up; plus one 128 x 128 run.

Pair evaluations per call: (iterations + 1) sweeps of N^2 pairs per frame (the row sums, then one sweep per iteration; S^B rides on the
first).  The cost-model bound: 44 SIMD-cycles per 64 pairs (about 9 plain VALU at 4 cycles plus one v_exp_f32 at 8), 256 CUs x 4 SIMDs
at 2.4 GHz.  Writes one JSON line per case to stdout and, with --out FILE, the same lines to FILE.

    python tools/time_crf.py [--out profiles/crf_time.jsonl]
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
from cgs_amd import crf  # noqa: E402

BOUND_PAIRS_PER_S = 256 * 4 * 2.4e9 * 64 / 44


def csrc_hash():
    d = os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fp:
            h.update(f.encode() + fp.read())
    return h.hexdigest()[:12]


def frames_noise(rs, n, h, w):
    return rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def frames_like(rs, n, h, w):
    """Flat colour blocks with a few repeated textured rows: many pairs with a non-negligible bilateral weight."""
    out = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        f = np.full((h, w, 3), rs.randint(0, 256, 3), np.uint8)
        for _ in range(5):
            y0, x0 = rs.randint(0, h), rs.randint(0, w)
            f[y0:y0 + rs.randint(4, h // 2), x0:x0 + rs.randint(4, w // 2)] = rs.randint(0, 256, 3)
        r = rs.randint(0, h - 6)
        f[r:r + 6] = rs.randint(0, 256, (1, w, 3))
        out[k] = f
    return out


def time_case(name, frames, p1, params, repeats=5):
    dev = "cuda"
    f = torch.from_numpy(frames).to(dev)
    p = torch.from_numpy(p1).to(dev)
    crf.dense_crf(f, p, params)                 # warm-up (module load, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        crf.dense_crf(f, p, params)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    n, h, w = p1.shape
    pairs = n * (params[5] + 1) * float(h * w) ** 2
    med = float(np.median(ms))
    return {"case": name, "n": n, "h": h, "w": w, "iterations": params[5], "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "frames_per_s": round(n / med * 1e3, 1), "pairs_per_s": float(f"{pairs / med * 1e3:.4g}"),
            "bound_fraction": round(pairs / med * 1e3 / BOUND_PAIRS_PER_S, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=2450)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    n = a.n
    p64 = rs.uniform(0, 1, (n, 64, 64)).astype(np.float32)
    rows = [time_case("noise_64", frames_noise(rs, n, 64, 64), p64, crf.REFERENCE_PARAMS),
            time_case("framelike_64", frames_like(rs, n, 64, 64), p64, crf.REFERENCE_PARAMS),
            time_case("framelike_128", frames_like(rs, 256, 128, 128), rs.uniform(0, 1, (256, 128, 128)).astype(np.float32),
                      crf.REFERENCE_PARAMS)]
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
