"""Times the evaluation-video composition (cgs_video_compose, csrc/video.hip) at the full -test size: n = 2450 frames in both layouts
(5 columns, 960 x 624; 8 columns, 1536 x 564), with plain and non-temporal stores, alternated, 5 timed repeats after a warm-up.

  compose_all   one launch writing all n frames (4.4 / 6.4 GB) into device memory
  compose_c64   n / 64 launches of 64 frames into one 64-frame buffer, as the encoder pipeline runs them
  stream_null   the whole pipeline (video.stream_frames: compose, copy into two pinned host buffers, a writer thread) into a sink that
                discards the bytes: the rate the GPU side can feed an encoder
GB/s counts the bytes of finished frames written (n * H * W * 3).  With --mp4 DIR and an `ffmpeg` on PATH, one real video of --mp4-frames
frames is also encoded (libx264) and its size and time reported.  One JSON line per case on stdout and, with --out FILE, in FILE.

    python tools/time_video.py [--out profiles/video_time.jsonl] [--mp4 DIR]
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cgs_amd import video  # noqa: E402


def csrc_hash():
    d = os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fp:
            h.update(f.encode() + fp.read())
    return h.hexdigest()[:12]


def sources(n, seed=0):
    rs = np.random.RandomState(seed)
    M = rs.rand(n, 64, 64).astype(np.float32)
    sal = np.minimum(rs.rand(n, 64, 64) * 1.5, 1.0)
    Y = rs.rand(n, 64, 64) < 0.3
    return {"X": rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8), "Y": Y, "M": M, "hardM": M > 0.5, "crfM": rs.rand(n, 64, 64) < 0.4,
            "salM": sal, "salhardM": (sal > 0.5).astype(np.uint8), "salcrfM": rs.rand(n, 64, 64) < 0.4}


class Null:
    def write(self, b):
        return len(b)


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def row(case, lay, n, ms, **kw):
    med = float(np.median(ms))
    nbytes = n * lay.height * lay.width * 3
    return {"case": case, "columns": len(lay.row1), "W": lay.width, "H": lay.height, "n": n, **kw, "ms_median": round(med, 3),
            "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "frames_per_s": round(n / med * 1e3, 1),
            "GB_per_s": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2450)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--mp4", default="", help="directory for one real libx264 video (needs ffmpeg on PATH)")
    ap.add_argument("--mp4-frames", type=int, default=245)
    a = ap.parse_args()
    n = a.n
    src = sources(n)
    rows = []
    for crf in (False, True):
        lay = video.plan(crf, True)
        comp = video.Composer(lay, src)
        full = torch.empty((n,) + comp.frame_shape, dtype=torch.uint8, device=comp.device)
        c64 = torch.empty((64,) + comp.frame_shape, dtype=torch.uint8, device=comp.device)
        per = {}
        for nt in (False, True):                  # warm-up both variants
            comp.compose(0, n, out=full, nontemporal=nt)
        torch.cuda.synchronize()
        ref = full.clone()
        for _ in range(a.repeats):                # alternate the store policies: A B A B ...
            for nt in (False, True):
                per.setdefault(("all", nt), []).extend(timed(lambda: comp.compose(0, n, out=full, nontemporal=nt), 1))
                per.setdefault(("c64", nt), []).extend(
                    timed(lambda: [comp.compose(f0, min(64, n - f0), out=c64, nontemporal=nt) for f0 in range(0, n, 64)], 1))
        assert torch.equal(full, ref), "plain and non-temporal stores composed different frames"
        del full, ref, c64
        for (case, nt), ms in sorted(per.items()):
            rows.append(row(f"compose_{case}", lay, n, ms, nontemporal=nt))
        video.stream_frames(comp, Null())         # warm-up (pinned buffers, thread)
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            video.stream_frames(comp, Null())
            ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(row("stream_null", lay, n, ms, nontemporal=video.NONTEMPORAL))
        if a.mp4 and not crf:
            exe = shutil.which("ffmpeg")
            if exe is None:
                rows.append({"case": "mp4", "skipped": "no ffmpeg on PATH"})
            else:
                sub = {k: v[:a.mp4_frames] for k, v in src.items()}
                path = os.path.join(a.mp4, "iou=0.5.mp4")
                t0 = time.perf_counter()
                video.write_video(path, lay, sub, ffmpeg=exe)
                rows.append({"case": "mp4", "file": path, "frames": a.mp4_frames, "bytes": os.path.getsize(path),
                             "s": round(time.perf_counter() - t0, 2)})
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
