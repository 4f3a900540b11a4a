"""Times the composition of the -viscritic / -vismasker videos (cgs_vis_compose, csrc/vis.hip) at the default --testsize: N = 5000
frames, the three videos of a run (time order, sorted by prediction, sorted by ground truth), R = 2 (256 x 768) and R = 1 (256 x 512),
with plain and non-temporal stores alternated in one process, 5 timed repeats after a warm-up.

  compose_all    per video one launch writing all N frames (2.9 / 2.0 GB) into device memory
  compose_chunk  per video N / chunk launches into one chunk-sized buffer (vis.CHUNK frames), as the encoder pipeline runs them
  stream_null    the three videos through video.stream_frames (compose, copy into two pinned host buffers, a writer thread) into a sink
                 that discards the bytes: the rate the GPU side can feed the encoders
  tables         the host side of one run: plot rows, label strings, PIL rendering of the distinct labels, the uploads
GB/s counts the bytes of finished frames written (3 N H 256 3).  One JSON line per case on stdout and, with --out FILE, appended to
FILE.

    python tools/time_vis.py [--out profiles/vis_time.jsonl]
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
from cgs_amd import video, vis  # noqa: E402


def csrc_hash():
    d = os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fp:
            h.update(f.encode() + fp.read())
    return h.hexdigest()[:12]


class Null:
    def write(self, b):
        return len(b)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def row(case, p, frames, ms, **kw):
    med = float(np.median(ms))
    nbytes = frames * p.height * p.width * 3
    return {"case": case, "R": p.R, "W": p.width, "H": p.height, "frames": frames, **kw, "ms_median": round(med, 3),
            "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "frames_per_s": round(frames / med * 1e3, 1),
            "GB_per_s": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=vis.CHUNK)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-labels", action="store_true", help="diagnostic: every label id -1, so no label is blended")
    a = ap.parse_args()
    n, chunk = a.n, min(a.chunk, a.n)
    rs = np.random.RandomState(0)
    X = torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).cuda()
    masks = torch.from_numpy(rs.rand(n, 64, 64).astype(np.float32)).cuda()
    values = np.stack((rs.rand(n), 0.3 + 0.4 * rs.rand(n)))
    rows = []
    t0 = time.perf_counter()
    tables = vis.upload_tables(values, n, X.device)
    torch.cuda.synchronize()
    rows.append({"case": "tables", "frames": n, "labels": len(tables.atlas), "s": round(time.perf_counter() - t0, 3)})
    if a.no_labels:
        tables = tables._replace(ids=torch.full_like(tables.ids, -1))
    for use_masks in (True, False):
        p = vis.plan(use_masks)
        comps = [vis.Composer(X, masks if use_masks else None, values, perm, tables=tables) for _, perm in vis.sortings(values, 1)]
        full = torch.empty((n,) + comps[0].frame_shape, dtype=torch.uint8, device=X.device)
        part = torch.empty((chunk,) + comps[0].frame_shape, dtype=torch.uint8, device=X.device)
        per = {}

        def all_videos(nt):
            for c in comps:
                c.compose(0, n, out=full, nontemporal=nt)

        def all_chunks(nt):
            for c in comps:
                for f0 in range(0, n, chunk):
                    c.compose(f0, min(chunk, n - f0), out=part, nontemporal=nt)
        sums = []
        for nt in (False, True):                  # warm-up both variants; both policies must compose the same frames
            comps[-1].compose(0, n, out=full, nontemporal=nt)
            torch.cuda.synchronize()
            sums.append(full.view(-1)[::7].long().sum().item())
            all_videos(nt)
        assert sums[0] == sums[1], "plain and non-temporal stores composed different frames"
        for _ in range(a.repeats):                # alternate the store policies: A B A B ...
            for nt in (False, True):
                per.setdefault(("all", nt), []).append(timed(lambda: all_videos(nt)))
                per.setdefault(("chunk", nt), []).append(timed(lambda: all_chunks(nt)))
        del full, part
        for (case, nt), ms in sorted(per.items()):
            rows.append(row(f"compose_{case}", p, 3 * n, ms, nontemporal=nt, **({"chunk": chunk} if case == "chunk" else {})))
        for c in comps:                           # warm-up (pinned buffers, thread)
            video.stream_frames(c, Null(), chunk)
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c in comps:
                video.stream_frames(c, Null(), chunk)
            ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(row("stream_null", p, 3 * n, ms, nontemporal=vis.NONTEMPORAL, chunk=chunk))
    if a.no_labels:
        rows = [{**r, "no_labels": True} for r in rows]
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
