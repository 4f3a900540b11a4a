"""Times what -process --source-video --overlay-fill adds, in the same run and on the same stacks as its yardsticks:

  compose_tracks    cgs_overlay_compose_tracks and
  compose_carried   cgs_overlay_compose_tracks_carried (csrc/overlay_tracks.hip) over tools/time_overlay_tracks.py's stacks -- about 256 MB of
                    frames at 360 x 640 and 1080 x 1920, layout "side", outline 1, boxes 1, non-temporal stores, 0 / 4 / 64 drifting objects
                    a frame -- with every second object of a frame carried (age 1).  The two are timed alternately; "ratio" is
                    compose_carried / compose_tracks of the window times.
  track_push        objects.TrackStream.push and
  fill_push         objects.FillStream.push (+ flush) over a flickering 64 x 64 label stack in chunks of 128 frames, at G = 1 and G = 8, in
                    microseconds per frame: the stream's tracker call, the window's tracker call, cgs_objects_track_fill_window and the torch
                    glue; no host synchronisation inside.
  ab                with --ab-lib OTHER.so (a build of another commit): cgs_overlay_compose_tracks of this build and of that one on the
                    1080 x 1920 stack with 4 objects, windows of 20 calls in turns, `--ab-windows` of each.  Per build the spread of its own
                    windows, (max - min) / min, and the difference of the two medians over the other build's median: the entry has not
                    slowed when the difference lies within the other build's own spread.

Per case the median of 5 timed calls after a warm-up, device events around each call, and windows of 20 back-to-back calls between two
events divided by 20.  Before timing, compose_carried is compared with tests/overlay_fill_ref.py on the first frame at 360 x 640, and
with all ages 0 with compose_tracks byte for byte; FillStream's result with objects.fill of the whole stack.  One JSON line per case on
stdout and, with --out FILE, appended to FILE.

    python tools/time_overlay_fill.py [--out profiles/overlay_fill_time.jsonl] [--ab-lib other/libcgs_hip.so]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import overlay_fill_ref  # noqa: E402
from cgs_amd import _lib, fit, objects, overlay  # noqa: E402
from time_fit import frames_like_footage  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402
from time_overlay import window_ms  # noqa: E402
from time_overlay_tracks import CHUNK, OBJECTS, SIZES, WINDOW, lattice_masks  # noqa: E402

GAPS = (1, 8)


def flickering_labels(n, seed=0):
    """int32 [n,64,64]: 16 squares of 9 x 9 cells on a 4 x 4 lattice, each drifting a cell every other frame and absent from a quarter
    of the frames, numbered per frame in raster order of those that are there."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 64, 64), dtype=np.int32)
    for f in range(n):
        k = 0
        for r in range(4):
            for c in range(4):
                if rs.rand() < 0.25:
                    continue
                k += 1
                x = (16 * c + 2 + f // 2) % 55
                out[f, 16 * r + 2:16 * r + 11, x:x + 9] = k
    return out


def other_entry(path):
    """cgs_overlay_compose_tracks of another build of the library, loaded beside this one."""
    fn = ctypes.CDLL(os.path.abspath(path)).cgs_overlay_compose_tracks
    fn.restype, fn.argtypes = _lib.SIGNATURES["cgs_overlay_compose_tracks"]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--stack-mb", type=int, default=256)
    ap.add_argument("--ab-lib", default="")
    ap.add_argument("--ab-name", default="the parent commit")
    ap.add_argument("--ab-windows", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_overlay_fill.py measures on the GPU: none is visible")
    rs = np.random.RandomState(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    font = torch.from_numpy(np.array(overlay.FONT)).to("cuda")
    rows = []
    for h, w in SIZES:
        n = max(1, (a.stack_mb << 20) // (3 * h * w))
        distinct = frames_like_footage(min(n, 8), h, w, rs)
        guide = torch.from_numpy(distinct).to("cuda")[torch.arange(n, device="cuda") % len(distinct)].contiguous()
        low = fit.down(guide)
        out = torch.empty((n, h, 2 * w, 3), dtype=torch.uint8, device="cuda")
        for count in OBJECTS:
            z = torch.from_numpy(lattice_masks(n, count)).to("cuda")
            up = fit.up(z, guide, low, thresh=0.5, want=("grey", "hard"))
            grey, hard = up.grey, up.hard
            res = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, max_objects=64)
            labels, table = res.labels, res.table
            ids = objects.track(labels, iou=0.3).track
            age = ((ids > 0) & (torch.arange(64, device="cuda")[None] % 2 == 1)).to(torch.int32).contiguous()
            found = int((ids > 0).sum()) // n
            if h == SIZES[0][0]:
                args = (guide[:1], grey[:1], hard[:1], labels[:1], ids[:1], table[:1])
                want = overlay_fill_ref.compose_carried_ref(distinct[:1], *(t.cpu().numpy() for t in args[1:]), age[:1].cpu().numpy(),
                                                            overlay.FONT, (0, 255, 0), 128, 1, 1, "side")
                if not np.array_equal(overlay.compose_tracks(*args, layout="side", age=age[:1]).cpu().numpy(), want):
                    raise SystemExit(f"{h}x{w}, {count} objects: compose_tracks(age=) differs from the checker")
                if not torch.equal(overlay.compose_tracks(*args, layout="side", age=torch.zeros_like(age[:1])),
                                   overlay.compose_tracks(*args, layout="side")):
                    raise SystemExit(f"{h}x{w}, {count} objects: all ages 0 differ from compose_tracks")
            common = (font.data_ptr(), n, h, w, 64, 0, 255, 0, 128, 1, 1, 2, _lib.OVERLAY_NONTEMPORAL, out.data_ptr())
            head = (guide.data_ptr(), grey.data_ptr(), hard.data_ptr(), labels.data_ptr(), ids.data_ptr(), table.data_ptr())
            tracks = lambda: _lib.call("cgs_overlay_compose_tracks", *head, *common, stream())
            carried = lambda: _lib.call("cgs_overlay_compose_tracks_carried", *head, age.data_ptr(), *common, stream())
            names = ("compose_tracks", "compose_carried")
            ms, win = {k: [] for k in names}, {k: [] for k in names}
            for _ in range(2):                                            # alternately: the two share whatever else the machine is doing
                for name, fn in zip(names, (tracks, carried)):
                    ms[name] += device_ms(fn)
                    win[name].append(window_ms(fn, WINDOW))
            for name in names:
                wmin = min(win[name])
                rows.append({"case": name, "h": h, "w": w, "objects_per_frame": found, "carried_per_frame": int((age > 0).sum()) // n, "n": n,
                             "layout": "side", "outline": 1, "boxes": 1, "ms_median": round(float(np.median(ms[name])), 4),
                             "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4), "ms_per_call_in_window": round(wmin, 4),
                             "ms_per_call_in_window_all": [round(v, 4) for v in win[name]], "us_per_frame": round(wmin * 1e3 / n, 3)})
            rows[-1]["ratio_to_compose_tracks"] = round(min(win["compose_carried"]) / min(win["compose_tracks"]), 4)
            if a.ab_lib and h == SIZES[-1][0] and count == 4:
                entry = other_entry(a.ab_lib)

                def other():
                    rc = entry(*head, *common, stream())
                    if rc:
                        raise SystemExit(f"--ab-lib: cgs_overlay_compose_tracks returned {rc}")
                this, that = [], []
                window_ms(tracks, WINDOW), window_ms(other, WINDOW)       # both warm
                for _ in range(a.ab_windows):
                    this.append(window_ms(tracks, WINDOW))
                    that.append(window_ms(other, WINDOW))
                spread = lambda v: (max(v) - min(v)) / min(v)
                diff = (float(np.median(this)) - float(np.median(that))) / float(np.median(that))
                rows.append({"case": "ab", "entry": "cgs_overlay_compose_tracks", "h": h, "w": w, "objects_per_frame": found, "n": n,
                             "window": WINDOW, "this_ms": [round(v, 4) for v in this], "other_ms": [round(v, 4) for v in that],
                             "this_spread": round(spread(this), 5), "other_spread": round(spread(that), 5),
                             "median_difference": round(diff, 5), "within_other_spread": bool(abs(diff) <= spread(that)),
                             "other": a.ab_name})
            del up, grey, hard, z
        del guide, out
        torch.cuda.empty_cache()

    n = 2048
    stack = torch.from_numpy(flickering_labels(n)).to("cuda")
    for G in GAPS:
        def track_all():
            ts = objects.TrackStream(0.3, max_gap=G)
            return torch.cat([ts.push(stack[lo:lo + CHUNK]) for lo in range(0, n, CHUNK)])

        def fill_all():
            fs = objects.FillStream(0.3, max_gap=G)
            parts = [fs.push(stack[lo:lo + CHUNK]) for lo in range(0, n, CHUNK)] + [fs.flush()]
            return parts, fs
        parts, fs = fill_all()
        whole = objects.fill(stack, objects.track(stack, iou=0.3, max_gap=G))
        for key in ("labels", "track", "age", "table"):
            if not torch.equal(torch.cat([getattr(p, key) for p in parts]), getattr(whole, key)):
                raise SystemExit(f"G = {G}: the stream's {key} differ from objects.fill's")
        new = int(fs.totals[0])
        for name, fn in (("track_push", track_all), ("fill_push", fill_all)):
            pm, pw = device_ms(fn), window_ms(fn, 5)
            rows.append({"case": name, "gap": G, "n": n, "chunk": CHUNK, "new_objects": new, "ms_median": round(float(np.median(pm)), 4),
                         "ms_per_call_in_window": round(pw, 4), "us_per_frame": round(pw * 1e3 / n, 3)})
        rows[-1]["ratio_to_track_push"] = round(rows[-1]["us_per_frame"] / rows[-2]["us_per_frame"], 3)
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
