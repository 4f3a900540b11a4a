"""Times cgs_overlay_compose_tracks (csrc/overlay_tracks.hip) against cgs_overlay_compose (csrc/overlay.hip) in the same run, and
objects.TrackStream.push, for -process --source-video --overlay-tracks.

  compose          cgs_overlay_compose and
  compose_tracks   cgs_overlay_compose_tracks over the same stack of about 256 MB of frames (so the frames do not stay in the 256 MiB
                   Infinity Cache between calls) at 360 x 640 and 1080 x 1920, layout "side", outline 1, boxes 1, non-temporal stores, with
                   0, 4 and 64 objects a frame: squares on an 8 x 8 lattice of the 64 x 64 grid that drift a cell a frame, over a background
                   of 0.02 (grey 5: tinted, as a network's never quite zero mask is), the masks brought to the frame's size by fit.up.  The two kernels are timed alternately; "ratio" is compose_tracks / compose of the window
                   times.  "bytes" is what cgs_overlay_compose moves (tools/time_overlay.py); compose_tracks adds the labels of a band's cell
                   rows, the ids and the table rows per workgroup, which stay in cache.
  push             objects.TrackStream.push over the stack's labels in chunks of 128 frames, in microseconds per frame (the chunk's
                   objects.track call and the torch gather / scatter of the renumbering; no host synchronisation inside).

Per case the median of 5 timed calls after a warm-up, device events around each call, and a window of 20 back-to-back calls between two
events divided by 20.  Before timing, compose_tracks is compared with tests/overlay_tracks_ref.py on the first frame at 360 x 640.  One
JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_overlay_tracks.py [--out profiles/overlay_tracks_time.jsonl]
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
sys.path.insert(0, os.path.join(REPO, "tools"))
import overlay_tracks_ref  # noqa: E402
from cgs_amd import _lib, fit, objects, overlay  # noqa: E402
from time_fit import frames_like_footage  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402
from time_overlay import overlay_bytes, window_ms  # noqa: E402

SIZES = ((360, 640), (1080, 1920))
OBJECTS = (0, 4, 64)
CHUNK, WINDOW = 128, 20


def lattice_masks(n, count):
    """float32 [n,64,64]: `count` squares of 5 x 5 cells on the 8 x 8 lattice, the whole pattern rolled by a cell a frame, over a
    background of 0.02 -- a network's mask is rarely exactly 0, so the grey byte is non-zero far from every object too."""
    base = np.full((64, 64), 0.02, dtype=np.float32)
    slots = [(r, c) for r in range(8) for c in range(8)]
    step = max(1, len(slots) // max(count, 1))
    for r, c in slots[::step][:count]:
        base[8 * r + 1:8 * r + 6, 8 * c + 1:8 * c + 6] = 1.0
    return np.stack([np.roll(base, f % 64, axis=1) for f in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--stack-mb", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_overlay_tracks.py measures on the GPU: none is visible")
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

            def push_all():
                ts = objects.TrackStream(0.3)
                return torch.cat([ts.push(labels[lo:lo + CHUNK]) for lo in range(0, n, CHUNK)])
            ids = push_all()
            if not torch.equal(ids, objects.track(labels, iou=0.3).track):
                raise SystemExit(f"{h}x{w}, {count} objects: the stream's numbers differ from objects.track's")
            found = int((ids > 0).sum()) // n
            if h == SIZES[0][0]:
                want = overlay_tracks_ref.compose_tracks_ref(distinct[:1], grey[:1].cpu().numpy(), hard[:1].cpu().numpy(),
                                                             labels[:1].cpu().numpy(), ids[:1].cpu().numpy(), table[:1].cpu().numpy(),
                                                             overlay.FONT, (0, 255, 0), 128, 1, 1, "side")
                got = overlay.compose_tracks(guide[:1], grey[:1], hard[:1], labels[:1], ids[:1], table[:1], layout="side").cpu().numpy()
                if not np.array_equal(got, want):
                    raise SystemExit(f"{h}x{w}, {count} objects: compose_tracks differs from the checker")
            plain = lambda: _lib.call("cgs_overlay_compose", guide.data_ptr(), grey.data_ptr(), hard.data_ptr(), n, h, w, 0, 255, 0, 128, 1, 2,
                                      _lib.OVERLAY_NONTEMPORAL, out.data_ptr(), stream())
            tracks = lambda: _lib.call("cgs_overlay_compose_tracks", guide.data_ptr(), grey.data_ptr(), hard.data_ptr(), labels.data_ptr(),
                                       ids.data_ptr(), table.data_ptr(), font.data_ptr(), n, h, w, 64, 0, 255, 0, 128, 1, 1, 2,
                                       _lib.OVERLAY_NONTEMPORAL, out.data_ptr(), stream())
            ms = {"compose": [], "compose_tracks": []}
            win = {"compose": [], "compose_tracks": []}
            for _ in range(2):                                            # alternately: the two share whatever else the machine is doing
                for name, fn in (("compose", plain), ("compose_tracks", tracks)):
                    ms[name] += device_ms(fn)
                    win[name].append(window_ms(fn, WINDOW))
            nbytes = overlay_bytes(n, h, w, 2, 1)
            for name in ("compose", "compose_tracks"):
                wmin = min(win[name])
                rows.append({"case": name, "h": h, "w": w, "objects_per_frame": found, "n": n, "layout": "side", "outline": 1, "boxes": 1,
                             "ms_median": round(float(np.median(ms[name])), 4), "ms_min": round(min(ms[name]), 4),
                             "ms_max": round(max(ms[name]), 4), "ms_per_call_in_window": round(wmin, 4),
                             "ms_per_call_in_window_all": [round(v, 4) for v in win[name]], "us_per_frame": round(wmin * 1e3 / n, 3),
                             "compose_bytes": int(nbytes), "tb_per_s_of_compose_bytes": round(nbytes / wmin / 1e9, 3)})
            rows[-1]["ratio_to_compose"] = round(min(win["compose_tracks"]) / min(win["compose"]), 4)
            pm, pw = device_ms(push_all), window_ms(push_all, 5)
            rows.append({"case": "push", "h": h, "w": w, "objects_per_frame": found, "n": n, "chunk": CHUNK,
                         "ms_median": round(float(np.median(pm)), 4), "ms_per_call_in_window": round(pw, 4),
                         "us_per_frame": round(pw * 1e3 / n, 3)})
            del up, grey, hard, z
        del guide, out
        torch.cuda.empty_cache()
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
