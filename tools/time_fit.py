"""Times the two kernels of -process -fit (csrc/fit.hip) at 360 x 640 and 1080 x 1920, each over a stack of about 256 MB of frames (so the
frames do not stay in the 256 MiB Infinity Cache between calls):

  down        cgs_fit_down_u8: the frames to 64 x 64
  up_soft     cgs_fit_up_joint writing the fp32 map only (4 bytes a pixel out)
  up_process  cgs_fit_up_joint writing grey and hard (2 bytes a pixel out): what -process -fit asks for per column pair

The C entry points are called on preallocated outputs, so a figure is the kernel and its launch, not the allocator.  Per case: the median
of 5 timed calls after a warm-up, device events around each call, and a window of 50 back-to-back calls between two events divided by
50.  "bytes" is what the kernel reads and writes, counted from the shapes: for down every source row once per cell row that it overlaps
(a row on the border of two cell rows is read twice) plus the 64 x 64 x 3 output; for up the guide, the five staged cell rows of `low`
and of the map per workgroup, and the outputs.  gb_per_s = bytes / the window time, to be read beside the 6.3 TB/s a copy reaches on
this part; up also reports pixels and taps per second, because its arithmetic (25 taps a pixel, one exponential each), not its traffic,
is what bounds it.  Beside each size what a user does without the kernels: PIL's resize on the host, BOX down to 64 x 64 and BILINEAR
back up, per frame (wall clock over --host-frames frames).  Before timing, down is compared with the checker (tests/fit_ref.py) on the
first frame and up with float64 on the first frame.
One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_fit.py [--out profiles/fit_time.jsonl]
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
import fit_ref  # noqa: E402
from cgs_amd import _lib, fit  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402

SIZES = ((360, 640), (1080, 1920))
WINDOW = 50
COPY_GB_PER_S = 6300.0          # the achievable HBM copy rate of the part (8 TB/s peak)


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


def down_bytes(n, h, w):
    rows = sum((h * o + h - 1) // 64 - (h * o) // 64 + 1 for o in range(64))          # source rows read, over the 64 cell rows
    return n * (rows * 3 * w + 64 * 64 * 3)


def up_bytes(n, h, w, out_bytes_per_pixel):
    staged = 64 * ((w + 255) // 256) * 5 * 64 * (3 + 4)                                # per frame: every workgroup stages five cell rows
    return n * (h * w * (3 + out_bytes_per_pixel) + staged)


def frames_like_footage(n, h, w, rs):
    """Smooth colour fields with a few hard-edged rectangles and a little noise: edges for the filter to follow."""
    ys, xs = np.linspace(0, 1, h)[:, None, None], np.linspace(0, 1, w)[None, :, None]
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for f in range(n):
        a, b, c = rs.rand(3) * 255, rs.rand(3) * 120 - 60, rs.rand(3) * 120 - 60
        img = a + b * ys + c * xs
        for _ in range(6):
            y0, x0 = rs.randint(0, h - 8), rs.randint(0, w - 8)
            img[y0:y0 + rs.randint(8, h // 2), x0:x0 + rs.randint(8, w // 2)] = rs.rand(3) * 255
        out[f] = np.clip(img + rs.randint(-4, 5, img.shape), 0, 255).astype(np.uint8)
    return out


def host_ms_per_frame(frames, masks, count):
    from PIL import Image
    t0 = time.perf_counter()
    for i in range(count):
        h, w = frames[i].shape[:2]
        Image.fromarray(frames[i]).resize((64, 64), Image.BOX)
        Image.fromarray(masks[i]).resize((w, h), Image.BILINEAR)
    return (time.perf_counter() - t0) * 1e3 / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--stack-mb", type=int, default=256)
    ap.add_argument("--host-frames", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fit.py measures on the GPU: none is visible")
    rs = np.random.RandomState(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    rows = []
    for h, w in SIZES:
        n = max(1, (a.stack_mb << 20) // (3 * h * w))
        distinct = frames_like_footage(min(n, 8), h, w, rs)
        guide = torch.from_numpy(distinct).to("cuda")[torch.arange(n, device="cuda") % len(distinct)].contiguous()
        masks = rs.rand(n, 64, 64).astype(np.float32)
        m = torch.from_numpy(masks).to("cuda")
        low = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device="cuda")
        soft = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        grey = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        hard = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        down = lambda: _lib.call("cgs_fit_down_u8", guide.data_ptr(), n, h, w, low.data_ptr(), stream())
        up = lambda s, g, hd: _lib.call("cgs_fit_up_joint", m.data_ptr(), _lib.FIT_MAP_F32, guide.data_ptr(), low.data_ptr(), n, h, w,
                                        fit.SIGMA_SPATIAL, fit.SIGMA_RANGE, 0.5, 1, s, g, hd, stream())
        up_soft = lambda: up(soft.data_ptr(), None, None)
        up_process = lambda: up(None, grey.data_ptr(), hard.data_ptr())
        down()
        up_soft()
        torch.cuda.synchronize()
        if not np.array_equal(low[:1].cpu().numpy(), fit_ref.down_ref(distinct[:1])):
            raise SystemExit(f"{h}x{w}: down differs from the checker")
        want = fit_ref.up_ref(masks[:1], distinct[:1], low[:1].cpu().numpy(), fit.SIGMA_SPATIAL, fit.SIGMA_RANGE)[0]
        err = float(np.abs(soft[0].cpu().numpy().astype(np.float64) - want).max())
        if err > 1e-5:
            raise SystemExit(f"{h}x{w}: up differs from float64 by {err:.2e}")
        host = host_ms_per_frame(distinct, (masks[:len(distinct)] * 255).astype(np.uint8), min(a.host_frames, len(distinct)))
        for case, fn, nbytes in (("down", down, down_bytes(n, h, w)), ("up_soft", up_soft, up_bytes(n, h, w, 4)),
                                 ("up_process", up_process, up_bytes(n, h, w, 2))):
            ms = device_ms(fn)
            win = window_ms(fn)
            med = float(np.median(ms))
            row = {"case": case, "h": h, "w": w, "n": n, "frame_mb": round(n * 3 * h * w / 2 ** 20, 1), "ms_median": round(med, 4),
                   "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), f"ms_per_call_in_window_of_{WINDOW}": round(win, 4),
                   "us_per_frame": round(win * 1e3 / n, 3), "frames_per_s": round(n / win * 1e3, 1), "bytes": nbytes,
                   "gb_per_s": round(nbytes / win / 1e6, 1), "share_of_copy_rate": round(nbytes / win / 1e6 / COPY_GB_PER_S, 4),
                   "host_pil_box_down_bilinear_up_ms_per_frame": round(host, 3)}
            if case != "down":
                row.update({"gpixels_per_s": round(n * h * w / win / 1e6, 2), "gtaps_per_s": round(25 * n * h * w / win / 1e6, 1),
                            "up_vs_float64_max_err": err})
            rows.append(row)
        del guide, soft, grey, hard
        torch.cuda.empty_cache()
    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
