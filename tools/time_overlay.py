"""Times the kernels of -process --source-video (csrc/overlay.hip, csrc/temporal.hip) and the device chain around them.

  overlay     cgs_overlay_compose at 360 x 640 and 1080 x 1920, each over a stack of about 256 MB of frames (so the frames do not stay
              in the 256 MiB Infinity Cache between calls), for the three layouts and outline thickness 0 / 1 / 4, non-temporal stores as
              the product runs them (and once with plain stores).  "bytes" is what the kernel moves, counted from the shapes: 3 + 1 bytes
              a pixel read, 1 more of `hard` with an outline (its halo rows twice), 3 k written.
  copy        a device-to-device copy of the same frames (bytes = 2 x the frames), and
  video       cgs_video_compose on its own -test layout (bytes = the frames written): the two yardsticks, measured in the same session.
  smooth      cgs_temporal_smooth at radius 1 / 3 / 8 over 4096 frames of 64 x 64, in microseconds per frame.
  chain       stage A + stage B of Handler._segment_video fed from device memory, no ffmpeg: fit.down, the network (fixture G1's
              weights), temporal.smooth at radius 3, fit.up (grey + hard), overlay.compose (side), in frames per second at both sizes.

The C entry points are called on preallocated outputs, so a kernel figure is the kernel and its launch, not the allocator.  Per case the
median of 5 timed calls after a warm-up, device events around each call, and a window of 50 back-to-back calls between two events divided
by 50 (10 for the chain).  Before timing, the overlay is compared with tests/overlay_ref.py on the first frame and the smoothing with
float64 on 8 frames.  One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_overlay.py [--out profiles/overlay_time.jsonl]
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
import overlay_ref  # noqa: E402
import temporal_ref  # noqa: E402
from cgs_amd import _lib, engine, fit, overlay, temporal, video  # noqa: E402
from time_fit import frames_like_footage  # noqa: E402
from time_metrics import csrc_hash, device_ms  # noqa: E402

SIZES = ((360, 640), (1080, 1920))
COPY_GB_PER_S = 6300.0          # the achievable HBM copy rate of the part (8 TB/s peak)
BAND = 16                       # rows of a workgroup's band (OV_BAND, csrc/overlay_body.h)


def window_ms(fn, window=50):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(window):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / window


def overlay_bytes(n, h, w, k, t):
    hard = 0
    if t:
        bands = (h + BAND - 1) // BAND
        hard = w * sum(min(h, b * BAND + BAND + t) - max(0, b * BAND - t) for b in range(bands))
    return n * (h * w * (4 + 3 * k) + hard)


def figures(case, ms, win, n, nbytes, **extra):
    return {"case": case, **extra, "n": n, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "ms_per_call_in_window": round(win, 4), "us_per_frame": round(win * 1e3 / n, 3),
            "frames_per_s": round(n / win * 1e3, 1), "bytes": int(nbytes), "tb_per_s": round(nbytes / win / 1e9, 3),
            "share_of_copy_rate": round(nbytes / win / 1e6 / COPY_GB_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--stack-mb", type=int, default=256)
    ap.add_argument("--smooth-frames", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_overlay.py measures on the GPU: none is visible")
    rs = np.random.RandomState(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    rows = []

    # ---- the network of the chain: fixture G1's weights
    raw = dict(np.load(os.path.join(REPO, "tests", "golden", "g1_weights_chfak1.npz")))
    pc = {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in raw.items() if k.startswith("critic/")}
    pm = {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in raw.items() if k.startswith("masker/")}
    eng = engine.HourglassEngine(64, device=torch.device("cuda:0"), dropout=0.0)
    eng.load_state(pc, pm)
    unit = torch.from_numpy((np.arange(256) / 255.0).astype(np.float32)).to("cuda")

    for h, w in SIZES:
        n = max(1, (a.stack_mb << 20) // (3 * h * w))
        distinct = frames_like_footage(min(n, 8), h, w, rs)
        guide = torch.from_numpy(distinct).to("cuda")[torch.arange(n, device="cuda") % len(distinct)].contiguous()
        low = fit.down(guide)
        z = torch.from_numpy(rs.rand(n, 64, 64).astype(np.float32)).to("cuda")
        up = fit.up(z, guide, low, thresh=0.5, want=("grey", "hard"))
        grey, hard = up.grey, up.hard
        out = torch.empty((n, h, 3 * w, 3), dtype=torch.uint8, device="cuda")
        want = overlay_ref.compose_ref(distinct[:1], grey[:1].cpu().numpy(), hard[:1].cpu().numpy(), (0, 255, 0), 128, 4, "triple")
        got = overlay.compose(guide[:1], grey[:1], hard[:1], outline=4, layout="triple").cpu().numpy()
        if not np.array_equal(got, want):
            raise SystemExit(f"{h}x{w}: the overlay differs from the checker")
        for layout, k in (("overlay", 1), ("side", 2), ("triple", 3)):
            for t in (0, 1, 4):
                for nt in ((True, False) if (k, t) == (2, 1) else (True,)):
                    fn = lambda: _lib.call("cgs_overlay_compose", guide.data_ptr(), grey.data_ptr(), hard.data_ptr(), n, h, w, 0, 255, 0, 128,
                                           t, k, _lib.OVERLAY_NONTEMPORAL if nt else 0, out.data_ptr(), stream())
                    rows.append(figures("overlay", device_ms(fn), window_ms(fn), n, overlay_bytes(n, h, w, k, t), h=h, w=w, layout=layout,
                                        outline=t, nontemporal=nt))
        dst = torch.empty_like(guide)
        fn = lambda: dst.copy_(guide)
        rows.append(figures("copy", device_ms(fn), window_ms(fn), n, 2 * guide.numel(), h=h, w=w))
        del dst, out

        # the chain, fed from device memory in chunks of at most 128 frames as the Handler runs it
        step = max(1, min(128, (256 << 20) // (3 * h * w)))

        def chain():
            for lo in range(0, n, step):
                g = guide[lo:lo + step]
                l = fit.down(g)
                _pred, Z = eng.infer(unit[l.long()])
                Z = temporal.smooth(Z.contiguous(), l, 3)
                u = fit.up(Z, g, l, thresh=0.5, want=("grey", "hard"))
                overlay.compose(g, u.grey, u.hard, layout="side")
        ms, win = device_ms(chain), window_ms(chain, 10)
        rows.append({"case": "chain", "h": h, "w": w, "n": n, "chunk": step, "smooth": 3, "layout": "side",
                     "ms_median": round(float(np.median(ms)), 3), "ms_per_call_in_window": round(win, 3),
                     "frames_per_s": round(n / win * 1e3, 1)})
        del guide, grey, hard, up
        torch.cuda.empty_cache()

    # ---- cgs_video_compose beside it: its own layout, 2450 frames of 960 x 624
    nv = 2450
    src = {"X": rs.randint(0, 256, (nv, 64, 64, 3)).astype(np.uint8), "Y": rs.rand(nv, 64, 64) < 0.3,
           "M": rs.rand(nv, 64, 64).astype(np.float32), "hardM": rs.rand(nv, 64, 64) < 0.5, "salM": rs.rand(nv, 64, 64),
           "salhardM": (rs.rand(nv, 64, 64) < 0.5).astype(np.uint8)}
    lay = video.plan(False, True)
    comp = video.Composer(lay, src)
    full = torch.empty((nv,) + comp.frame_shape, dtype=torch.uint8, device=comp.device)
    fn = lambda: comp.compose(0, nv, out=full)
    rows.append(figures("video", device_ms(fn), window_ms(fn), nv, full.numel(), h=lay.height, w=lay.width))
    del full, comp

    # ---- the smoothing
    ns = a.smooth_frames
    zs, ls = temporal_ref_inputs(ns, rs)
    zd, ld = torch.from_numpy(zs).to("cuda"), torch.from_numpy(ls).to("cuda")
    od = torch.empty_like(zd)
    err = float(np.abs(temporal.smooth(zd[:8], ld[:8], 3).cpu().numpy().astype(np.float64) - temporal_ref.smooth_ref(zs[:8], ls[:8], 3, 16.0)).max())
    if err > 2.6e-5:
        raise SystemExit(f"the smoothing differs from float64 by {err:.2e}")
    for radius in (1, 3, 8):
        fn = lambda: _lib.call("cgs_temporal_smooth", zd.data_ptr(), ld.data_ptr(), ns, 0, ns, radius, 16.0, od.data_ptr(), stream())
        r = figures("smooth", device_ms(fn), window_ms(fn), ns, ns * 64 * 64 * (3 + 4 + 4), radius=radius, smooth_vs_float64_max_err=err)
        r["gtaps_per_s"] = round(ns * 4096 * (18 * radius + 1) / r["ms_per_call_in_window"] / 1e6, 1)
        rows.append(r)

    stamp = {"csrc": csrc_hash(), "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    lines = [json.dumps({**r, **stamp}) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


def temporal_ref_inputs(n, rs):
    """A drifting blocky stack as tests/test_gpu_temporal.py builds it, n frames long (the drift wraps every 64 frames)."""
    colour = np.repeat(np.repeat(rs.randint(0, 256, (8, 16, 3)), 9, axis=0), 9, axis=1)
    value = np.repeat(np.repeat(rs.rand(8, 16), 9, axis=0), 9, axis=1)
    low = np.stack([colour[3:67, (f % 64):(f % 64) + 64] for f in range(n)])
    z = np.stack([value[3:67, (f % 64):(f % 64) + 64] for f in range(n)])
    low = np.clip(low + rs.randint(-6, 7, low.shape), 0, 255).astype(np.uint8)
    return np.clip(z + rs.uniform(-0.05, 0.05, z.shape), 0.0, 1.0).astype(np.float32), low


if __name__ == "__main__":
    main()
