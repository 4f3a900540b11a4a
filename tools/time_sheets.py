"""Times the PNG sheets of the training loops (cgs_sheet_compose, csrc/sheet.hip; cgs_amd/sheets.py).

  kernel   the compose kernel at n = 64 and n = 512 by device events (bytes moved from the shapes: A, B, Z read, the sheet written),
           the copy of a sheet into a pinned slot, and what the writer thread spends per sheet (PIL labels + PNG) at zlib levels
           6 (PIL's default), 1 and 0 on noise frames, the worst case for the encoder
  loop     ONE run of the mask-training loop (Handler.segmentation_training, bench.py's cli-train set-up: 16384 synthetic frames,
           the G1 critic, thresholds at its 40 / 60 % quantiles) with --visevery V over --mepochs epochs: train_images_per_s as the
           loop reports it, the sheets written, the drain time at close()
  loops    `loop` in fresh child processes, alternated (parent tree, --visevery 100, --visevery 0) x --runs, with the spread of each;
           --parent DIR is a checkout of the parent commit (it writes no sheets; CGS_LIB_PATH points it at this tree's library, whose
           step kernels are the same sources)
One JSON line per case on stdout and, with --out FILE, appended to FILE.

    python tools/time_sheets.py kernel [--out profiles/sheets_time.jsonl]
    python tools/time_sheets.py loops --runs 3 --parent /path/to/parent/checkout
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(rows, out):
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


def kernel(a):
    import torch
    sys.path.insert(0, REPO)
    from cgs_amd import sheets, video
    from PIL import Image
    rows = []
    rs = np.random.RandomState(0)
    for n in (64, 512):
        A, B = (torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).cuda() for _ in range(2))
        Z = torch.from_numpy(rs.rand(n, 64, 64).astype(np.float32)).cuda()
        out = torch.empty(sheets.sheet_shape(n), dtype=torch.uint8, device="cuda")
        host = torch.empty(sheets.sheet_shape(n), dtype=torch.uint8, pin_memory=True)
        for _ in range(3):
            sheets.compose(A, B, Z, out=out)
            host.copy_(out, non_blocking=True)
        torch.cuda.synchronize()
        ms, ms_copy = [], []
        for _ in range(a.repeats):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            sheets.compose(A, B, Z, out=out)
            e[1].record()
            host.copy_(out, non_blocking=True)
            e[2].record()
            torch.cuda.synchronize()
            ms.append(e[0].elapsed_time(e[1]))
            ms_copy.append(e[1].elapsed_time(e[2]))
        nbytes = A.numel() + B.numel() + 4 * Z.numel() + out.numel()
        med = float(np.median(ms))
        rows.append({"case": "compose", "n": n, "bytes_read": A.numel() + B.numel() + 4 * Z.numel(), "bytes_written": out.numel(),
                     "us_median": round(med * 1e3, 1), "us_min": round(min(ms) * 1e3, 1), "us_max": round(max(ms) * 1e3, 1),
                     "GB_per_s": round(nbytes / med / 1e6, 1), "copy_to_pinned_us_median": round(float(np.median(ms_copy)) * 1e3, 1)})
        if n == 64:
            px = host.numpy().copy()
            font = video.resolve_font(sheets.FONT_SIZE)[0]
            vals = [rs.rand(n).tolist() for _ in range(5)]
            for level in (6, 1, 0):
                t = []
                for _ in range(a.png_repeats):
                    t0 = time.perf_counter()
                    img = sheets.draw_rows(Image.fromarray(px), sheets.segment_rows(*vals), n, font)
                    buf = io.BytesIO()
                    img.save(buf, format="PNG", compress_level=level)
                    t.append((time.perf_counter() - t0) * 1e3)
                rows.append({"case": "writer_thread_per_sheet", "n": n, "compress_level": level, "ships": level == sheets.COMPRESS_LEVEL,
                             "ms_median": round(float(np.median(t)), 1), "ms_min": round(min(t), 1), "MB": round(len(buf.getvalue()) / 1e6, 2),
                             "frames": "uniform noise"})
    stamp = {"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    emit([{**r, **stamp} for r in rows], a.out)


def loop(a):
    tree = os.path.abspath(a.tree or REPO)
    sys.path.insert(0, tree)
    sys.path.insert(1, REPO)                     # bench.py's helpers (the G1 weights) come from this tree
    import tempfile
    import bench                                 # (before torch: it sets the HIP runtime's environment as the benchmark does)
    import torch
    from cgs_amd import cli, handler
    pc, pm = bench.g1_weights()
    rs = np.random.RandomState(0)
    nfr = 16384
    X = rs.randint(0, 256, (nfr, 64, 64, 3)).astype(np.uint8)
    X[: nfr // 2] = (X[: nfr // 2] * 0.3).astype(np.uint8)
    Y = rs.rand(7, nfr)
    os.chdir(tempfile.mkdtemp(prefix="cgs_sheets_"))
    args = cli.parse_args(["--model", "m", "--dropout", "0.3", "--visevery", str(a.visevery), "--mepochs", str(a.mepochs),
                           "--saveevery", "1000"])
    H = handler.Handler(args)
    H.critic.load_state_dict(pc)
    H.masker.load_state_dict(pm)
    H.X, H.Y = X, Y
    preds = H._sweep_preds(H._engine(64), X).numpy()
    args.high_rew_thresh, args.low_rew_thresh = float(np.quantile(preds, 0.6)), float(np.quantile(preds, 0.4))
    t0 = time.perf_counter()
    H.segmentation_training()
    wall = time.perf_counter() - t0
    sheets_written = len([f for f in os.listdir("m/segment") if f.startswith("e")])
    emit([{"case": "loop", "tree": a.label or os.path.basename(tree), "visevery": a.visevery, "mepochs": a.mepochs,
           "train_images_per_s": round(H.train_images_per_s, 1), "sheets": sheets_written,
           "drain_s": round(getattr(H, "sheet_drain_s", 0.0), 3), "wall_s": round(wall, 2), "device": torch.cuda.get_device_name(0)}], a.out)


def loops(a):
    cases = ([("parent", a.parent, 100)] if a.parent else []) + [("sheets", REPO, 100), ("sheets", REPO, 0)]
    rates = {}
    for _ in range(a.runs):
        for label, tree, v in cases:                # alternated: parent, on, off, parent, on, off, ...
            env = dict(os.environ)
            if label == "parent":
                env["CGS_LIB_PATH"] = os.path.join(REPO, "critic-guided-segmentation-of-rewarding-objects-in-first-person-views_amd",
                                                   "libcgs_hip.so")
            cmd = [sys.executable, os.path.abspath(__file__), "loop", "--tree", tree, "--label", label, "--visevery", str(v),
                   "--mepochs", str(a.mepochs)] + (["--out", a.out] if a.out else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:                   # a failed child ends the series: nothing more is started on the GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"case": "loop"')][-1]
            print(line, flush=True)
            rates.setdefault((label, v), []).append(json.loads(line)["train_images_per_s"])
    rows = [{"case": "loops_summary", "tree": label, "visevery": v, "runs": len(x), "images_per_s": x,
             "median": float(np.median(x)), "spread_rel": round((max(x) - min(x)) / float(np.median(x)), 4)} for (label, v), x in rates.items()]
    emit(rows, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "loop", "loops"])
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--png-repeats", type=int, default=5)
    ap.add_argument("--visevery", type=int, default=100)
    ap.add_argument("--mepochs", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tree", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    {"kernel": kernel, "loop": loop, "loops": loops}[a.what](a)


if __name__ == "__main__":
    main()
