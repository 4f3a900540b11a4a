"""Do two builds of the library give the same bytes on the video path?  For a refactor of csrc/overlay*.hip / csrc/temporal*.hip.

    CGS_LIB_PATH=<pkg>/libcgs_hip_parent.so python tools/same_bytes.py run a.npz      (tools/build_rev.py REV parent builds it)
    python tools/same_bytes.py run b.npz                                              (the tree's library; a fresh process per library)
    python tools/same_bytes.py compare a.npz b.npz [--out profiles/FILE.jsonl]

`run` calls the five entry points on seeded inputs and keeps every output: cgs_overlay_compose and cgs_overlay_compose_tracks at 360 x 640
(16 pixels a thread), 72 x 100 (4) and 66 x 70 (1), layout "triple", outline 2, boxes 1, 3 frames with 4 tracked objects; cgs_temporal_flow at
search 4, cgs_temporal_smooth and cgs_temporal_smooth_mc (along those vectors) at radius 3 over 64 panned frames.  `compare` needs no GPU:
one JSON line per output with its shape, its SHA-256 in both files and whether the bytes are equal; exit status 1 when any differ."""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

SEED, SIZES, FRAMES, OBJECTS, SMOOTH_FRAMES, RADIUS, SEARCH = 0, ((360, 640), (72, 100), (66, 70)), 3, 4, 64, 3, 4


def run(path):
    import torch
    from cgs_amd import _lib, fit, objects, overlay, temporal
    from time_fit import frames_like_footage
    from time_overlay_tracks import lattice_masks
    from time_temporal_motion import panned
    rs = np.random.RandomState(SEED)
    out = {}
    for h, w in SIZES:
        guide = torch.from_numpy(frames_like_footage(FRAMES, h, w, rs)).to("cuda")
        z = torch.from_numpy(lattice_masks(FRAMES, OBJECTS)).to("cuda")
        up = fit.up(z, guide, fit.down(guide), thresh=0.5, want=("grey", "hard"))
        res = objects.label(z, thresh=0.5, inclusive=True, connectivity=8, max_objects=64)
        ids = objects.track(res.labels, iou=0.3).track
        out[f"cgs_overlay_compose {h}x{w}"] = overlay.compose(guide, up.grey, up.hard, outline=2, layout="triple")
        out[f"cgs_overlay_compose_tracks {h}x{w}"] = overlay.compose_tracks(guide, up.grey, up.hard, res.labels, ids, res.table, outline=2,
                                                                            boxes=1, layout="triple")
    zs, ls = panned(SMOOTH_FRAMES, rs)
    zd, ld = torch.from_numpy(zs).to("cuda"), torch.from_numpy(ls).to("cuda")
    fwd, bwd = temporal.flow(ld, SEARCH)
    out["cgs_temporal_flow fwd"], out["cgs_temporal_flow bwd"] = fwd, bwd
    out["cgs_temporal_smooth"] = temporal.smooth(zd, ld, RADIUS)
    out["cgs_temporal_smooth_mc"] = temporal.smooth(zd, ld, RADIUS, motion=(fwd, bwd))
    torch.cuda.synchronize()
    np.savez(path, **{k: v.cpu().numpy() for k, v in out.items()})
    print(f"{_lib.LIB_PATH}: {len(out)} outputs -> {path}")


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    sha = lambda v: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]
    lines = []
    for k in a.files:
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        lines.append(json.dumps({"case": "same_bytes", "output": k, "seed": SEED, "shape": list(a[k].shape), "dtype": str(a[k].dtype),
                                 "sha256_a": sha(a[k]), "sha256_b": sha(b[k]), "equal": bool(same)}))
    print("\n".join(lines))
    if out_path:
        with open(out_path, "a") as fp:
            fp.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(l)["equal"] for l in lines) else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else ""))
