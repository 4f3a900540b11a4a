#!/usr/bin/env python3
"""G14: the -vismasker / -viscritic videos of the reference (Handler.visualize, main.py:702-884), captured from the reference's OWN
`main.main()` on G9's synthetic frames (loop_inputs.synthetic_frames, seed 9) with the G1 checkpoints and --testsize 10.  (Twelve frames
would put the file over the 1 MiB a committed file may have: the noise tiles do not compress.  Not a size = 1 mod 128: the reference's
squeeze() then breaks its own concatenate.)

    -train -critic '' -masker '' -vismasker --model m --datasize 40 --testsize 10       (three videos of 256 x 768)
    the same command with -viscritic                                                     (three videos of 256 x 512)

Everything around the reference is as for G13 (make_golden_video.py, make_golden_loops.py, whose helpers are reused).  `ffmpeg` is the
recording chain of make_golden_video.py, one record per vidwrite call.  The empty `cv2` stub gets the two functions make_video calls:

  resize(pic, (0, 0), fx=4, fy=4, interpolation=INTER_NEAREST)   np.repeat by fx along the columns and fy along the rows, which is
                                                                 what INTER_NEAREST computes for an integer scale factor
                                                                 (dst[y][x] = src[y // 4][x // 4]);
  cvtColor(img, COLOR_RGB2BGR)                                   the channels reversed; the reference discards the result.

Forward hooks on the reference's critic and masker record `preds` and `masks` of every batch; a wrapper around numpy.argsort records
the sortings of main.py:880-883.  Stored (data only, no reference source): argv, N, the seeds, preds, masks, values, the sortings, the
file names and ffmpeg keyword arguments, the full streams of the three -vismasker videos, a SHA-256 per frame of the three -viscritic
videos, the PIL / FreeType versions.

Run where the reference checkout is (make_golden_loops.REF), from any scratch directory:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <repo>/tests/golden/make_golden_vis.py
"""
import gzip
import hashlib
import json
import os
import pickle
import shutil
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ffmpeg_stub = types.ModuleType("ffmpeg")
sys.modules["ffmpeg"] = ffmpeg_stub
import make_golden_loops as loops  # noqa: E402  (stubs, sys.path to the reference)
from make_golden_video import Chain  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from loop_inputs import synthetic_frames  # noqa: E402

DATASIZE, TESTSIZE, SEED = 40, 10, 9
cv2_stub = sys.modules["cv2"]
cv2_stub.INTER_NEAREST, cv2_stub.COLOR_RGB2BGR = 0, 4


def resize(src, dsize, fx=0, fy=0, interpolation=None):
    """cv2.resize for the one call make_video makes (main.py:852): dsize (0, 0), integer fx = fy, INTER_NEAREST -- every source pixel
    repeated fx times along x and fy times along y, dtype kept."""
    assert tuple(dsize) == (0, 0) and interpolation == cv2_stub.INTER_NEAREST and fx == int(fx) >= 1 and fy == int(fy) >= 1
    return np.repeat(np.repeat(src, int(fy), axis=0), int(fx), axis=1)


def cvtColor(src, code):
    assert code == cv2_stub.COLOR_RGB2BGR
    return src[..., ::-1]


cv2_stub.resize, cv2_stub.cvtColor = resize, cvtColor


class Chains:
    """One recording Chain per ffmpeg.input(...) call, i.e. per video."""

    def __init__(self):
        self.recs = []

    def input(self, *args, **kw):
        c = Chain()
        self.recs.append(c.rec)
        return c.input(*args, **kw)


def run(flag, pc, pm, X, Y, I):
    import main as refmain
    tmp = loops.scratch()
    cwd = os.getcwd()
    os.chdir(tmp)
    chains = Chains()
    ffmpeg_stub.input = chains.input
    refmain.ffmpeg = ffmpeg_stub
    refmain.cv2 = cv2_stub
    got = {"preds": [], "masks": [], "sortings": [], "ckpt": []}
    real_init, real_argsort = refmain.Handler.__init__, np.argsort

    def init(self, args):
        real_init(self, args)
        os.makedirs(self.save_path, exist_ok=True)
        torch.save(pc, self.save_paths["critic"])
        torch.save(pm, self.save_paths["masker"])
        got["ckpt"] = [self.save_paths["critic"], self.save_paths["masker"]]
        self.critic.register_forward_hook(lambda mod, inp, out: got["preds"].append(out[0].detach().squeeze().cpu().numpy().copy()))
        self.masker.register_forward_hook(lambda mod, inp, out: got["masks"].append(out.detach().cpu().numpy().copy()))

    def argsort(a, *args, **kw):
        r = real_argsort(a, *args, **kw)
        if getattr(a, "shape", None) == (TESTSIZE,):
            got["sortings"].append(np.asarray(r).copy())
        return r
    refmain.Handler.__init__ = init
    np.argsort = argsort
    try:
        os.makedirs("runs/data/straight")
        with gzip.GzipFile(f"runs/data/straight/Treechop-trunk-{DATASIZE}-[0.98-0.97-0.96-0.95].pickle", "wb") as fp:
            pickle.dump((X, Y, I), fp)
        argv = ["-train", "-critic", "", "-masker", "", flag, "--model", "m", "--datasize", str(DATASIZE), "--testsize", str(TESTSIZE)]
        loops.run_main(argv)
    finally:
        np.argsort = real_argsort
        refmain.Handler.__init__ = real_init
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    streams = []
    for rec in chains.recs:
        w, h = (int(v) for v in rec["input"]["s"].split("x"))
        raw = np.frombuffer(bytes(rec["stdin"]), dtype=np.uint8)
        assert raw.size == TESTSIZE * w * h * 3, (raw.size, w, h)
        streams.append(raw.reshape(TESTSIZE, h, w, 3))
    # main.py:880-883 reverse the argsort: the sortings as make_video receives them
    sortings = [s[::-1].copy() for s in got["sortings"]]
    return argv, chains.recs, streams, np.concatenate(got["preds"]), got["masks"], sortings, got["ckpt"]


def g14(out_path):
    import PIL
    from PIL import features
    pc, pm = loops.g1()
    X, Y, I = synthetic_frames(DATASIZE + TESTSIZE, SEED)
    argv_m, recs_m, streams_m, preds_m, masks_m, sort_m, ckpt = run("-vismasker", pc, pm, X, Y, I)
    argv_c, recs_c, streams_c, preds_c, masks_c, sort_c, _ = run("-viscritic", pc, pm, X, Y, I)
    assert len(streams_m) == len(streams_c) == 3 and not masks_c and np.array_equal(preds_m, preds_c)
    assert all(np.array_equal(a, b) for a, b in zip(sort_m, sort_c)) and len(sort_m) == 2
    masks = np.concatenate(masks_m)
    values = np.stack((Y[1, -TESTSIZE:], preds_m), axis=0)             # main.py:804 (--rewidx 1)

    def meta(recs):
        return json.dumps([{"file": r["output_args"][0], "input_args": r["input_args"], "input": r["input"], "output": r["output"],
                            "run_async": r["run_async"], "calls": r["calls"]} for r in recs])
    out = {"argv_vismasker_json": np.array(json.dumps(argv_m)), "argv_viscritic_json": np.array(json.dumps(argv_c)),
           "n": np.array(TESTSIZE), "datasize": np.array(DATASIZE), "data_seed": np.array(SEED),
           "checkpoint_names": np.array(ckpt), "preds": preds_m.astype(np.float32), "masks": masks.astype(np.float32),
           "values": values, "sorting_pred": sort_m[0].astype(np.int64), "sorting_gt": sort_m[1].astype(np.int64),
           "vismasker_ffmpeg_json": np.array(meta(recs_m)), "viscritic_ffmpeg_json": np.array(meta(recs_c)),
           "vismasker_frames": np.stack(streams_m),
           "viscritic_sha256": np.array([[hashlib.sha256(f.tobytes()).hexdigest() for f in s] for s in streams_c]),
           "pil_version": np.array(PIL.__version__), "freetype_version": np.array(features.version("freetype2") or ""),
           "raqm": np.array(bool(features.check("raqm")))}
    np.savez_compressed(out_path, **out)
    print("wrote", os.path.basename(out_path), out["vismasker_frames"].shape, [r["output_args"][0] for r in recs_m],
          "preds", preds_m.min(), preds_m.max(), f"{os.path.getsize(out_path) / 1e6:.2f} MB")


if __name__ == "__main__":
    g14(os.path.join(HERE, "g14_vis.npz"))
