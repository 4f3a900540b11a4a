#!/usr/bin/env python3
"""G13: the evaluation video of the reference's `main.py -test --model m --output-video v` (Handler.eval, main.py:1027-1087), captured
from the reference's OWN `main.main()` on a synthetic `red-trees/` set of 8 evaluated frames.

`ffmpeg` is replaced by a chain object that records what vidwrite (main.py:45-62) hands it: the `input` and `output` keyword arguments,
the output file name, `overwrite_output`, and every byte written to stdin.  The stream is the frames themselves (rawvideo rgb24), so no
encoder is needed.  Everything else is as for G9 / G10 (make_golden_loops.py, whose helpers are reused): the torchvision / cv2 / minerl
stubs, DejaVuSans at the relative font path Handler.__init__ and eval open, the G1 checkpoints.

The 8-column layout (-salience -crf) cannot be captured: the reference's crf() raises NameError (its densecrf import is commented out).

Run where the reference checkout is (make_golden_loops.REF), from any scratch directory:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <repo>/tests/golden/make_golden_video.py

Only DATA is written (g13_test_video.npz); no reference source is copied."""
import json
import os
import shutil
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ffmpeg_stub = types.ModuleType("ffmpeg")
sys.modules["ffmpeg"] = ffmpeg_stub
import make_golden_loops as loops  # noqa: E402  (stubs, sys.path to the reference, seeds)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from loop_inputs import synthetic_eval_set  # noqa: E402

N_SET, SEED = 116, 13            # X[100:5000:2] of 116 frames = 8 evaluated frames


class Chain:
    """ffmpeg.input(...).output(...).overwrite_output().run_async(pipe_stdin=True) -> process with stdin.write / close, wait."""

    def __init__(self):
        self.rec = {"stdin": bytearray(), "calls": []}

    def input(self, *args, **kw):
        self.rec["calls"].append("input")
        self.rec["input_args"], self.rec["input"] = list(args), kw
        return self

    def output(self, *args, **kw):
        self.rec["calls"].append("output")
        self.rec["output_args"], self.rec["output"] = list(args), kw
        return self

    def overwrite_output(self):
        self.rec["calls"].append("overwrite_output")
        return self

    def run_async(self, **kw):
        self.rec["calls"].append("run_async")
        self.rec["run_async"] = kw
        rec = self.rec

        class Stdin:
            def write(self, b):
                rec["stdin"] += bytes(b)

            def close(self):
                rec["calls"].append("close")

        class Proc:
            stdin = Stdin()

            def wait(self):
                rec["calls"].append("wait")
                return 0
        return Proc()


def g13(out_path):
    import PIL
    from PIL import features
    import main as refmain
    pc, pm = loops.g1()
    X, Yrgb = synthetic_eval_set(N_SET, SEED)
    tmp = loops.scratch()
    cwd = os.getcwd()
    os.chdir(tmp)
    chain = Chain()
    ffmpeg_stub.input = chain.input
    refmain.ffmpeg = ffmpeg_stub
    ious = []
    real_iou, real_init = refmain.Handler.get_iou, refmain.Handler.__init__

    def get_iou(self, A, B):
        r = real_iou(self, A, B)
        ious.append(float(r))
        return r

    def init(self, args):
        real_init(self, args)
        if not os.path.exists(self.save_paths["critic"]):
            os.makedirs(self.save_path, exist_ok=True)
            torch.save(pc, self.save_paths["critic"])
            torch.save(pm, self.save_paths["masker"])
    refmain.Handler.get_iou, refmain.Handler.__init__ = get_iou, init
    try:
        os.makedirs("red-trees")
        np.save("red-trees/X.npy", X)
        np.save("red-trees/Y.npy", Yrgb)
        argv = ["-test", "--model", "m", "--output-video", "v"]
        loops.run_main(argv)
        rec = chain.rec
        w, h = (int(v) for v in rec["input"]["s"].split("x"))
        raw = np.frombuffer(bytes(rec["stdin"]), dtype=np.uint8)
        assert raw.size % (w * h * 3) == 0, (raw.size, w, h)
        frames = raw.reshape(-1, h, w, 3)
        out = {"argv_json": np.array(json.dumps(argv)), "n_set": np.array(N_SET), "data_seed": np.array(SEED),
               "frames": frames, "ious": np.array(ious),
               "input_args_json": np.array(json.dumps(rec["input_args"])), "input_kwargs_json": np.array(json.dumps(rec["input"])),
               "output_args_json": np.array(json.dumps(rec["output_args"])), "output_kwargs_json": np.array(json.dumps(rec["output"])),
               "run_async_kwargs_json": np.array(json.dumps(rec["run_async"])), "calls_json": np.array(json.dumps(rec["calls"])),
               "file_name": np.array(rec["output_args"][0]), "stream_bytes": np.array(raw.size),
               "pil_version": np.array(PIL.__version__), "freetype_version": np.array(features.version("freetype2") or "")}
        np.savez_compressed(out_path, **out)
        print("wrote", os.path.basename(out_path), frames.shape, "file", rec["output_args"][0], "ious", ious,
              f"{os.path.getsize(out_path) / 1e6:.2f} MB")
    finally:
        refmain.Handler.get_iou, refmain.Handler.__init__ = real_iou, real_init
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    g13(os.path.join(HERE, "g13_test_video.npz"))
