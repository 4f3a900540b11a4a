#!/usr/bin/env python3
"""G15: the PNG sheets of the reference's training loops (main.py:203-226, 465-530), captured from the reference's OWN `main.main()`
on G9's synthetic frames (loop_inputs.synthetic_frames, seed 9), everything around the reference as for G9 / G14
(make_golden_loops.py, whose stubs, scratch directory -- DejaVuSans at the path Handler.__init__ opens -- and seeds are reused).

  segment  G9's command line (its thresholds included) plus `--visevery 1`, with the reference's own phase-1 critic (G9's
           critic_after_p1) and the G1 masker saved as the two checkpoints before main() looks for them: critic_pipe returns early
           (main.py:164-166) and the mask training starts from the state G9's did, a sheet after every step.  --dropout 0.
           Hooks: the masker's forward (Z of step 0), the critic's forward (its input A of step 0; pred, negpred, replacevalue,
           injectvalue), np.random.choice (the three index draws), torch.rand (the two shift draws), plt.hist (the sweep: which
           frames form the high and the low set).  Read back: segment/e0_b0.png and the directory listing.
  critic   `-train -masker '' --datasize 256 --testsize 64 --dropout 0 --cepochs 1` from the G1 weights, seeds as G9: four
           batches, critic/e0_b0.png after the first.  Hooks: the DataLoader's index column, the shift draws, the critic's forward.

Stored (data only, no reference source).  g15_sheets.npz: the argv, seeds, frame indices of A and B and the roll of step 0, Y and
the four prediction vectors, the listing; of the segment sheet rows 0-127 (the label band) in full, a SHA-256 per 64-pixel image
column of the rows below, columns 0, 1, 32, 63 of those rows in full; of the critic sheet rows 0-15 and 32-47 (its two label bands)
in full, a SHA-256 per image column of the whole sheet, columns 0, 1, 32, 63 in full; the PIL / FreeType versions and the font.
g15_sheets_z0.npz / g15_sheets_z1.npz: Z of step 0, images 0-31 / 32-63 (1 MiB of fp32 together: two files keep each under the
1 MiB a committed file may have).  The frames are regenerated from the seed by the tests, not stored.

Run where the reference checkout is (make_golden_loops.REF), from any scratch directory:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <repo>/tests/golden/make_golden_sheets.py
"""
import gzip
import hashlib
import json
import os
import pickle
import shutil
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_loops as loops  # noqa: E402  (stubs, sys.path to the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from loop_inputs import SEED_P1, SEED_P2, DATASIZE, TESTSIZE, synthetic_frames  # noqa: E402

FULL_COLUMNS = (0, 1, 32, 63)
CRITIC_DATASIZE, CRITIC_TESTSIZE = 256, 64


def column_hashes(sheet, row0=0):
    return [hashlib.sha256(np.ascontiguousarray(sheet[row0:, x:x + 64]).tobytes()).hexdigest() for x in range(0, sheet.shape[1], 64)]


def columns(sheet, row0=0):
    return np.stack([sheet[row0:, 64 * c:64 * c + 64] for c in FULL_COLUMNS])


def dataset(datasize, X, Y, I):
    os.makedirs("runs/data/straight", exist_ok=True)
    with gzip.GzipFile(f"runs/data/straight/Treechop-trunk-{datasize}-[0.98-0.97-0.96-0.95].pickle", "wb") as fp:
        pickle.dump((X, Y, I), fp)


def first(out):
    return out[0] if isinstance(out, tuple) else out


def segment_run(g9, pc_after_p1, pm):
    import main as refmain
    X, Y, I = synthetic_frames(DATASIZE + TESTSIZE, int(g9["data_seed"]))
    argv = json.loads(str(g9["argv_json"])) + ["--visevery", "1"]
    tmp = loops.scratch()
    cwd = os.getcwd()
    os.chdir(tmp)
    rec = loops.Recorders(refmain)
    got = {"on": False, "Z": [], "crit_in": [], "crit_out": [], "H": None, "ckpt": []}
    real_init, real_seg = refmain.Handler.__init__, refmain.Handler.segmentation_training

    def init(self, args):
        real_init(self, args)
        got["H"] = self
        os.makedirs(self.save_path, exist_ok=True)
        torch.save(pc_after_p1, self.save_paths["critic"])
        torch.save(pm, self.save_paths["masker"])
        got["ckpt"] = [self.save_paths["critic"], self.save_paths["masker"]]

        def critic_hook(mod, inp, out):
            if rec.choice and len(got["crit_out"]) < 4:          # the loop has drawn its first indices: step 0
                got["crit_in"].append(inp[0].detach().numpy().copy())
                got["crit_out"].append(first(out).detach().squeeze().numpy().copy())

        def masker_hook(mod, inp, out):
            if not got["Z"]:
                got["Z"].append(out.detach().numpy().copy())
        self.critic.register_forward_hook(critic_hook)
        self.masker.register_forward_hook(masker_hook)

    def segmentation_training(self):
        np.random.seed(SEED_P2)
        torch.manual_seed(SEED_P2)
        return real_seg(self)
    refmain.Handler.__init__, refmain.Handler.segmentation_training = init, segmentation_training
    try:
        dataset(DATASIZE, X, Y, I)
        rec.install()
        loops.run_main(argv)
        rec.remove()
        H = got["H"]
        listing = sorted(os.listdir("m/segment"))
        sheet = np.array(Image.open("m/segment/e0_b0.png"))
        font = H.font.getname()
    finally:
        rec.remove()
        refmain.Handler.__init__, refmain.Handler.segmentation_training = real_init, real_seg
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    args = H.args
    preds = rec.hist[0]
    pos_idx, neg_idx = np.flatnonzero(preds > args.high_rew_thresh), np.flatnonzero(preds < args.low_rew_thresh)
    Xtrain, Ytrain = X[:-TESTSIZE], Y[:, :-TESTSIZE]
    assert np.array_equal(Xtrain[pos_idx], H.Xpos) and np.array_equal(Xtrain[neg_idx], H.Xneg)
    Hidx, Lidx, Cidx = rec.choice[:3]
    a_frames, b_frames = np.concatenate((pos_idx[Hidx], neg_idx[Lidx])), neg_idx[Cidx]
    r1, r2 = rec.rand[:2]
    amount = int(args.shift * r1)
    roll = -amount if r2 > 0.5 else amount
    A = np.roll(Xtrain[a_frames], roll, axis=2)
    B = Xtrain[b_frames]
    # what the reference fed its critic in step 0 is A / 255 and B / 255 of exactly these frames
    assert np.array_equal(got["crit_in"][0], (torch.from_numpy(A).permute(0, 3, 1, 2).float() / 255.0).numpy())
    assert np.array_equal(got["crit_in"][1], (torch.from_numpy(B).permute(0, 3, 1, 2).float() / 255.0).numpy())
    Z = got["Z"][0]
    assert Z.shape == (64, 1, 64, 64) and Z.dtype == np.float32 and sheet.shape == (448, 4096, 3)
    assert np.array_equal(sheet[128:192], np.concatenate(A, axis=1)) and np.array_equal(sheet[192:256], np.concatenate(B, axis=1))
    Y0 = np.concatenate((H.Ypos[args.rewidx, Hidx], H.Yneg[args.rewidx, Lidx]))
    pred, negpred, replacevalue, injectvalue = got["crit_out"]
    out = {"argv_json": np.array(json.dumps(argv)), "seed": np.array(SEED_P2), "data_seed": g9["data_seed"],
           "datasize": np.array(DATASIZE), "testsize": np.array(TESTSIZE), "checkpoint_names": np.array(got["ckpt"]),
           "listing_json": np.array(json.dumps(listing)), "a_frames": a_frames.astype(np.int32), "b_frames": b_frames.astype(np.int32),
           "choice": np.concatenate((Hidx, Lidx, Cidx)).astype(np.int32), "shift_draws": np.array([r1, r2]), "roll": np.array(roll),
           "Y": Y0.astype(np.float64), "pred": pred.astype(np.float32), "negpred": negpred.astype(np.float32),
           "replacevalue": replacevalue.astype(np.float32), "injectvalue": injectvalue.astype(np.float32),
           "segment_band": sheet[:128], "segment_sha256": np.array(column_hashes(sheet, 128)), "segment_columns": columns(sheet, 128),
           "full_columns": np.array(FULL_COLUMNS), "font": np.array(json.dumps(list(font)))}
    return out, Z[:, 0]


def critic_run(pc, pm):
    import main as refmain
    X, Y, I = synthetic_frames(CRITIC_DATASIZE + CRITIC_TESTSIZE, 9)
    argv = ["-train", "-masker", "", "--model", "m", "--datasize", str(CRITIC_DATASIZE), "--testsize", str(CRITIC_TESTSIZE),
            "--dropout", "0", "--cepochs", "1"]
    tmp = loops.scratch()
    cwd = os.getcwd()
    os.chdir(tmp)
    rec = loops.Recorders(refmain)
    got = {"pred": []}
    real_cp = refmain.Handler.critic_pipe

    def critic_pipe(self, mode="train", test=0):
        self.critic.load_state_dict(pc)
        self.masker.load_state_dict(pm)
        self.train_loader = loops.LoaderProxy(self.train_loader, rec.batches)
        self.critic.register_forward_hook(lambda mod, inp, out: got["pred"].append(first(out).detach().squeeze().numpy().copy()))
        np.random.seed(SEED_P1)
        torch.manual_seed(SEED_P1)
        return real_cp(self, mode, test)
    refmain.Handler.critic_pipe = critic_pipe
    try:
        dataset(CRITIC_DATASIZE, X, Y, I)
        rec.install()
        loops.run_main(argv)
        rec.remove()
        listing = sorted(os.listdir("m/critic"))
        sheet = np.array(Image.open("m/critic/e0_b0.png"))
    finally:
        rec.remove()
        refmain.Handler.critic_pipe = real_cp
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    idx = rec.batches[0]
    r1, r2 = rec.rand[:2]
    amount = int(12 * r1)
    roll = -amount if r2 > 0.5 else amount
    Xb = np.roll(X[:-CRITIC_TESTSIZE][idx], roll, axis=2)
    assert sheet.shape == (64, 64 * len(idx), 3)
    return {"critic_argv_json": np.array(json.dumps(argv)), "critic_seed": np.array(SEED_P1), "critic_datasize": np.array(CRITIC_DATASIZE),
            "critic_testsize": np.array(CRITIC_TESTSIZE), "critic_listing_json": np.array(json.dumps(listing)),
            "critic_idx": idx.astype(np.int32), "critic_roll": np.array(roll), "critic_shift_draws": np.array([r1, r2]),
            "critic_Y": Y[1, :-CRITIC_TESTSIZE][idx].astype(np.float32), "critic_pred": got["pred"][0].astype(np.float32),
            "critic_bands": np.stack((sheet[0:16], sheet[32:48])), "critic_sha256": np.array(column_hashes(sheet)),
            "critic_columns": columns(sheet), "critic_frames_equal": np.array(np.array_equal(sheet[16:32], np.concatenate(Xb, axis=1)[16:32]))}


def g15(out_dir):
    import PIL
    from PIL import features
    pc, pm = loops.g1()
    g9 = dict(np.load(os.path.join(HERE, "g9_train_loop.npz")))
    pc_after_p1 = {k[len("critic_after_p1/"):]: torch.from_numpy(v) for k, v in g9.items() if k.startswith("critic_after_p1/")}
    out, Z = segment_run(g9, pc_after_p1, pm)
    out.update(critic_run(pc, pm))
    out.update({"pil_version": np.array(PIL.__version__), "freetype_version": np.array(features.version("freetype2") or ""),
                "raqm": np.array(bool(features.check("raqm")))})
    np.savez_compressed(os.path.join(out_dir, "g15_sheets.npz"), **out)
    np.savez_compressed(os.path.join(out_dir, "g15_sheets_z0.npz"), Z=Z[:32])
    np.savez_compressed(os.path.join(out_dir, "g15_sheets_z1.npz"), Z=Z[32:])
    for f in ("g15_sheets.npz", "g15_sheets_z0.npz", "g15_sheets_z1.npz"):
        size = os.path.getsize(os.path.join(out_dir, f))
        assert size < 2 ** 20, (f, size)
        print(f"wrote {f}: {size / 1e6:.2f} MB")
    print("segment listing", json.loads(str(out["listing_json"]))[:4], "...; critic listing", json.loads(str(out["critic_listing_json"])),
          "; font", str(out["font"]), "; A/B frames in the critic sheet equal:", bool(out["critic_frames_equal"]))


if __name__ == "__main__":
    g15(HERE)
