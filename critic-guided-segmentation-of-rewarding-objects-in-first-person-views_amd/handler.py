"""Host-side orchestration of the ``-train`` and ``-process`` paths: the reference's ``Handler`` surface
(main.py:66-156, 158-236, 238-312, 314-575, 584-591, 1103-1223) with its inner loops replaced by the fused
HIP engine.  Same method names, same checkpoint / dataset file naming, same output file names.

Out of scope here: --trainasvis and --purevis.  The PNG sheets of the two training loops (main.py:203-226,
465-530) and the two histograms of the contrastive split (main.py:255-264) are written through sheets.py: the segment sheet's pixels
are composed on the GPU and every PNG is encoded by a writer thread, off the step path.  ``collect_data`` reads an
existing gz-pickle or, when the ``minerl`` package is importable, builds it from MineRL episodes exactly as the reference labels them
(the MineRL download / decoder itself is the package's; it is absent from this image).  ``-eval`` (section 8 f2) is carried over, with
the evaluation video of ``-test`` / ``--output-video`` (video.py: frames composed on the GPU); ``-crf`` runs the dense CRF of crf.py
(exact mean field on the GPU) in both ``-process`` and ``-eval``.  ``-viscritic`` / ``-vismasker`` (main.py:702-884) write their videos
through vis.py (frames composed on the GPU).
"""
import gzip
import math
import os
import pickle

import numpy as np
import torch

from . import _lib, dataformat, evaluate, metrics, parallel, process, sheets, video, vis
from .crf import GRID_KEYS, dense_crf, grid_points, parse_crf_grid
from .engine import HourglassEngine
from .evaluate import _json_safe, write_json    # noqa: F401  (_json_safe: tests read it from here)
from .generic_engine import GenericEngine
from .nets import NewCritic, UnetDecoder


def checkpoint_names(args):
    """Checkpoint file stems of the reference: ``k=v`` joined by '-' for TRUTHY values only (main.py:86-91), e.g.
    critic-rewidx=1-cepochs=15-datamode=trunk-datasize=100000-shift=12-chfak=1-dropout=0.3 / masker-mepochs=1-L1=0.5-inject=True."""
    d = args.__dict__
    critic_args = "-".join(f"{a}={d[a]}" for a in
                           ["rewidx", "cepochs", "datamode", "datasize", "threshrew", "shift", "chfak", "dropout"] if d[a])
    masker_args = "-".join(f"{a}={d[a]}" for a in ["mepochs", "L1", "L2", "inject"] if d[a])
    return critic_args, masker_args


def pyplot():
    """matplotlib's pyplot on the Agg backend, or None where matplotlib cannot be imported: the plots are then left out."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except Exception:
        return None
    return plt


class Handler:
    def __init__(self, args):
        self.args = args
        if not torch.cuda.is_available():
            raise _lib.CgsError("this build runs the Hourglass on an MI355X through HIP kernels; no GPU is visible "
                                "and there is no CPU fallback")
        # one process per GPU under torchrun (RANK / LOCAL_RANK / WORLD_SIZE): the training steps then all-reduce their gradients
        # and the contrastive sweep is sharded by frame; a plain `python main.py` is world size 1
        self.pg = parallel.init_from_env()
        self.rank, local, self.world = parallel.env_world()
        self.device = f"cuda:{local}" if self.world > 1 else "cuda"
        print("device:", self.device)
        # attribute names, directory layout and checkpoint file names are the reference's (main.py:66-107): they are the contract
        self.criticname, self.maskername = "critic", "masker"
        self.ious, self.bestepoch = (0, 0), 0
        self.reset_models()
        self.models = {self.criticname: self.critic, self.maskername: self.masker}
        self.critic_args, self.masker_args = checkpoint_names(args)
        root = f"{args.name}/"
        self.path, self.data_path = root, "runs/data/straight/"
        self.train_path, self.result_path, self.save_path = (root + sub for sub in ("train/", "results/", "saves/"))
        self.save_paths = {name: f"{self.save_path}{name}-{tag}.pt"
                           for name, tag in ((self.criticname, self.critic_args), (self.maskername, self.masker_args))}
        self._engines = {}
        self.crf_reports, self.sweep = [], None      # --crf-grid / --thresh-grid / --salience-grid: the tables of Handler.crf, the dict of eval_sweep.json
        self.objects = None         # -eval -objects: the dict of eval_objects.json
        self.matches = None         # -eval -objects --match-iou: the dict of eval_match.json
        self.tracks = None          # -eval -objects --track-iou: the dict of eval_tracks.json
        self.boundary = None        # -eval --boundary-tol: the dict of eval_boundary.json
        self.clean = None           # -eval --clean: the dict of eval_clean.json
        self.cut = None             # -eval --graph-cut: the dict of eval_cut.json
        self._trace = None          # tests set a dict of lists (Handler.start_trace): per-step indices / losses of the two training loops

    def start_trace(self):
        """Keep every step's frame indices, shift and loss values of critic_pipe / segmentation_training (device clones, no host sync)."""
        self._trace = {"p1_idx": [], "p1_loss": [], "p2_idx": [], "p2_roll": [], "p2_loss": []}
        return self._trace

    # ------------------------------------------------------------------ models / checkpoints
    def reset_models(self):
        args = self.args
        self.critic = NewCritic(bottleneck=args.neck, chfak=args.chfak, dropout=args.dropout).to(self.device)
        self.masker = UnetDecoder(bottleneck=args.neck, chfak=args.chfak).to(self.device)
        if args.separate:       # main.py:110-111: a second critic feeds the masker; like the reference it is never checkpointed
            self.sepcrit = NewCritic(bottleneck=args.neck, chfak=args.chfak, dropout=args.dropout).to(self.device)

    def load_models(self, modelnames=[]):
        """Loads the named checkpoints (all when empty); False at the first missing file (main.py:130-141)."""
        for name in (modelnames or list(self.models)):
            ckpt = self.save_paths[name]
            if not os.path.isfile(ckpt):
                if not self.args.train:
                    print(f"{ckpt} not found")
                return False
            print("loading:", ckpt)
            self.models[name].load_state_dict(torch.load(ckpt, map_location=torch.device(self.device)))
        return True

    def save_models(self, modelnames=[]):
        if self.rank != 0:          # replicas are identical: one writer
            return
        os.makedirs(self.save_path, exist_ok=True)
        for name in (modelnames or list(self.models)):
            print("saving:", self.save_paths[name])
            torch.save(self.models[name].state_dict(), self.save_paths[name])

    # ------------------------------------------------------------------ data
    def collect_data(self):
        args = self.args
        filepath = dataformat.dataset_path(args.envname, args.datamode, args.datasize, args.gammas, self.data_path)
        print("collecting dataset at", filepath)
        if not os.path.exists(filepath):
            return self._collect_fresh(filepath)
        print("loading existing dataset...")
        X, Y, I = dataformat.read_dataset(filepath)
        print("finished loading exisiting dataset")
        return X, Y, I

    def _collect_fresh(self, filepath):
        """main.py:1286-1359: no pickle yet -> read MineRL episodes through the `minerl` package (imported lazily; absent in this image,
        where only a test stub stands in for it), label them (dataformat.build_dataset: trunk filter main.py:1325, clipped discounted
        rewards main.py:1336-1346) and write the gz-pickle.  Like the reference, the pickle holds the rows that were filled and the
        RETURNED arrays are the full --datasize + --testsize buffers (zero rows at the end when the episodes ran out)."""
        args = self.args
        try:
            import minerl
        except ImportError as e:
            raise FileNotFoundError(
                f"{filepath} not found and the `minerl` package is not installed. This build reads the reference's gz-pickle (X uint8 "
                "[N,64,64,3], Y float [7,N], I uint16 [N]); collecting it from MineRL needs `minerl` + its data (SURVEY.md 2.3).") from e
        root = os.getenv("MINERL_DATA_ROOT", "data/")
        env = f"MineRL{args.envname}VectorObf-v0"
        os.makedirs(self.data_path, exist_ok=True)
        if not os.path.exists(f"{root}/{env}"):
            minerl.data.download(root, experiment=env)
        data = minerl.data.make(env, data_dir=root, num_workers=args.workers[0], worker_batch_size=args.workers[1])
        size = args.datasize + args.testsize
        print("collecting straight data set with", args.datasize, "+", args.testsize, "frames")

        def episodes():
            for name in data.get_trajectory_names():
                state, _action, reward, _next, _done = zip(*data.load_data(name))
                yield np.stack([s["pov"] for s in state]), np.array(reward)
        X, Y, I = dataformat.build_dataset(episodes(), size, mode=args.datamode, gammas=[float(g) for g in args.gammas.split("-")])
        rows = len(X)
        with gzip.GzipFile(filepath, "wb") as fp:
            pickle.dump((X, Y, I), fp)
        Xf = np.zeros((size, 64, 64, 3), dtype=np.uint8)
        Yf = np.zeros((dataformat.Y_ROWS, size), dtype=np.float64)
        If = np.zeros(size, dtype=np.uint16)
        Xf[:rows], Yf[:, :rows], If[:rows] = X, Y, I
        return Xf, Yf, If

    def load_data(self, batch_size=64):
        """Train / test split (the last --testsize frames are the test set) and the --threshrew binarisation (main.py:113-128)."""
        X, Y, I = self.collect_data()
        cut, thr = -self.args.testsize, self.args.threshrew
        label = (lambda y: (y > thr).astype(np.float64)) if thr else (lambda y: y)
        self.X, self.Y, self.I = X[:cut], label(Y[:, :cut]), I[:cut]
        self.XX, self.YY, self.II = X[cut:], label(Y[:, cut:]), I[cut:]
        print("dataset shapes", X.shape, Y.shape, self.X.shape, self.Y.shape)
        self.batch_size = batch_size

    def _batches(self):
        """Shuffled mini-batches of (X uint8, Y[rewidx], frame indices) in the order the reference's
        DataLoader(TensorDataset(X, Y.t(), arange), batch_size, shuffle=True) yields them (main.py:125-129): the index stream comes from
        the same torch.utils.data.DataLoader over the frame indices, so a seeded run draws from the global torch RNG exactly as the
        reference does (one base-seed draw per epoch, one sampler-seed draw, the permutation from the sampler's private generator) and
        the shift draws that follow line up with the reference's (pinned by the G9 capture, tests/test_gpu_loops.py)."""
        order = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.arange(len(self.X))), batch_size=self.batch_size, shuffle=True)
        for (idx_t,) in order:
            idx = idx_t.numpy()
            yield torch.from_numpy(self.X[idx]), torch.from_numpy(self.Y[self.args.rewidx, idx]).float(), idx

    def _shift_draw(self):
        """The two draws main.py:585-586 takes from the global torch RNG, as a signed roll along the width (positive = the
        reference's "right" branch, negative = its "left" branch)."""
        amount = int(self.args.shift * torch.rand(1))
        return -amount if bool(torch.rand(1) > 0.5) else amount

    def shift_batch(self, X):
        """Whole-batch circular roll along the width (main.py:584-591): one torch.roll instead of the reference's cat of slices."""
        return torch.roll(X, shifts=Handler._shift_draw(self), dims=2)

    # ------------------------------------------------------------------ engines
    def _generic_size(self):
        return self.args.chfak != 1 or self.args.neck != 32

    def _engine(self, n, live=True, training=False, dropout=None):
        """The engine for batches of n images: the fused fixed-shape kernels at chfak = 1, neck = 32 (the code default), the
        shape-generic ones for every other model size (the paper's chfak = 5).  dropout: override of --dropout (0 after a
        -directeval evaluation, which leaves the reference's modules in eval mode for the rest of the training)."""
        a = self.args
        p_drop = a.dropout if dropout is None else dropout
        key = (n, live, p_drop)
        if key not in self._engines:
            first = next(iter(self._engines.values()), None)
            kw = dict(device=self.device, dropout=p_drop, lfak=a.lfak, L1=a.L1, L2=a.L2, inject=a.inject, live=live,
                      threshrew=a.threshrew, share_with=first, process_group=self.pg, separate=bool(a.separate),
                      staticnorm=bool(a.staticnorm))
            if self._generic_size():
                e = GenericEngine(n, chfak=a.chfak, neck=a.neck, **kw)
            else:
                e = HourglassEngine(n, **kw)
            if first is None:
                # modules and engine share one parameter buffer from now on
                e.adopt(self.critic, self.masker, self.sepcrit if a.separate else None)
                parallel.broadcast_params_(e.flat, self.pg)
            self._engines[key] = e
        return self._engines[key]

    def _reset_adam(self):
        for e in self._engines.values():
            e.reset_optimizer()
            break

    # ------------------------------------------------------------------ phase 1: critic regression
    def _refuse_unbuilt_flags(self):
        """Flags the reference reads on this path that this build does not implement: refuse instead of training something else.
        None at present: -staticnorm '' (mask regulariser weighted by 1 - pred, main.py:415-418) runs in the fused features.0 + mix
        backward, which every step takes."""

    def critic_pipe(self, mode="train", test=0):
        args = self.args
        self._refuse_unbuilt_flags()
        if args.cload and self.load_models([self.criticname]):
            print("loaded critic, no new training")
            return
        result_path = self.path + "critic/"
        os.makedirs(result_path, exist_ok=True)
        if self.rank == 0:                        # (data parallel: one writer)
            with open(result_path + "log.txt", "w") as log_file:
                log_file.write(f"{self.args}\n\n")
        llog = []
        self.critic.train()
        # -directeval (main.py:179-180): Handler.eval() puts critic and masker into eval mode and never back (main.py:900-902; the
        # re-.train() at main.py:1019-1020 is commented out), so -- unless -noevalmode -- the reference then trains with Dropout OFF
        self._p1_dropout = 0.0 if (args.directeval and not args.noevalmode) else None
        self._engine(self.batch_size, training=True, dropout=self._p1_dropout)
        self._reset_adam()                       # a fresh torch.optim.Adam(critic.parameters()) (main.py:178)
        if args.directeval:
            self.eval()
            if args.noevalmode:
                self.critic.train()
        # critic/e{epoch}_b{b}.png every 100th batch (main.py:203-226), rank 0's shard: encoded by the writer thread
        writer = sheets.SheetWriter() if self.rank == 0 else None
        try:
            for epoch in range(int(mode == "test") or args.cepochs):
                for b_idx, (X, Y, idx) in enumerate(self._batches()):
                    if args.shift:
                        X = self.shift_batch(X)
                    eng = self._engine(len(X), dropout=self._p1_dropout)
                    losses = eng.phase1_step(X.contiguous().to(self.device, non_blocking=True), Y.to(self.device, non_blocking=True))
                    if writer is not None and not b_idx % sheets.CRITIC_EVERY:
                        # the prediction is the forward's, before the update (as the reference's); its copy is enqueued before the next step
                        writer.submit_critic(sheets.segment_path(result_path, epoch, b_idx), X, Y, eng.last_phase1_pred())
                    if self._trace is not None:      # (tests: the loop-level pin G9) no host sync: device clones
                        self._trace["p1_idx"].append(idx.copy())
                        self._trace["p1_loss"].append(losses[:1].clone())
                    if not b_idx % 10:
                        val = float(losses[0])       # the only host sync, every 10th batch
                        llog.append(val)
                        print(f"critic e{epoch + 1} b{b_idx}", val, end="\r")
                if not (epoch + 1) % args.saveevery:
                    self.save_models(modelnames=[self.criticname])
                if self.rank == 0:                    # (data parallel: one writer)
                    self._plot(result_path + "_loss.png", {"Train Loss": llog})
        finally:
            if writer is not None:
                writer.close()
        print()

    # ------------------------------------------------------------------ contrastive split
    def _sweep_preds(self, eng, X, batchsize=4096):
        """Eval-mode critic value of every frame (main.py:245-253), on the device in large batches; under data parallelism each
        rank sweeps a contiguous shard of the frames and the shards are all-gathered."""
        n = len(X)
        lo, hi = 0, n
        per = n
        if self.world > 1:
            per = -(-n // self.world)
            lo, hi = min(n, self.rank * per), min(n, (self.rank + 1) * per)
        out = torch.zeros(per, device=self.device)
        for b in range(lo, hi, batchsize):
            e = min(hi, b + batchsize)
            pred, _ = eng.infer(torch.from_numpy(X[b:e]).to(self.device), want_mask=False)
            out[b - lo:e - lo] = pred
        if self.world > 1:
            parts = [torch.zeros_like(out) for _ in range(self.world)]
            torch.distributed.all_gather(parts, out, group=self.pg)
            out = torch.cat(parts)[:n]
        return out.cpu()

    def extract_contrastive_data(self):
        """Splits the training frames by the critic's value into the high set (> --high-rew-thresh) and the low set
        (< --low-rew-thresh) (main.py:238-312), keeps both resident on the device as uint8 and sets up the reference's index
        sampler (32 high + 32 low frames for A, 64 low frames for B, drawn with replacement from the global numpy RNG)."""
        args = self.args
        self.critic.eval()
        eng = self._engine(2 * 32)
        os.makedirs(self.path, exist_ok=True)
        if args.critic or args.cload:
            preds = self._sweep_preds(eng, self.X)
            if self.rank == 0:                    # main.py:255-264: the two histograms of the split
                self._hist(self.path + f"pred_idx{args.rewidx}_hist.png", preds.numpy())
                self._hist(self.path + f"GT_idx{args.rewidx}_hist.png", self.Y[args.rewidx])
            positives, negatives = preds > args.high_rew_thresh, preds < args.low_rew_thresh
        else:
            print("no critic provided -> using random pos and neg frames")
            positives = torch.rand(len(self.X)) > 0.5
            if self.world > 1:                    # every rank must hold the same split (same set sizes, same number of steps)
                flag = positives.to(torch.uint8).to(self.device)
                torch.distributed.broadcast(flag, src=0, group=self.pg)
                positives = flag.cpu().bool()
            negatives = ~positives
            preds = torch.cat((positives, negatives), dim=0)
        npos, nneg = int(positives.sum()), int(negatives.sum())
        if self.rank == 0:      # the reference leaves the two counts behind as an (empty) file name
            open(self.path + f"{npos}>{args.high_rew_thresh}__{nneg}<{args.low_rew_thresh}.txt", "w").close()
        assert npos >= 500 and nneg >= 500
        assert preds[positives].float().mean() > args.high_rew_thresh
        pos, neg = positives.numpy(), negatives.numpy()
        self.Xpos, self.Ypos = self.X[pos], self.Y[:, pos]
        self.Xneg, self.Yneg = self.X[neg], self.Y[:, neg]
        # device-resident copies: a training step then gathers its frames with one index upload, no host frames involved
        dev = self.device
        self._Xpos_d, self._Xneg_d = torch.from_numpy(self.Xpos).to(dev), torch.from_numpy(self.Xneg).to(dev)
        self._ypos_d = torch.from_numpy(np.ascontiguousarray(self.Ypos[args.rewidx])).float().to(dev)
        self._yneg_d = torch.from_numpy(np.ascontiguousarray(self.Yneg[args.rewidx])).float().to(dev)
        self.XposIdxs, self.XnegIdxs, self.ContrastIdxs = np.arange(npos), np.arange(nneg), np.arange(nneg)
        self.contrastive_batchsize = 32
        cb = self.contrastive_batchsize
        self.get_contrastive_idxs = lambda: (np.random.choice(self.XposIdxs, cb), np.random.choice(self.XnegIdxs, cb),
                                             np.random.choice(self.ContrastIdxs, 2 * cb))

    # ------------------------------------------------------------------ phase 2: mask training
    def segmentation_training(self):
        """main.py:314-575: per step three index draws (numpy RNG, as the reference), the two shift draws (torch RNG), ONE 128-entry
        index upload; the frames are gathered, rolled and trained on without leaving the device.  Every --visevery steps rank 0
        leaves segment/e{epoch}_b{b}.png (main.py:465-530) behind: composed on the GPU from the step's own tensors right after the
        step, copied out asynchronously and encoded by a writer thread (sheets.py) -- no host sync, no RNG draw.  --visevery 0
        writes none (this build's own meaning of 0: the reference divides by zero there)."""
        import time
        args = self.args
        self._refuse_unbuilt_flags()
        self.extract_contrastive_data()
        train_path = self.path + "segment/"
        os.makedirs(train_path, exist_ok=True)
        if self.rank == 0:
            with open(train_path + "log.txt", "w") as log_file:
                log_file.write(f"{self.args}\n\n")
        log = []
        self.critic.train()
        self.masker.train()
        n = 2 * self.contrastive_batchsize
        # -directeval (main.py:337-338) leaves the modules in eval mode (see critic_pipe): the training that follows runs without Dropout
        eng = self._engine(n, live=args.live, training=True, dropout=0.0 if (args.directeval and not args.noevalmode) else None)
        self._reset_adam()                       # a fresh Adam over critic+masker (live) or masker (frozen)
        if args.directeval:
            self.eval()
            if args.noevalmode:
                self.critic.train()
                self.masker.train()
        # The host runs ahead of the device (it only syncs every 10th step): ONE pinned buffer would be overwritten with later draws
        # while earlier asynchronous uploads are still queued, and several steps would train on the same (or a torn) index set.
        # A ring of pinned buffers, each reused only after ITS upload's event has completed, keeps one fresh draw per step.
        ring = 16
        idx_hosts = [torch.empty(2 * n, dtype=torch.int64).pin_memory() for _ in range(ring)]
        idx_events = [None] * ring
        idx_dev = torch.empty(2 * n, dtype=torch.int64, device=self.device)
        self._last_idx_draws = []                # (debug / tests) the host draws of the last few steps, in order
        names = ["replace", "inject", "norm", "live-critic"]
        steps, steps_t0, t0, dt = 0, 0, time.perf_counter(), 0.0
        writer = sheets.SheetWriter() if (self.rank == 0 and args.visevery > 0) else None
        drain = 0.0
        try:
            for epoch in range(args.mepochs):
                for b_idx in range(math.ceil(self.Xpos.shape[0] / self.contrastive_batchsize)):
                    Hidx, Lidx, Cidx = self.get_contrastive_idxs()
                    slot = steps % ring
                    if idx_events[slot] is not None:
                        idx_events[slot].synchronize()                   # the upload that last used this buffer has finished
                    idx_host = idx_hosts[slot]
                    idx_host.copy_(torch.from_numpy(np.concatenate((Hidx, Lidx, Cidx))))
                    idx_dev.copy_(idx_host, non_blocking=True)
                    idx_events[slot] = torch.cuda.Event()
                    idx_events[slot].record()
                    if getattr(self, "_record_idx_draws", False):
                        self._last_idx_draws.append(idx_host.clone())
                    roll = self._shift_draw() if args.shift else 0      # torch.roll(X, roll, dims=2): dst[x] = src[x - roll]
                    eng.gather_contrastive(self._Xpos_d, self._Xneg_d, self._ypos_d, self._yneg_d, idx_dev, shift_px=(-roll) % 64)
                    losses = eng.phase2_step()
                    steps += 1
                    if writer is not None and sheets.wanted(args.visevery, b_idx):
                        # views of the step's own buffers (forward with the pre-update weights, as the reference draws); the compose
                        # and the copies are enqueued here, before the next gather_contrastive: stream order protects them
                        A, B, Z, *values = eng.last_phase2_views()
                        y_host = np.concatenate((self.Ypos[args.rewidx, Hidx], self.Yneg[args.rewidx, Lidx]))      # float64, as main.py:346-351
                        writer.submit_segment(sheets.segment_path(train_path, epoch, b_idx), A, B, Z, y_host, values, args.inject)
                    if self._trace is not None:      # (tests: the loop-level pin G9)
                        self._trace["p2_idx"].append(np.concatenate((Hidx, Lidx, Cidx)))
                        self._trace["p2_roll"].append(roll)
                        self._trace["p2_loss"].append(losses[:6].clone())
                    if steps == 20:                                      # throughput is reported for the steady state (after the
                        torch.cuda.synchronize()                         # eager first step and the graph capture)
                        t0, steps_t0, dt = time.perf_counter(), steps, 0.0
                    if not b_idx % 10:                                   # the only host sync
                        c, r, i, l1, l2, total = losses[:6].tolist()
                        log.append((r, i if args.inject else 0, l1 + l2, c if args.live else 0))
                        msg = f"e{epoch} b{b_idx}" + (f"    live-critic {c}" if args.live else "") + f"   replace: {r}"
                        msg += (f"   inject: {i}" if args.inject else "") + (f"   L1: {l1}" if args.L1 else "") + (f"   L2: {l2}" if args.L2 else "")
                        print(msg, end="\r")
                torch.cuda.synchronize()
                dt += time.perf_counter() - t0            # (plots and checkpoints are not part of the step throughput)
                if self.rank == 0:
                    llog = np.array(log)
                    self._plot(train_path + "_loss.png", {nm: llog[:, k] for k, nm in enumerate(names)})
                if not (epoch + 1) % args.saveevery:
                    self.save_models(modelnames=[self.maskername])
                t0 = time.perf_counter()
        finally:
            if writer is not None:           # the ring drains outside the timed region, like the plots and checkpoints
                t_close = time.perf_counter()
                writer.close()
                drain = time.perf_counter() - t_close
        self.train_images_per_s = (steps - steps_t0) * n * self.world / dt if dt > 0 else 0.0
        print(f"\nmask training: {steps} steps of {n} A-images, {steps - steps_t0} of them in {dt:.3f} s = {self.train_images_per_s:.0f} images/s"
              + (f" over {self.world} ranks" if self.world > 1 else ""))
        if writer is not None:
            k = len(writer.written)
            print(f"sheets: {k} written to {train_path}, {writer.encode_s / max(k, 1) * 1e3:.1f} ms of the writer thread per sheet; "
                  f"drain at close {drain * 1e3:.1f} ms (not part of the throughput)")
        self.sheet_drain_s = drain
        self.save_models(modelnames=[self.maskername])

    # ------------------------------------------------------------------ -process: masks for a folder of images
    def segment(self, folder):
        from PIL import Image
        print("STARTING SEGMENTATION...")
        args = self.args
        os.makedirs(self.path, exist_ok=True)
        if args.noevalmode and args.salience:
            raise NotImplementedError("-noevalmode together with -salience (Dropout inside the saliency backward) is not implemented")
        if args.process_salience and not args.salience:
            raise ValueError("-process_salience needs -salience (the reference collects the maps only then, main.py:1136-1147)")
        if getattr(args, "source_video", ""):           # (this build's flag) a video file in, an overlay video out; `folder` is not read
            return self._segment_video(args.source_video)
        if getattr(args, "fit", False):                 # (this build's flag) frames of any one size; everything below stays as it is
            return self._segment_fit(folder)
        files, stems = process.list_folder(folder)
        file_bytes = np.stack([np.array(Image.open(os.path.join(folder, f)))[..., :3] for f in files])        # NHWC, as the files hold them
        frames = file_bytes / 255.0                                                                              # NHWC float64 in [0,1]
        fp16 = bool(getattr(args, "fp16", False))      # (this build's switch) BASELINE config 4: fp16 layers on the uint8 frames

        def to_device(chunk):
            t = torch.from_numpy(chunk).float().to(self.device)
            return (t * 255.0).round().to(torch.uint8) if fp16 else t

        preds, M, sal = self._sweep_masks(frames, to_device, "segmentation in progress", want_saliency=bool(args.salience), fp16=fp16)
        print()
        print("postprocessing...")
        cols = [M]                      # one column per output kind, in the order of process.KINDS
        if args.binarymaskthreshold:
            cols.append(M >= args.binarymaskthreshold)
        if args.crf:                    # main.py:1169-1172 (with --binarymaskthreshold 0 this column lands in position 2)
            cols.append(self.crf(frames, M, None))
        refined, hard = cols[-1] if args.crf else None, "crf-mask"      # the refined hard mask --clean and -objects read, and its name
        if getattr(args, "graph_cut", None):    # (this build's flag) not a column: {stem}-cut-mask.png and cut.json; it takes the CRF mask's place
            os.makedirs(args.mask_output_imgs, exist_ok=True)
            thresh, res = process.cut_source(args, np.ascontiguousarray(file_bytes, dtype=np.uint8), M[:, 0], self.device)
            refined, hard = res.mask.cpu().numpy()[:, None], "cut-mask"
            process.write_cut(args, thresh, res.stats, stems[:len(frames)], self.rank, pngs=refined[:, 0])
        cleaned = None
        if getattr(args, "clean", None):        # (this build's flag) not a column either: {stem}-clean-mask.png and clean.json
            os.makedirs(args.mask_output_imgs, exist_ok=True)
            source, thresh, res = process.clean_source(args, M[:, 0], refined[:, 0] if refined is not None else None, self.device, hard)
            cleaned = res.mask
            process.write_clean(args, source, thresh, res.counts, stems[:len(frames)], self.rank, pngs=cleaned.cpu().numpy())
        if getattr(args, "objects", False):     # (this build's flag) not a column: the by-position naming and the strip stay as they are
            process.objects_and_tracks(args, M, refined, stems[:len(frames)], self.device, self.rank, hard=hard,
                                       low=np.ascontiguousarray(file_bytes, dtype=np.uint8)
                                       if getattr(args, "track_motion", 0) or getattr(args, "track_reid", None)
                                       or getattr(args, "object_value", False) else None,
                                       cleaned=cleaned, infer=self._value_infer())
        if args.process_salience:       # main.py:1176-1197
            sal_maps, sal_hard = self._saliency_post(sal, preds, args.salience_thresh, args.salglobal)
            cols += [sal_maps, sal_hard]
            if args.crf:                # main.py:1200-1203
                cols.append(self.crf(frames, sal_maps, None))
        out_dir = args.mask_output_imgs
        os.makedirs(out_dir, exist_ok=True)
        to_u8 = lambda a: (a * 255).astype(np.uint8)
        process.write_columns(out_dir, stems[:len(frames)], to_u8(frames), [to_u8(c[:, 0]) for c in cols], args.concatenated)
        return M

    FIT_CHUNK_FRAMES, FIT_CHUNK_BYTES = 128, 256 << 20      # a chunk of -process -fit: at most so many frames and frame bytes

    def _segment_fit(self, folder):
        """-process -fit: a folder of frames of one size, 64 to 4096 pixels a side.  Per chunk of at most 128 frames and about 256 MB the
        uint8 frames are uploaded, shrunk to 64 x 64 on the GPU (fit.down), run through the network as -process runs 64 x 64 frames (and
        through -crf on the shrunk frames), and every column is brought back to the frame's size along the frame's edges (fit.up): the
        mask as grey, thresholded at --binarymaskthreshold (inclusive, main.py:1164), the CRF labels thresholded at 0.5.  The files keep
        their names and the by-position rule, at H x W; -objects and --track-iou work on the 64 x 64 masks, in the 64 x 64 grid's
        coordinates.  Rank 0 leaves {R}/fit.json.  Returns the 64 x 64 masks [n,1,64,64] as segment does."""
        from PIL import Image
        from . import fit
        args = self.args
        files, stems = process.list_folder(folder)
        if not files:
            raise ValueError(f"-fit: {folder!r} holds no files")
        size = None
        for f in files:
            with Image.open(os.path.join(folder, f)) as im:
                wh = im.size
            if size is None:
                try:
                    fit.check_size(wh[1], wh[0])
                except ValueError as e:
                    raise ValueError(f"-fit: {f}: {e}") from None
                size = wh
            elif wh != size:
                raise ValueError(f"-fit: {f} is {wh[1]}x{wh[0]}, the files before it are {size[1]}x{size[0]}: a folder holds one size")
        W, H = size
        fp16 = bool(getattr(args, "fp16", False))
        thr = args.binarymaskthreshold
        self.critic.eval()
        self.masker.eval()
        eng = self._engine(2 * 32)
        out_dir = args.mask_output_imgs
        os.makedirs(out_dir, exist_ok=True)
        sig = dict(sigma_s=args.fit_spatial, sigma_r=args.fit_range)
        step = process.chunk_frames(self.FIT_CHUNK_FRAMES, self.FIT_CHUNK_BYTES, H, W)
        masks, crf_masks = [], []
        spec = getattr(args, "clean", None)              # --clean: per chunk the cleaned 64 x 64 masks and their counts, on the device
        cleaned, clean_counts, clean_head = [], [], None
        cut_spec = getattr(args, "graph_cut", None)      # --graph-cut: per chunk the cut 64 x 64 masks and their stats, on the device
        cut_masks, cut_stats, cut_thr = [], [], None
        lows = [] if getattr(args, "objects", False) and (getattr(args, "track_motion", 0) or getattr(args, "track_reid", None)
                                                          or getattr(args, "object_value", False)) else None     # --track-motion / --track-reid / --object-value: the shrunk frames
        unit = process.unit_table(self.device)
        for lo in range(0, len(files), step):
            print("segmentation in progress", round(lo / len(files), 2), end="%\r")
            host = np.stack([np.array(Image.open(os.path.join(folder, f)))[..., :3] for f in files[lo:lo + step]])    # NHWC uint8
            guide = torch.from_numpy(np.ascontiguousarray(host, dtype=np.uint8)).to(self.device)
            low = fit.down(guide)
            if lows is not None:
                lows.append(low)
            Z = process.fit_infer(eng, low, unit, fp16, bool(args.noevalmode))
            M = Z.cpu().numpy()[:, None]
            masks.append(M)
            up = fit.up(Z.contiguous(), guide, low, thresh=thr if thr else None, want=("grey", "hard") if thr else ("grey",), **sig)
            cols = [up.grey.cpu().numpy()]
            if thr:
                cols.append(up.hard.cpu().numpy() * np.uint8(255))
            if args.crf:
                labels = self.crf(low.cpu().numpy() / 255.0, M, None)
                crf_masks.append(labels)
                dev_labels = torch.from_numpy(np.ascontiguousarray(labels[:, 0]).view(np.uint8)).to(self.device)
                cols.append(fit.up(dev_labels, guide, low, thresh=0.5, want=("hard",), **sig).hard.cpu().numpy() * np.uint8(255))
            if cut_spec:                                 # on the shrunk frames; brought to H x W as the CRF labels are; not a column
                cut_thr, cres = process.cut_source(args, low, Z.contiguous(), self.device)
                cut_masks.append(cres.mask)
                cut_stats.append(cres.stats)
                big = fit.up(cres.mask.view(torch.uint8), guide, low, thresh=0.5, want=("hard",), **sig).hard
                if self.rank == 0:
                    process.write_cut_pngs(out_dir, stems[lo:lo + len(host)], big.cpu().numpy())
            if spec:                                     # brought to H x W as the CRF labels are; not a column
                source, thresh, res = process.clean_source(args, Z, labels[:, 0] if args.crf else (cres.mask if cut_spec else None),
                                                           self.device, "cut-mask" if cut_spec else "crf-mask")
                clean_head = (source, thresh)
                cleaned.append(res.mask)
                clean_counts.append(res.counts)
                big = fit.up(res.mask.view(torch.uint8), guide, low, thresh=0.5, want=("hard",), **sig).hard
                if self.rank == 0:
                    process.write_clean_pngs(out_dir, stems[lo:lo + len(host)], big.cpu().numpy())
            process.write_columns(out_dir, stems[lo:lo + len(host)], host, cols, args.concatenated)
        print()
        M = np.concatenate(masks, axis=0)
        crf_mask = np.concatenate(crf_masks, axis=0) if args.crf else None
        if cut_spec:
            crf_mask = torch.cat(cut_masks).cpu().numpy()[:, None]
            process.write_cut(args, cut_thr, torch.cat(cut_stats), stems[:len(files)], self.rank)
        if spec:
            process.write_clean(args, *clean_head, torch.cat(clean_counts), stems[:len(files)], self.rank)
        if getattr(args, "objects", False):
            process.objects_and_tracks(args, M, crf_mask, stems[:len(files)], self.device, self.rank,
                                       low=torch.cat(lows) if lows is not None else None, cleaned=torch.cat(cleaned) if spec else None,
                                       infer=self._value_infer(), hard="cut-mask" if cut_spec else "crf-mask")
        write_json(f"{out_dir}/fit.json", {"frame_size": [H, W], "net_size": [fit.SIDE, fit.SIDE], "sigma_spatial": args.fit_spatial,
                                           "sigma_range": args.fit_range, "radius": fit.RADIUS, "frames": len(files)}, self.rank)
        return M

    VIDEO_CHUNK_FRAMES, VIDEO_CHUNK_BYTES = 128, 256 << 20    # a chunk of -process --source-video: at most so many frames and frame bytes

    def _segment_video(self, path):
        """-process --source-video IN --overlay-video OUT: the frames of a video file, 64 to 4096 pixels a side, decoded by ffmpeg a chunk
        of at most 128 frames and about 256 MB at a time (video_in.read_chunks).  Two stages, so that the smoother has its lookahead:
          A  upload, fit.down, the network exactly as _segment_fit feeds it;
          B  --smooth R > 0: temporal.smooth over a rolling device stack -- the last R frames before the chunk, the chunk, the first R
             after it, with their shrunk frames, with --smooth-motion S > 0 along temporal.flow of that same window -- then fit.up (the
             grey byte, and the hard mask at --binarymaskthreshold, inclusive; no hard mask and so no outline at threshold 0),
             overlay.compose, an asynchronous copy into a pinned double buffer and the encoder (video.ffmpeg_argv with the probed rate).
             With --overlay-tracks T the smoothed masks are labelled (objects.label at the threshold, 8-connected, --overlay-min-area),
             objects.TrackStream numbers the objects through the chunks as objects.track numbers the whole stack, and
             overlay.compose_tracks draws each in its track's colour with its box and number in place of overlay.compose.
             With --overlay-motion S the stream tracks along temporal.flow's backward vectors of the chunk's shrunk frames and the one
             before them (kept across the chunk boundary); the vectors stay on the device, 128 bytes a frame pair, for the reports.
             With --overlay-fill (and --overlay-gap G >= 1) stage B splits: B1 is the above up to the labelling and pushes into an
             objects.FillStream, which returns the frames that became final -- all but the last G pushed -- with the masks that bridged
             links jump over filled in (objects.fill's result for the whole stack); B2 takes as many frames from the queue `held`, sets
             the smoothed mask to 1 on the cells whose filled label differs from the segmented one, adds the carried objects' table rows
             to the labeller's (disjoint: new objects are numbered behind the frame's largest label), and runs fit.up and
             overlay.compose_tracks(age=), which draws a carried object hatched.  flush() behind the last chunk draws the last G frames.
             The encoder gets the same frames in the same order, G frames later; G more frames of guide stay on the device.
        Stage A of chunk c + 1 runs before stage B of chunk c (a chunk waits until R frames after it are there, or the stream has ended).
        No PNG is written.  Rank 0 leaves {R}/{stem of OUT}.json, with --overlay-tracks also {R}/{stem}-objects.json and
        {R}/{stem}-tracks.json (process.video_reports; skipped beyond objects.TRACK_MAX_FRAMES frames, the video is complete all the
        same).  With --overlay-clean SPEC the masks are replaced, after --smooth and before fit.up and the labelling, by clean.clean's
        `gated` at --binarymaskthreshold: tint, outline, track labels and the reports follow the cleaned mask, and {stem}.json gains
        "clean".  Returns the 64 x 64 masks [n,1,64,64], the smoothed ones with --smooth, the gated ones with --overlay-clean."""
        from collections import deque
        import subprocess
        from . import clean, cli, fit, objects, overlay, temporal, video_in
        args = self.args
        spec = getattr(args, "overlay_clean", None)                           # --overlay-clean: the parsed spec
        clean_counts = torch.zeros(len(clean.COUNTS), dtype=torch.int64, device=self.device) if spec else None
        track_iou = getattr(args, "overlay_tracks", None)
        track_gap = int(getattr(args, "overlay_gap", 0) or 0)                 # --overlay-gap: objects.TrackStream's max_gap
        track_motion = int(getattr(args, "overlay_motion", 0) or 0)           # --overlay-motion: the search range of its block vectors
        track_fill = bool(getattr(args, "overlay_fill", False)) and track_iou is not None and track_gap > 0      # --overlay-fill
        stream = (objects.FillStream if track_fill else objects.TrackStream)(
            track_iou, max_objects=overlay.MAX_TRACK_OBJECTS, max_gap=track_gap, motion=bool(track_motion)) if track_iou is not None else None
        held = deque()                                 # --overlay-fill: chunks through B1 whose frames are not all drawn yet
        before_low, fields = None, []                  # --overlay-motion: the shrunk frame before the chunk; every chunk's vectors
        ffmpeg, ffprobe = video_in.find_ffmpeg(), video_in.find_ffprobe()
        W, H, rate = video_in.probe(path, ffprobe)
        k = args.overlay_panels
        cli.check_video_size(W, H, k)                  # before the first frame is decoded
        fp16 = bool(getattr(args, "fp16", False))
        thr, R, S = args.binarymaskthreshold, args.smooth, getattr(args, "smooth_motion", 0)
        self.critic.eval()
        self.masker.eval()
        eng = self._engine(2 * 32)
        out_dir, out_path = args.mask_output_imgs, args.overlay_video
        os.makedirs(out_dir, exist_ok=True)
        if os.path.dirname(out_path):
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
        sig = dict(sigma_s=args.fit_spatial, sigma_r=args.fit_range)
        step = process.chunk_frames(self.VIDEO_CHUNK_FRAMES, self.VIDEO_CHUNK_BYTES, H, W)
        unit = process.unit_table(self.device)
        masks = []
        proc = subprocess.Popen(video.ffmpeg_argv(ffmpeg, out_path, k * W, H, framerate=rate), stdin=subprocess.PIPE)
        writer = video.FrameWriter(proc.stdin, (H, k * W, 3), step)
        pending = deque()                              # chunks through stage A, waiting for stage B: (guide, low, Z)
        tail = None                                    # (Z, low) of the last R frames before the first pending chunk, unsmoothed
        # --smooth-motion: the forward vectors' summed length and the number of saturated ones, on the device; the number of vectors
        moved, vectors = torch.zeros(2, dtype=torch.float64, device=self.device) if S else None, 0

        def stage_a(host):
            guide = torch.from_numpy(host).to(self.device)        # (a blocking copy: the reader may refill the buffer afterwards)
            low = fit.down(guide)
            return guide, low, process.fit_infer(eng, low, unit, fp16, bool(args.noevalmode)).contiguous().clone()

        def stage_b2(filled):
            """Draws the frames of `filled` (objects.Filled, in stream order): the oldest held ones."""
            at, n_final = 0, int(filled.labels.shape[0])
            while at < n_final:
                guide, low, Zs, seg, table, lo = held[0]
                m = min(n_final - at, len(Zs) - lo)    # one chunk's frames at a time: at most `step`, what a submit takes
                cut, new = slice(lo, lo + m), slice(at, at + m)
                labels = filled.labels[new]
                Zf = torch.where(labels != seg[cut], torch.ones_like(Zs[cut]), Zs[cut])
                up = fit.up(Zf, guide[cut], low[cut], thresh=thr if thr else None, want=("grey", "hard") if thr else ("grey",), **sig)
                writer.submit(overlay.compose_tracks(guide[cut], up.grey, up.hard, labels, filled.track[new], table[cut] + filled.table[new],
                                                     color=args.overlay_color, alpha256=args.overlay_alpha256,
                                                     outline=args.overlay_outline, boxes=args.overlay_boxes, layout=args.overlay_layout,
                                                     age=filled.age[new]))
                at += m
                held[0][5] = lo + m
                if held[0][5] == len(Zs):
                    held.popleft()

        def stage_b():
            nonlocal tail, moved, vectors, before_low, clean_counts
            guide, low, Z = pending.popleft()
            if R:
                zs, ls = [Z], [low]
                need = R
                for _g, l2, z2 in pending:             # the head of what follows, R frames of it
                    if need <= 0:
                        break
                    zs.append(z2[:need])
                    ls.append(l2[:need])
                    need -= len(zs[-1])
                f0 = 0
                if tail is not None:
                    zs.insert(0, tail[0])
                    ls.insert(0, tail[1])
                    f0 = len(tail[0])
                zw, lw, motion = torch.cat(zs), torch.cat(ls), None
                if S:
                    motion = temporal.flow(lw, S)
                    own = motion[0][max(f0 - 1, 0):f0 + len(Z) - 1].to(torch.float64)      # the pairs that end in this chunk: each pair once
                    moved = moved + torch.stack((own.pow(2).sum(dim=-1).sqrt().sum(), (own.abs().amax(dim=-1) >= S).sum().to(torch.float64)))
                    vectors += own.shape[0] * own.shape[1] * own.shape[2]
                Zs = temporal.smooth(zw, lw, R, args.smooth_range, f0, f0 + len(Z), motion=motion)
                before = (torch.cat((tail[0], Z)), torch.cat((tail[1], low))) if tail is not None else (Z, low)
                tail = (before[0][-R:], before[1][-R:])
            else:
                Zs = Z
            if spec:                                   # per frame, so the chunking does not show: gated >= thr is the cleaned mask
                res = clean.clean(Zs, thresh=thr, inclusive=True, want_gated=True, **clean.spec_kwargs(spec))
                Zs, clean_counts = res.gated, clean_counts + res.counts.sum(dim=0, dtype=torch.int64)
            masks.append(Zs.cpu().numpy()[:, None])
            if not track_fill:                         # (--overlay-fill upsamples in B2, the filled mask)
                up = fit.up(Zs, guide, low, thresh=thr if thr else None, want=("grey", "hard") if thr else ("grey",), **sig)
            if stream is not None:
                res = objects.label(Zs, thresh=thr, inclusive=True, connectivity=8, min_area=args.overlay_min_area,
                                    max_objects=overlay.MAX_TRACK_OBJECTS)
                if track_motion:                       # row i: from frame i of the chunk to the frame before it in the stream
                    first = before_low is None
                    bwd = temporal.flow(low if first else torch.cat((before_low, low)), track_motion)[1]
                    if first:                          # no frame before the stream's first: a row the stream ignores
                        bwd = torch.cat((bwd.new_zeros((1,) + tuple(bwd.shape[1:])), bwd))
                    before_low = low[-1:].clone()
                    fields.append(bwd)
                    ids = stream.push(res.labels, bwd)
                else:
                    ids = stream.push(res.labels)
                if track_fill:                         # B1 ends here: `ids` is the FillStream's Filled for the frames that became final
                    held.append([guide, low, Zs, res.labels, res.table, 0])
                    return stage_b2(ids)
                frames = overlay.compose_tracks(guide, up.grey, up.hard, res.labels, ids, res.table,
                                                color=args.overlay_color, alpha256=args.overlay_alpha256, outline=args.overlay_outline,
                                                boxes=args.overlay_boxes, layout=args.overlay_layout)
            else:
                frames = overlay.compose(guide, up.grey, up.hard, color=args.overlay_color, alpha256=args.overlay_alpha256,
                                         outline=args.overlay_outline, layout=args.overlay_layout)
            writer.submit(frames)

        failure, done = None, 0
        try:
            for host in video_in.read_chunks(path, step, size=(W, H), ffmpeg=ffmpeg):
                print("segmentation in progress, frame", done, end="\r")
                done += len(host)
                pending.append(stage_a(host))
                while pending and sum(len(c[2]) for c in list(pending)[1:]) >= max(R, 1):
                    stage_b()
            while pending:
                stage_b()
            if track_fill and done:
                stage_b2(stream.flush())
            writer.close()
        except BrokenPipeError as e:
            failure = e
        finally:
            try:
                writer.close()
            except BaseException as e:               # (the first failure is the one reported)
                failure = failure or e
            try:
                proc.stdin.close()
            except BrokenPipeError:
                pass
            rc = proc.wait()
        if rc != 0 or isinstance(failure, BrokenPipeError):
            raise RuntimeError(f"ffmpeg exited with status {rc} while writing {out_path}" + (f" ({failure})" if failure else ""))
        if failure is not None:
            raise failure
        print()
        M = np.concatenate(masks, axis=0)
        stem = os.path.basename(out_path).rsplit(".", 1)[0]
        smooth = {"radius": R, "sigma_t": temporal.sigma_t(R), "sigma_range": args.smooth_range} if R else None
        if R and S:                                    # (the one host sync of the motion figures)
            length, saturated = moved.tolist()
            smooth["motion"] = {"search": S, "block": temporal.BLOCK, "mean_cells_per_frame": length / max(vectors, 1),
                                "saturated": saturated / max(vectors, 1)}
        tracks = {}
        if stream is not None:
            reports = None
            if len(M) <= objects.TRACK_MAX_FRAMES:
                reports = process.video_reports(args, M, stem, self.device, self.rank,
                                                bwd=torch.cat(fields)[1:] if track_motion else None)
            else:
                print(f"--overlay-tracks: {len(M)} frames are more than the {objects.TRACK_MAX_FRAMES} one report holds: the video is complete, "
                      f"{stem}-objects.json and {stem}-tracks.json are not written")
            tracks = {"tracks": {"iou": track_iou, "min_area": args.overlay_min_area, "boxes": args.overlay_boxes,
                                 "scale": overlay.scale(H, W), "max_objects": overlay.MAX_TRACK_OBJECTS, "n_tracks": int(stream.n_tracks),
                                 **({"gap": track_gap} if track_gap else {}), **({"motion": track_motion} if track_motion else {}),
                                 **({"fill": dict(zip(("objects", "cells", "dropped", "vanished"), (int(v) for v in stream.totals.tolist())))}
                                    if track_fill else {}),
                                 "reports": reports}}
        write_json(f"{out_dir}/{stem}.json", {
            "frame_size": [H, W], "frames": len(M), "rate": rate, "layout": args.overlay_layout, "color": list(args.overlay_color),
            "alpha256": args.overlay_alpha256, "outline": args.overlay_outline, "threshold": thr,
            "smooth": smooth,
            "sigma_spatial": args.fit_spatial, "sigma_range": args.fit_range, **tracks,
            **({"clean": {**clean.clean_report(clean_counts, spec), "frames": len(M)}} if spec else {})}, self.rank)
        return M

    def _value_infer(self):
        """--object-value: the critic as objects.value asks it, uint8 frames [b,64,64,3] -> values [b], always fp32 and eval mode (None
        without the flag)."""
        if not getattr(self.args, "object_value", False):
            return None
        eng = self._engine(2 * 32)
        return lambda X: eng.infer(X, want_mask=False)[0]

    def _sweep_masks(self, X, to_device, progress, want_saliency=False, fp16=False, batchsize=128, train_mode=None):
        """The inference loop shared by -process and -eval (main.py:1130-1151, 900-953): eval-mode critic + masker over X in batches
        of 128, optionally the saliency baseline |d mean(pred) / d batch| summed over the colour channels.
        Returns (preds [n], masks [n,1,64,64], saliency [n,1,64,64] or None) as numpy.  train_mode: None follows -noevalmode."""
        args = self.args
        train_mode = bool(args.noevalmode) if train_mode is None else train_mode
        self.critic.eval()
        self.masker.eval()
        eng = self._engine(2 * 32)
        preds, masks, sal = [], [], []
        for lo in range(0, len(X), batchsize):
            print(progress, round(lo / len(X), 2), end="%\r")
            batch = to_device(X[lo:lo + batchsize])
            if want_saliency:
                _unused, dx = eng.saliency(batch)
                sal.append(dx.abs().sum(dim=-1)[:, None].cpu().numpy())
            if fp16:
                pred, Z = eng.infer(batch, fp16=True)
            else:
                pred, Z = eng.infer(batch, train_mode=train_mode)                 # -noevalmode: Dropout stays on (main.py:1109-1118)
            preds.append(pred.cpu().numpy())
            masks.append(Z.cpu().numpy()[:, None])
        cat = lambda parts: np.concatenate(parts, axis=0)
        return cat(preds), cat(masks), (cat(sal) if want_saliency else None)

    @staticmethod
    def _saliency_post(salM, preds, thresh, salglobal):
        """main.py:976-1003 / 1176-1197: normalise the |gradient| maps (by the global mean of the non-negative part x thresh, or by
        each map's k-th smallest value), weight them by the critic's prediction, clip at 1, threshold.  Returns (maps, hard uint8)."""
        tiny = np.finfo(np.float64).tiny                      # (= sys.float_info.min: keeps 0 / 0 finite)
        if salglobal:
            scale = np.where(salM >= 0, salM, 0.0).mean() * thresh
        else:
            n, hw = salM.shape[0], salM.shape[-1] * salM.shape[-2]
            scale = np.sort(salM.reshape(n, 1, hw), axis=-1)[:, :, int(hw * thresh), None, None]
        out = np.minimum(salM / (scale + tiny) * preds.reshape(-1, 1, 1, 1), 1.0)
        return out, (out > thresh).astype(np.uint8)

    # ------------------------------------------------------------------ -crf: dense-CRF refinement of mask stacks
    def crf(self, imgs, mask, Y, skip=1):
        """main.py:1226-1263: every `skip`-th frame's mask [n,1,h,w] (P of label 1) refined by the two-label dense CRF, the whole stack in
        one GPU call per grid point; the other frames keep their mask.  Returns (mask >= 1) as NCHW bool.  imgs: NHWC uint8, or float in
        [0,1] (then (255 * img).astype(uint8) as the reference, which gives back the uint8 frame).  Like the reference, every 50th refined
        frame leaves {path}crf/{i}_mask.png, {i}_img.png, {i}_crf.png (rank 0).
        The grid is --crf-grid's (crf.parse_crf_grid), by default the reference's one point (crf.REFERENCE_PARAMS); then Y is not used.
        With --crf-grid the frames, the probabilities and Y[::skip] are uploaded once, every point's labels are scored on the GPU against
        Y[::skip] with the reference's sum(Y & M) / sum(Y | M) (metrics.iou_counts), the table goes to self.crf_reports, and the labels
        of the BEST point come back (ties: the first in grid order; an empty union ranks last) -- the reference computes the ranking
        and then returns the labels of the LAST point.  A grid of several points needs Y."""
        grid = getattr(self.args, "crf_grid", "")
        points = grid_points(parse_crf_grid(grid))
        if len(points) > 1 and Y is None:
            raise ValueError("a CRF grid of more than one point is scored against the labels Y, and there are none (-process)")
        mask = np.array(mask, copy=True)
        imgs = np.asarray(imgs)[::skip]
        frames = imgs if imgs.dtype == np.uint8 else (255 * imgs).astype(np.uint8)
        prob = np.ascontiguousarray(mask[::skip, 0], dtype=np.float32)
        dev_frames, dev_prob = torch.from_numpy(np.ascontiguousarray(frames)).to(self.device), torch.from_numpy(prob).to(self.device)
        if grid and Y is not None:
            truth = torch.from_numpy(np.ascontiguousarray(np.asarray(Y)[::skip], dtype=bool)).to(self.device)
            rows, best = [], None
            for point in points:
                dev_labels = dense_crf(dev_frames, dev_prob, point)
                inter, union = metrics.iou_counts(dev_labels, truth).tolist()
                rows.append({"params": dict(zip(GRID_KEYS, point)), "inter": inter, "union": union, "iou": metrics.ratio(inter, union)})
                if metrics.best_index([r["iou"] for r in rows]) == len(rows) - 1:
                    best = dev_labels                                  # the only labels kept on the device, and the only ones copied back
            b = metrics.best_index([r["iou"] for r in rows])
            self.crf_reports.append({"rows": rows, "best": {"index": b, "params": rows[b]["params"], "iou": rows[b]["iou"]}})
            labels = best.cpu().numpy()
        else:
            labels = dense_crf(dev_frames, dev_prob, points[0]).cpu().numpy()
        if self.rank == 0:
            self._crf_debug_pngs(imgs, prob, labels)
        mask[::skip, 0] = labels
        return mask >= 1

    def _crf_debug_pngs(self, imgs, prob, labels):
        plt = pyplot()
        if plt is None:
            return
        out = self.path + "crf/"
        os.makedirs(out, exist_ok=True)
        for i in range(0, len(labels), 50):
            plt.imsave(out + f"{i}_mask.png", prob[i])
            plt.imsave(out + f"{i}_img.png", imgs[i])
            plt.imsave(out + f"{i}_crf.png", labels[i])

    # ------------------------------------------------------------------ -eval: IoU on the labelled red-trees set
    @staticmethod
    def get_iou(A, B):
        """Intersection over union of two boolean stacks taken over the WHOLE set, 3 digits (main.py:1265-1270)."""
        A, B = np.asarray(A, dtype=bool), np.asarray(B, dtype=bool)
        both, either = np.count_nonzero(A & B), np.count_nonzero(A | B)
        return round(both / either, 3) if either else float("nan")

    def eval(self, folder="", vis=False):
        """main.py:891-1087: masks of `red-trees/X.npy[100:5000:2]` (batch 128, eval mode), thresholded
        at --eval-thresh, IoU against `all(Y.npy, axis=-1)`; with -salience also the saliency baseline of main.py:941-953,
        976-1003 (|d mean(pred)/dX| summed over channels, normalised, weighted by pred, thresholded) and its IoU; with -crf the IoU of
        the CRF-refined mask (and saliency map) as well.  Returns [iou, crfiou, saliou, salcrfiou] without the entries whose flag is
        off, in the reference's order (main.py:1005-1015).  With -test, or --output-video, rank 0 then writes the evaluation video of
        main.py:1027-1087 (video.py) when the IoU is above 0; its layout and ffmpeg are checked before the sweep."""
        args = self.args
        if args.noevalmode and args.salience:
            raise NotImplementedError("-noevalmode together with -salience (Dropout inside the saliency backward) is not implemented")
        if args.resimages or folder or vis:
            raise NotImplementedError("-resimages / folder evaluation are outside this build's scope")
        vid = (video.plan(bool(args.crf), bool(args.salience)), video.find_ffmpeg()) if video.wanted(args) else None
        pick = slice(100, 5000, 2)                                        # the reference's evaluation subset
        frames = np.load("red-trees/X.npy")[pick]                         # uint8 [n,64,64,3] (the reference divides by 255 here)
        truth = np.load("red-trees/Y.npy")[pick].all(axis=-1)             # [n,64,64] bool: all three label channels set
        want_sal = bool(args.salience)

        def to_device(chunk):
            t = torch.from_numpy(np.ascontiguousarray(chunk)).to(self.device)
            # uint8 frames go to the kernels as they are (/255 fused); the saliency backward needs the float batch (main.py:921,939)
            return (t.double() / 255.0).float() if (t.dtype != torch.uint8 or want_sal) else t

        preds, M, sal = self._sweep_masks(frames, to_device, "eval at", want_saliency=want_sal)
        hard_m = M[:, 0] > args.eval_thresh
        ious = [self.get_iou(hard_m, truth)]
        st = evaluate.Stacks(args, self.device, truth=truth, mask=M[:, 0])

        def report(fn, name=None, *more):         # a report's file (the sweeps share one, written below), then its summary line
            rep, line = fn(args, st, *more)
            if name:
                write_json(self.path + name, rep, self.rank)
            print(line)
            return rep
        sweep, n_reports = {}, len(self.crf_reports)
        if getattr(args, "thresh_grid", ""):    # (this build's flags) the sweeps of eval_sweep.json
            sweep["thresholds"] = report(evaluate.thresh_sweep)
        crf_m = maps = sal_hard = sal_crf = None
        if args.crf:                                                      # main.py:969-972
            crf_m = st.host["crf"] = self.crf(frames, M, truth)[:, 0]
            ious.append(self.get_iou(crf_m, truth))
        if want_sal:
            maps, sal_hard = self._saliency_post(sal, preds, args.salience_thresh, args.salglobal)
            st.host["saliency"] = sal_hard[:, 0]
            ious.append(self.get_iou(sal_hard[:, 0], truth))
            if getattr(args, "salience_grid", ""):
                st.host.update(sal=sal[:, 0], preds=preds)
                sweep["saliency"] = report(evaluate.saliency_sweep)
            if args.crf:                                                  # main.py:1000-1003
                sal_crf = st.host["saliency_crf"] = self.crf(frames, maps, truth)[:, 0]
                ious.append(self.get_iou(sal_crf, truth))
        if getattr(args, "crf_grid", "") and args.crf:
            sweep["crf"] = report(evaluate.crf_grid, None, self.crf_reports[n_reports:])
        if sweep:
            self.sweep = sweep
            write_json(self.path + "eval_sweep.json", sweep, self.rank)
        if getattr(args, "graph_cut", None):    # (this build's flag) the mask refined by a min cut on the GPU; it stands where the CRF mask stands
            st.host["frames"] = frames if frames.dtype == np.uint8 else (255 * frames).astype(np.uint8)
            self.cut = report(evaluate.cut_report, "eval_cut.json")
            st.host["cut"] = st.cut().mask.cpu().numpy()
        if getattr(args, "clean", None):        # (this build's flag) the masks cleaned on the GPU; the reports below then read those
            self.clean = report(evaluate.clean_report, "eval_clean.json")
        if getattr(args, "objects", False):     # (this build's flags) the masks as objects, matched to the truth's, followed through the frames
            if getattr(args, "object_value", False):    # the critic is asked about every object, on the frames as bytes
                st.host["frames"] = frames if frames.dtype == np.uint8 else (255 * frames).astype(np.uint8)
                st.infer = self._value_infer()
            self.objects = report(evaluate.objects_report, "eval_objects.json")
            if getattr(args, "match_iou", ""):
                self.matches = report(evaluate.match_report, "eval_match.json")
            if getattr(args, "track_iou", ""):
                if getattr(args, "track_motion", 0) or getattr(args, "track_reid", None):   # the frames as bytes, the conversion of Handler.crf
                    st.host["frames"] = frames if frames.dtype == np.uint8 else (255 * frames).astype(np.uint8)
                self.tracks = report(evaluate.tracks_report, "eval_tracks.json")
        if getattr(args, "boundary_tol", ""):   # (this build's flag) the outlines against the truth's outline
            self.boundary = report(evaluate.boundary_report, "eval_boundary.json")
        print("\nRESULTS", ious)
        if vid is not None and self.rank == 0 and ious[0] > self.ious[0]:          # main.py:1027
            layout, exe = vid
            sources = {"X": frames, "Y": truth, "M": M[:, 0], "hardM": hard_m, "crfM": crf_m, "salM": maps[:, 0],
                       "salhardM": sal_hard[:, 0], "salcrfM": sal_crf}
            path = video.output_path(args.output_video, ious[0])
            n = video.write_video(path, layout, {k: v for k, v in sources.items() if v is not None}, self.device, ffmpeg=exe)
            print(f"video: {path} ({n} frames of {layout.width}x{layout.height})")
        return ious

    # ------------------------------------------------------------------ -viscritic / -vismasker: the value-curve videos
    def visualize(self):
        """main.py:702-884: the critic's value (and with -vismasker the mask) of every frame of the test split, eval mode in batches of
        128 -- -noevalmode has no effect, the reference calls .eval() here itself -- then {path}{visname}.mp4, -pred-sorted.mp4 and,
        with --sortidx != 0, -GT-sorted.mp4 (vis.py; rank 0 writes).  ffmpeg is looked for before the sweep.  Returns the paths."""
        args = self.args
        vis.refuse_unbuilt(args)
        if not hasattr(self, "XX"):
            raise ValueError("-viscritic / -vismasker need the test split of load_data() (self.XX): run with -train")
        exe = video.find_ffmpeg()
        to_device = lambda chunk: torch.from_numpy(np.ascontiguousarray(chunk)).to(self.device)
        preds, M, _unused = self._sweep_masks(self.XX, to_device, "progress at", train_mode=False)
        print()
        values = np.stack((np.asarray(self.YY[args.rewidx], dtype=np.float64), preds.astype(np.float64)), axis=0)      # main.py:804
        if self.rank != 0:
            return []
        paths = vis.write_videos(self.path, args.visname, args.sortidx, self.XX, M if args.vismasker else None, values, self.device,
                                 ffmpeg=exe)
        p = vis.plan(bool(args.vismasker))
        print(f"videos: {', '.join(paths)} ({len(self.XX)} frames of {p.width}x{p.height})")
        return paths

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _plot(path, series):
        plt = pyplot()
        if plt is None:
            return
        plt.clf()
        for name, vals in series.items():
            vals = np.asarray(vals, dtype=np.float64)
            if len(vals) == 0:
                continue
            k = min(30, len(vals))
            avg = np.convolve(vals, np.ones(k) / k, mode="valid")
            plt.plot(avg, label=name)
        plt.legend()
        plt.savefig(path)

    @staticmethod
    def _hist(path, values):
        """plt.clf(); plt.hist(values); plt.savefig(path) of main.py:257-264."""
        plt = pyplot()
        if plt is None:
            return
        plt.clf()
        plt.hist(np.asarray(values))
        print("saving histogramm", path)
        plt.savefig(path)
