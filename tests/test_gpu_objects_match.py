"""Object matching on the GPU (cgs_objects_match, cgs_amd.objects.match, -eval -objects --match-iou) against the pixel loop and the
Fractions of tests/objects_match_ref.py.  Everything the kernel gives is integer: exact equality everywhere; only sum_iou and pq,
float64 sums formed by torch, are compared to a relative 1e-9."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_match_ref as ref  # noqa: E402
import objects_ref  # noqa: E402
from cgs_amd import _lib, cli, handler, objects  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MILLI = (500, 750, 950, 1000)
IOU = tuple(m / 1000 for m in MILLI)
PATTERNS = objects_ref.patterns()


def _gpu(pred, truth, milli=MILLI, K=64, **kw):
    """objects.match on a stack (arrays are uploaded as int32), back on the host as the checker's (counts [n, 2 + 2 T], best)."""
    up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    res = objects.match(up(pred), up(truth), iou=[m / 1000 for m in milli], max_objects=K, **kw)
    torch.cuda.synchronize()
    n, T = res.pred_max.shape[0], len(milli)
    assert res.pred_max.shape == res.truth_max.shape == (n,) and res.matched_pred.shape == res.matched_truth.shape == (n, T)
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in res if t is not None)
    counts = np.empty((n, 2 + 2 * T), dtype=np.int32)
    counts[:, 0], counts[:, 1] = res.pred_max.cpu().numpy(), res.truth_max.cpu().numpy()
    counts[:, 2::2], counts[:, 3::2] = res.matched_pred.cpu().numpy(), res.matched_truth.cpu().numpy()
    if res.best is None:
        return counts, None
    assert res.best.shape == (n, 2, K, 4)
    return counts, res.best.cpu().numpy()


def _check(pred, truth, milli=MILLI, K=64):
    """pred, truth: integer [n,h,w].  The kernel's answer must be the checker's; returns the checker's (counts, best, sum_iou)."""
    want = ref.match(pred, truth, milli, K)
    counts, best = _gpu(pred, truth, milli, K)
    np.testing.assert_array_equal(counts, want[0], err_msg=f"counts, K={K}")
    np.testing.assert_array_equal(best, want[1], err_msg=f"best, K={K}")
    return want


def _labels(on, conn):
    return objects_ref.label_frame(on, conn, 1)[0]


def _strips(count):
    """A hand-numbered map of exactly `count` objects: consecutive raster chunks of 4096 // count pixels, the rest to the last one."""
    return np.minimum(np.arange(4096) // (4096 // count) + 1, count).astype(np.int32).reshape(64, 64)


@functools.lru_cache(maxsize=None)
def _named():
    """name -> (pred, truth) int32 [64,64], the 64 x 64 frames of the tests below (shared, never written to)."""
    full, empty = np.ones((64, 64), dtype=np.int32), np.zeros((64, 64), dtype=np.int32)
    board = _labels(PATTERNS["checkerboard"], 4)
    out = {}
    for seed in range(3):
        p, t = ref.generator_frame(seed)
        out[f"gen{seed}"] = (_labels(p, 8), _labels(t, 8))
    out.update({"full-full": (full, full), "empty-full": (empty, full), "full-spiral": (full, _labels(PATTERNS["spiral"], 8)),
                "full-empty": (full, empty), "empty-empty": (empty, empty), "board-strips": (board, _strips(64)),
                "strips65-rolled64": (_strips(65), np.roll(_strips(64), 10)), "random": (_labels(PATTERNS["random0.45"], 8), _labels(PATTERNS["random0.593"], 4))})
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _named_ref(name, K=64):
    p, t = _named()[name]
    return ref.match_frame(p, t, MILLI, K)[:2]


# ---------------------------------------------------------------- 1. generator frames, labelled on the GPU
@pytest.mark.parametrize("conn", [4, 8])
def test_generator_frames(conn):
    frames = [ref.generator_frame(seed) for seed in range(6)]
    dev = [torch.from_numpy(np.stack([f[i] for f in frames])).to(DEV) for i in (0, 1)]
    pl, tl = (objects.label(d, connectivity=conn).labels for d in dev)
    for got, i in ((pl, 0), (tl, 1)):
        np.testing.assert_array_equal(got.cpu().numpy(), objects_ref.label(np.stack([f[i] for f in frames]), conn)[0])
    counts, best, sums = ref.match(pl.cpu().numpy(), tl.cpu().numpy(), MILLI)
    pred_max, truth_max, mp, mt = ref.split_counts(counts)
    # the frames show what they are for: about the checker's output, not the kernel's
    total = mp.sum(axis=0)
    assert total[0] > total[1] > total[2] >= total[3] > 0                  # matches are lost from 0.5 to 0.75 to 0.95; exact ones stay
    assert (pred_max.sum() - total[0] > 0) and (truth_max.sum() - mt.sum(axis=0)[0] > 0)            # fp > 0 and fn > 0
    np.testing.assert_array_equal(mp, mt)                                  # two maps of one connectivity: one-to-one
    got_counts, got_best = _gpu(pl, tl)
    np.testing.assert_array_equal(got_counts, counts)
    np.testing.assert_array_equal(got_best, best)
    np.testing.assert_allclose(objects.sum_iou(objects.match(pl, tl, iou=IOU).best, IOU).cpu().numpy(), sums, rtol=1e-9, atol=0)


# ---------------------------------------------------------------- 2. hand-made maps
def test_hand_made_maps():
    h, w = 4, 6
    z = lambda: np.zeros((h, w), dtype=np.int32)
    frames = {}
    p, t = z(), z()                      # IoU exactly 1/2: two predicted pixels, one of them truth
    p[1, 2:4], t[1, 2] = 1, 1
    frames["half"] = (p, t)
    p, t = z(), z()                      # IoU exactly 1
    p[2:4, 1:3], t[2:4, 1:3] = 1, 1
    frames["one"] = (p, t)
    p, t = z(), z()                      # one predicted object over two truth objects, IoU 1/2 with each
    p[0, 0:2], t[0, 0], t[0, 1] = 1, 1, 2
    frames["two-truths"] = (p, t)
    frames["two-preds"] = (t, p)         # and the other way round
    p, t = z(), z()                      # equal IoU 2/6 with truth 3 and truth 2 (in raster order 3 comes first), and a lone object 2
    p[0, 0:4], t[0, 0:2], t[0, 2:4] = 1, 3, 2
    t[1, 0:2], t[1, 2:4] = 3, 2
    p[3, 3:6] = 2
    frames["tie"] = (p, t)
    frames["zero-pred"], frames["zero-truth"], frames["zero-both"] = (z(), frames["tie"][1]), (frames["tie"][0], z()), (z(), z())
    p, t = frames["tie"][0].copy(), frames["tie"][1].copy()
    p[p == 0], t[t == 0] = -1, -7        # negative values are background
    p[2, 5] = np.iinfo(np.int32).min
    frames["negative"] = (p, t)
    milli = (500, 501, 1000)
    names = list(frames)
    counts, best, _ = _check(np.stack([frames[k][0] for k in names]), np.stack([frames[k][1] for k in names]), milli, K=4)
    got = {k: (counts[i].tolist(), best[i]) for i, k in enumerate(names)}
    # spelled out, so that the checker is not the only witness
    assert got["half"][0] == [1, 1, 1, 1, 0, 0, 0, 0] and got["half"][1][0, 0].tolist() == [1, 1, 2, 1]
    assert got["one"][0] == [1, 1, 1, 1, 1, 1, 1, 1] and got["one"][1][1, 0].tolist() == [1, 4, 4, 4]
    assert got["two-truths"][0] == [1, 2, 1, 2, 0, 0, 0, 0] and got["two-truths"][1][0, 0].tolist() == [1, 1, 2, 1]
    assert got["two-preds"][0] == [2, 1, 2, 1, 0, 0, 0, 0] and got["two-preds"][1][1, 0].tolist() == [1, 1, 2, 1]
    assert got["tie"][1][0, 0].tolist() == [2, 2, 4, 4] and got["tie"][1][0, 1].tolist() == [0, 0, 3, 0] and got["tie"][0] == [2, 3, 0, 0, 0, 0, 0, 0]
    assert got["tie"][1][1].tolist() == [[0, 0, 0, 0], [1, 2, 4, 4], [1, 2, 4, 4], [0, 0, 0, 0]]     # truth 1 is absent: area 0
    assert got["zero-pred"][0][:2] == [0, 3] and not got["zero-pred"][1][0].any() and got["zero-pred"][1][1, 1:3].tolist() == [[0, 0, 4, 0]] * 2
    assert got["zero-truth"][0][:2] == [2, 0] and got["zero-truth"][1][0, :2].tolist() == [[0, 0, 4, 0], [0, 0, 3, 0]] and not got["zero-truth"][1][1].any()
    assert not any(got["zero-both"][0]) and not got["zero-both"][1].any()
    assert got["negative"][0] == got["tie"][0] and np.array_equal(got["negative"][1], got["tie"][1])


# ---------------------------------------------------------------- 3. shapes and row ends
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (37, 64), (64, 33)])
def test_shapes_and_row_ends(h, w):
    rs = np.random.RandomState(100 * h + w)
    ends = np.zeros((h, w), dtype=np.int32)          # (y, w-1) and (y+1, 0) carry the pair (1, 1) and nothing else in those rows does:
    for y in range(0, h - 1, 3):                     # neighbours in memory, not in the image
        ends[y, w - 1] = ends[y + 1, 0] = 1
    diag = np.zeros((h, w), dtype=np.int32)          # the same in every row
    diag[0::2, w - 1], diag[1::2, 0] = 2, 2
    runs = np.repeat(rs.randint(-1, 6, (h, (w + 3) // 4)), 4, axis=1)[:, :w]           # runs of four equal labels
    pred = np.stack([ends, diag, np.ones((h, w)), rs.randint(-1, 5, (h, w)), runs, rs.randint(0, 70, (h, w)), np.zeros((h, w))]).astype(np.int32)
    truth = np.stack([ends, diag, np.ones((h, w)), rs.randint(-1, 4, (h, w)), np.roll(runs, 1, axis=1), rs.randint(0, 3, (h, w)), np.ones((h, w))]).astype(np.int32)
    counts, best, _ = _check(pred, truth)
    _check(pred, truth, K=3)
    if h > 1 and w > 2:
        n_ends = int(ends.sum())                     # every pixel a run of its own: areas and intersection count each once
        assert n_ends >= 2 and best[0, 0, 0].tolist() == [1, n_ends, n_ends, n_ends] and best[0, 1, 0].tolist() == [1, n_ends, n_ends, n_ends]
    assert best[2, 0, 0].tolist() == [1, h * w, h * w, h * w]


# ---------------------------------------------------------------- 4. the cap
@pytest.mark.parametrize("K", [1, 7, 64])
def test_cap(K):
    board = _named()["board-strips"][0]
    assert board.max() == 2048 and _strips(64).max() == 64 and _strips(65).max() == 65 and len(np.unique(_strips(65))) == 65
    s64, s65, r64, r65 = _strips(64), _strips(65), np.roll(_strips(64), 10), np.roll(_strips(65), 10)
    pred = np.stack([s64, s65, s64, s65, board, s64, board])
    truth = np.stack([r64, r64, r65, r65, s64, board, board])
    counts, best, _ = _check(pred, truth, K=K)
    assert counts[:, 0].tolist() == [64, 65, 64, 65, 2048, 64, 2048] and counts[:, 1].tolist() == [64, 64, 65, 65, 64, 2048, 2048]
    assert (counts[:, 2:] <= K).all() and (best[:, :, :, 0] <= K).all()            # objects above the cap add nothing and match nothing
    assert counts[0, 2] == K and counts[0, 2 + 2] == 0 and counts[6, 2 + 6] == K      # strips: IoU 54 / 74 each; board on board: 1 each
    assert best[0, 0, K - 1].tolist() == [K, 54, 64, 64] and best[0, 1, K - 1].tolist() == [K, 54, 64, 64]
    # a smaller cap leaves the areas of the objects below it alone
    np.testing.assert_array_equal(best[1, 0, :, 2], ref.match_frame(s65, r64, MILLI, 64)[1][0, :K, 2])
    # rows beyond the largest label are zero, and a stale buffer is overwritten whole: the entry point on buffers full of junk
    few = np.stack([np.minimum(s64, 3) * (s64 <= 3), np.zeros((64, 64), dtype=np.int32)]).astype(np.int32)
    dp, dt = torch.from_numpy(few).to(DEV), torch.from_numpy(np.stack([r64, s64])).to(DEV)
    thr = torch.tensor(MILLI, dtype=torch.int32).to(DEV)
    out_counts = torch.full((2, 2 + 2 * len(MILLI)), 123456789, dtype=torch.int32, device=DEV)
    out_best = torch.full((2, 2, K, 4), 123456789, dtype=torch.int32, device=DEV)
    _lib.call("cgs_objects_match", dp.data_ptr(), dt.data_ptr(), 2, 64, 64, K, thr.data_ptr(), len(MILLI), out_counts.data_ptr(),
              out_best.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = ref.match(few, np.stack([r64, s64]), MILLI, K)
    np.testing.assert_array_equal(out_counts.cpu().numpy(), want[0])
    np.testing.assert_array_equal(out_best.cpu().numpy(), want[1])
    assert not want[1][0, 0, 3:].any() and not want[1][1, 0].any() and want[1][1, 1, :K, 2].tolist() == [64] * K


# ---------------------------------------------------------------- 5. contention shapes
def test_contention_shapes():
    names = ["full-full", "full-spiral", "full-empty"]
    counts, best, _ = _check(np.stack([_named()[k][0] for k in names]), np.stack([_named()[k][1] for k in names]))
    assert counts[0].tolist() == [1, 1] + [1, 1] * 4 and best[0, :, 0].tolist() == [[1, 4096, 4096, 4096]] * 2
    assert counts[1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0] and best[1, :, 0].tolist() == [[1, 2111, 4096, 2111], [1, 2111, 2111, 4096]]
    assert counts[2].tolist() == [1, 0] + [0, 0] * 4 and best[2, 0, 0].tolist() == [0, 0, 4096, 0] and not best[2, 1].any()


# ---------------------------------------------------------------- 6. several frames in one launch
@pytest.mark.parametrize("n", [1, 37])
def test_frames_of_one_launch_do_not_leak(n):
    names = list(_named())
    assert names.index("empty-full") == names.index("full-full") + 1 and names.index("empty-empty") == names.index("full-empty") + 1
    order = [names[(k + 3) % len(names)] for k in range(n)]                # starts at full-full
    counts, best = _gpu(np.stack([_named()[k][0] for k in order]), np.stack([_named()[k][1] for k in order]))
    np.testing.assert_array_equal(counts, np.stack([_named_ref(k)[0] for k in order]))
    np.testing.assert_array_equal(best, np.stack([_named_ref(k)[1] for k in order]))


# ---------------------------------------------------------------- 7. optional output, consistency, views
def test_optional_output_and_consistency():
    names = ["gen0", "random", "strips65-rolled64", "board-strips", "full-spiral", "gen2"]
    pred, truth = np.stack([_named()[k][0] for k in names]), np.stack([_named()[k][1] for k in names])
    milli = tuple(range(500, 1001, 50)) + (501, 999)
    for K in (7, 64):
        counts, best = _gpu(pred, truth, milli, K)
        bare, none = _gpu(pred, truth, milli, K, want_best=False)
        assert none is None
        np.testing.assert_array_equal(bare, counts)
        # the counts are the rows of `best` that reach each threshold, recomputed here in Python integers
        for side in (0, 1):
            for k, m in enumerate(milli):
                reach = [[int(r[1]) > 0 and 1000 * int(r[1]) >= m * int(r[2] + r[3] - r[1]) for r in frame[side]] for frame in best]
                assert counts[:, 2 + 2 * k + side].tolist() == [sum(f) for f in reach], (K, side, m)
    assert counts[:, 2].sum() > counts[:, 2 + 2 * 10].sum() > 0            # 0.5 against 1.0: the thresholds are not all alike here
    # one frame as [h,w]
    one, one_best = _gpu(pred[0], truth[0], milli)
    np.testing.assert_array_equal(one, _gpu(pred[:1], truth[:1], milli)[0])
    # views: every second column of a wider stack, and a transposed frame
    rs = np.random.RandomState(7)
    wide_p, wide_t = (torch.from_numpy(rs.randint(-1, 9, (3, 64, 128)).astype(np.int32)).to(DEV) for _ in range(2))
    vp, vt = wide_p[:, :, ::2], wide_t[:, :, 1::2]
    assert not vp.is_contiguous() and not vt.is_contiguous()
    a, b = _gpu(vp, vt), _gpu(vp.contiguous(), vt.contiguous())
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0], ref.match(vp.cpu().numpy(), vt.cpu().numpy(), MILLI)[0])
    tp, tt = wide_p[0, :, :40].t(), wide_t[0, :, :40].t()                  # [40,64]
    assert not tp.is_contiguous()
    np.testing.assert_array_equal(_gpu(tp, tt)[1], ref.match(tp.cpu().numpy()[None], tt.cpu().numpy()[None], MILLI)[1])


# ---------------------------------------------------------------- 8. Handler and CLI
def _run(argv, capsys):
    capsys.readouterr()
    H = cli.main(argv + ["--model", "m"])
    return H, capsys.readouterr().out


def _results(out):
    return out.split("RESULTS [")[-1].split("]")[0]


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The synthetic red-trees/ and G1 checkpoints of test_gpu_objects.py's fixture, 420 frames (160 evaluated), rebuilt here; the
    test paints its own truth into Y.npy once it has seen the masks."""
    root = str(tmp_path)
    for name, state in zip([str(s) for s in golden("g6_process.npz")["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    Xe = np.stack([_structured(64, 64, 200 + k % 40)[0] for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    monkeypatch.chdir(root)
    return root, Xe[slice(100, 5000, 2)]


def _block(on, truth_labels, conn, min_area, milli):
    """What one block of eval_match.json must hold for the on-mask `on`: objects_ref's labels, the checker's match, match_report."""
    counts, _, sums = ref.match(objects_ref.label(on, conn, min_area, 64)[0], truth_labels, milli)
    return objects.match_report(*ref.split_counts(counts), sums, [m / 1000 for m in milli])


def _same_block(got, want):
    assert {k: v for k, v in got.items() if k != "per_iou"} == {k: v for k, v in want.items() if k != "per_iou"}
    assert len(got["per_iou"]) == len(want["per_iou"])
    for g, w in zip(got["per_iou"], want["per_iou"]):
        assert set(g) == set(w)
        for key in w:
            if key in ("sum_iou", "pq") and w[key] is not None:            # float64 sums in two orders: 2450 x 64 terms at most
                assert g[key] == pytest.approx(w[key], rel=1e-9, abs=0), key
            elif key in ("precision", "recall", "f1") and w[key] is not None:
                assert g[key] == w[key], key                               # the same integers through the same expression
            else:
                assert g[key] == w[key] and type(g[key]) is type(w[key]), key


def test_cli_eval_match(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))                                        # a float32 value: half of the pixels are above it
    # a rectangle can match none of these masks' ragged objects at IoU 1/2, so the truth painted into Y.npy is the masks cut a
    # little higher: objects that shrink, split or vanish against the predicted ones
    truth = M[:, 0] > np.float32(np.percentile(M, 55))
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    on = objects_ref.on_pixels(M[:, 0], thr)
    milli = list(range(500, 951, 50))
    truth_labels = objects_ref.label(truth, 8, 1, 64)[0]
    want = _block(on, truth_labels, 8, 4, milli)
    first, last = want["per_iou"][0], want["per_iou"][-1]
    assert first["matched_pred"] > last["matched_pred"] > 0 and first["fp"] > 0 and first["fn"] > 0      # matches, and unmatched on each side
    match_file, objects_file = os.path.join(root, "m", "eval_match.json"), os.path.join(root, "m", "eval_objects.json")
    head = {"connectivity": 8, "min_area": 4, "threshold": thr, "max_objects": 64, "iou": [m / 1000 for m in milli]}

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4"]
    H0, base = _run(common, capsys)
    assert not os.path.exists(match_file) and "MATCH" not in base and H0.matches is None
    objects_json = _read(objects_file)
    H1, out = _run(common + ["--match-iou", "0.5:0.95:10"], capsys)
    assert out.count("\nMATCH conn=8 min_area=4 iou>=0.5 (10 thresholds): matched ") == 1 and out.index("OBJECTS") < out.index("MATCH") < out.index("RESULTS")
    assert f"matched {first['matched_pred']}/{want['pred_objects']} predicted, {first['matched_truth']}/{want['truth_objects']} truth objects" in out
    line = lambda text, word: [ln for ln in text.split("\n") if ln.startswith(word)]
    assert _results(out) == _results(base) and line(out, "OBJECTS") == line(base, "OBJECTS") and len(line(base, "OBJECTS")) == 1
    assert _read(objects_file) == objects_json and H1.objects == H0.objects
    with open(match_file) as fp:
        report = json.load(fp)
    assert report == H1.matches and set(report) == set(head) | {"mask"}
    assert {k: report[k] for k in head} == head
    _same_block(report["mask"], want)

    H2, out = _run(["-crf"] + common + ["--match-iou", "0.5:0.95:10"], capsys)
    assert out.count("\nMATCH ") == 1 and "; crf matched " in out and out.index("MATCH") < out.index("RESULTS")
    with open(match_file) as fp:
        report = json.load(fp)
    assert report == H2.matches and set(report) == set(head) | {"mask", "crf"} and {k: report[k] for k in head} == head
    _same_block(report["mask"], want)
    crf_on = H.crf(frames, M, truth)[:, 0]
    _same_block(report["crf"], _block(crf_on, truth_labels, 8, 4, milli))
