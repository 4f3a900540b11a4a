"""Object tracking on the GPU (cgs_objects_track, cgs_objects_track_switches, cgs_amd.objects.track / switches, -objects --track-iou)
against the np.bincount tables, Fractions and frame-by-frame walk of tests/objects_track_ref.py.  Everything the kernels give is
integer: exact equality everywhere."""
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

import objects_ref  # noqa: E402
import objects_track_ref as ref  # noqa: E402
from cgs_amd import _lib, cli, handler, objects  # noqa: E402
from test_gpu_metrics import _structured  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _gpu(labels, milli, K=64, max_tracks=None, paint=True):
    """objects.track on a stack (arrays are uploaded as int32), back on the host in the checker's form."""
    res = objects.track(_up(labels), iou=milli / 1000, max_objects=K, max_tracks=max_tracks, want_labels=paint, want_rgb=paint)
    torch.cuda.synchronize()
    n = res.prev.shape[0]
    assert res.prev.shape == res.track.shape == (n, K) and res.table.shape == (n * K if max_tracks is None else max_tracks, 8)
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in res[:7])
    out = {"prev": res.prev.cpu().numpy(), "track": res.track.cpu().numpy(), "table": res.table.cpu().numpy(),
           "totals": np.array([int(res.n_tracks), int(res.n_links), int(res.n_objects), int(res.longest)], dtype=np.int32)}
    if paint:
        assert res.rgb.dtype == torch.uint8 and res.rgb.shape == res.track_labels.shape + (3,)
        out["track_labels"], out["rgb"] = res.track_labels.cpu().numpy(), res.rgb.cpu().numpy()
    else:
        assert res.track_labels is None and res.rgb is None
    return out


def _same(got, want, what=""):
    for key in ("prev", "track", "totals", "table"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")
    if "track_labels" in got and "track_labels" in want:
        np.testing.assert_array_equal(got["track_labels"], want["track_labels"], err_msg=f"track_labels {what}")
        np.testing.assert_array_equal(got["rgb"], ref.colours(want["track_labels"]), err_msg=f"rgb {what}")


def _check(labels, milli, K=64, max_tracks=None):
    """The kernels' answer must be the checker's; returns the checker's."""
    labels = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[None]
    want = ref.track(labels, milli, K, max_tracks, want_paint=True)
    _same(_gpu(labels, milli, K, max_tracks), want, f"milli={milli} K={K}")
    return want


# ---------------------------------------------------------------- 1. chain lengths around the round counts of the pointer doubling
def _chains(n):
    """4 x 4 frames: object 1 (row 0) in every frame; object 2 (row 1) jumps between two places that do not overlap at every fifth
    frame, which breaks its chain before and after; object 3 (row 3) exists in three frames of every six."""
    s = np.zeros((n, 4, 4), dtype=np.int32)
    s[:, 0] = 1
    for f in range(n):
        if f % 5 == 4:
            s[f, 1, 2:] = 2
        else:
            s[f, 1, :2] = 2
        if (f // 3) % 2 == 0:
            s[f, 3, 1:] = 3
    return s


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 65, 66, 129, 130, 257, 258, 1025, 1026])
def test_chain_lengths_around_the_round_counts(n):
    want = _check(_chains(n), 500, K=3)
    assert want["totals"][3] == n and want["table"][0].tolist() == [0, 1, n, 4 * n, 4, 4, 4 * (n - 1), 4 * (n - 1)]
    assert (want["track"][:, 0] == 1).all() and want["totals"][2] == n + n + sum((f // 3) % 2 == 0 for f in range(n))
    if n >= 10:
        lengths = want["table"][:want["totals"][0], 2].tolist()
        assert 1 in lengths and 4 in lengths and 3 in lengths               # object 2's singletons and runs of four, object 3's runs
    # the numbering order: heads by frame, then by label
    heads = [tuple(r[:2]) for r in want["table"][:want["totals"][0]].tolist()]
    assert heads == sorted(heads) == want["heads"]
    _check(_chains(n), 500, K=2)                                            # object 3 above the cap


# ---------------------------------------------------------------- 2. hand-made 64 x 64 cases
def test_moving_square():
    n = 12
    s = np.zeros((n, 64, 64), dtype=np.int32)
    for f in range(n):
        s[f, 10:26, 5 + f:21 + f] = 1                                       # IoU 15 / 17 with the frame before
    low, high = _check(s, 300), _check(s, 950)
    assert low["totals"].tolist() == [1, n - 1, n, n] and low["table"][0].tolist() == [0, 1, n, 256 * n, 256, 256, 240 * (n - 1), 272 * (n - 1)]
    assert high["totals"].tolist() == [n, 0, n, 1] and high["track"][:, 0].tolist() == list(range(1, n + 1))
    assert _check(s, 882)["totals"][0] == 1 and _check(s, 883)["totals"][0] == n           # 15 / 17 = 0.88235...


def test_split_merge_tie_permutation_and_empty_frames():
    z = lambda n: np.zeros((n, 64, 64), dtype=np.int32)
    s = z(3)                                                                # a bar splits into a long and a short part and merges again
    s[0, 20:24, 4:60] = 1
    s[1, 20:24, 4:40], s[1, 20:24, 44:60] = 2, 1
    s[2, 20:24, 4:60] = 1
    want = _check(s, 300)
    assert want["prev"][:, :2].tolist() == [[0, 0], [0, 1], [2, 0]] and want["track"][:, :2].tolist() == [[1, 0], [2, 1], [1, 0]]
    assert want["totals"].tolist() == [2, 2, 4, 3] and want["table"][1].tolist() == [1, 1, 1, 64, 64, 64, 0, 0]
    s = z(2)                                                                # an exact tie: 128 / 256 with both halves
    s[0, 8:16, 0:16], s[0, 8:16, 16:32] = 1, 2
    s[1, 8:16, 0:32] = 1
    assert _check(s, 500)["prev"][1, 0] == 1 and _check(s, 501)["totals"].tolist() == [3, 0, 3, 1]
    assert _check(s[::-1].copy(), 500)["prev"][1, :2].tolist() == [1, 0]
    rs = np.random.RandomState(5)                                           # six stripes whose numbers are permuted in every frame
    base = np.repeat(np.arange(1, 7), 10)[:, None] * np.ones((1, 64), dtype=np.int64)
    s = z(7)
    for f in range(7):
        perm = np.concatenate([[0], rs.permutation(6) + 1])
        s[f, 2:62] = perm[base]
    want = _check(s, 1000)
    assert want["totals"].tolist() == [6, 36, 42, 7] and sorted(want["track"][6, :6].tolist()) == [1, 2, 3, 4, 5, 6]
    s = z(5)                                                                # an empty frame in the middle
    s[:, 30:40, 30:40] = 1
    s[2] = 0
    assert _check(s, 500)["totals"].tolist() == [2, 2, 4, 2]
    want = _check(z(4), 500)                                                # an all-empty stack
    assert not want["totals"].any() and not want["table"].any() and not want["track"].any()


# ---------------------------------------------------------------- 3. the cap
def _strips(count):
    return np.minimum(np.arange(4096) // (4096 // count) + 1, count).astype(np.int32).reshape(64, 64)


def test_cap():
    s = np.stack([_strips(65)] * 3)
    want = _check(s, 500)
    assert want["totals"].tolist() == [64, 128, 192, 3] and not want["track_labels"][s == 65].any() and want["track_labels"][s <= 64].all()
    for K in (1, 3):
        want = _check(s, 500, K=K)
        assert want["totals"].tolist() == [K, 2 * K, 3 * K, 3] and np.count_nonzero(want["track_labels"]) == 3 * 63 * K
    moving = np.stack([np.roll(_strips(64), 40 * f) for f in range(4)])     # at most 40 / 88 with any strip before: every object a track
    cut = _check(moving, 500, max_tracks=10)
    assert cut["totals"][0] == 256 and cut["track"].max() == 256 and cut["table"].shape == (10, 8) and cut["table"][:, 2].tolist() == [1] * 10
    few = _check(np.stack([_strips(3)] * 2), 500, max_tracks=7)             # and rows beyond N are zero in a table of junk
    assert few["table"][:3, 2].tolist() == [2, 2, 2] and not few["table"][3:].any()


# ---------------------------------------------------------------- 4. shapes, views, optional outputs
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (64, 1), (1, 64), (64, 64)])
def test_shapes(h, w):
    rs = np.random.RandomState(100 * h + w)
    blocks = np.repeat(np.repeat(rs.randint(-1, 6, (9, (h + 3) // 4, (w + 3) // 4)), 4, axis=1), 4, axis=2)[:, :h, :w]
    blocks[5:] = np.where(rs.rand(4, h, w) < 0.1, 70, blocks[4])            # four frames alike but for specks of a label above the cap
    _check(blocks, 300)
    _check(blocks, 300, K=3)
    _check(rs.randint(0, 3, (6, h, w)), 1)
    one = _check(np.ones((5, h, w)), 1000)
    assert one["totals"].tolist() == [1, 4, 5, 5] and one["table"][0, 3:].tolist() == [5 * h * w, h * w, h * w, 4 * h * w, 4 * h * w]


def test_views_and_optional_outputs():
    rs = np.random.RandomState(3)
    frame = rs.randint(0, 5, (40, 64)).astype(np.int32)
    got = _gpu(frame, 500)                                                  # [h,w]: one frame
    _same(got, ref.track(frame[None], 500, want_paint=True))
    assert got["prev"].shape == (1, 64) and got["track_labels"].shape == (1, 40, 64)
    wide = torch.from_numpy(np.repeat(rs.randint(-1, 9, (6, 64, 32)), 4, axis=2).astype(np.int32)).to(DEV)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    _same(_gpu(view, 400), ref.track(view.cpu().numpy(), 400, want_paint=True))
    t = wide[0, :, :40].t()
    assert not t.is_contiguous()
    _same(_gpu(t, 400), ref.track(t.cpu().numpy()[None], 400, want_paint=True))
    with_paint, bare = _gpu(view, 400), _gpu(view, 400, paint=False)
    _same(bare, with_paint)
    only_labels = objects.track(view, iou=0.4, want_labels=True)
    assert only_labels.rgb is None
    np.testing.assert_array_equal(only_labels.track_labels.cpu().numpy(), with_paint["track_labels"])
    only_rgb = objects.track(view, iou=0.4, want_rgb=True)
    assert only_rgb.track_labels is None
    np.testing.assert_array_equal(only_rgb.rgb.cpu().numpy(), with_paint["rgb"])


# ---------------------------------------------------------------- 5. generator stacks, labelled on the GPU
@functools.lru_cache(maxsize=None)
def _generator_masks():
    """64 masks of test_gpu_metrics._structured (a noisy central disc with speckle), frame f rolled by f pixels."""
    p = np.stack([np.roll(_structured(64, 64, 300 + f)[1], f, axis=1) for f in range(64)])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _generator_labels(conn, thresh=0.5):
    got = objects.label(torch.from_numpy(_generator_masks().copy()).to(DEV), thresh=thresh, connectivity=conn).labels
    np.testing.assert_array_equal(got.cpu().numpy(), objects_ref.label(_generator_masks() > np.float32(thresh), conn)[0])
    return got


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("milli", [100, 300, 500, 900])
def test_generator_stacks(conn, milli):
    labels = _generator_labels(conn)
    want = _check(labels, milli)
    # the stack shows what it is for: about the checker's output, not the kernels'
    lengths = want["table"][:want["totals"][0], 2]
    assert lengths.max() >= 3 and (lengths == 1).any() and np.bincount([f for f, _ in want["heads"]]).max() >= 2
    assert labels.max() > 64 and want["totals"][1] > 0


# ---------------------------------------------------------------- 6. the colours
def test_rgb_is_the_formula_and_never_black():
    got = _gpu(np.stack([np.roll(_strips(64), 40 * f) for f in range(5)]), 500)
    assert got["totals"][0] == 64 * 5 and got["track_labels"].max() == 320
    want = np.zeros(got["track_labels"].shape + (3,), dtype=np.uint8)
    for t in range(1, 321):                                                 # the header's formula in Python integers
        hsh = (t * 2654435761) & 0xFFFFFFFF
        want[got["track_labels"] == t] = [64 + ((hsh >> (8 * c)) & 255) * 191 // 255 for c in range(3)]
    np.testing.assert_array_equal(got["rgb"], want)
    assert (got["rgb"].min(axis=-1) >= 64).all()
    part = _gpu(_chains(7), 500, K=2)                                       # background and an untracked object are black
    assert (part["rgb"][part["track_labels"] == 0] == 0).all() and (part["rgb"][part["track_labels"] > 0] >= 64).all()
    assert not part["track_labels"][_chains(7) == 3].any()


# ---------------------------------------------------------------- 7. switches
def _switches(pred, truth, track_milli, match_milli, K=64):
    pred, truth, iou = _up(pred), _up(truth), [m / 1000 for m in match_milli]
    pt, tt = (objects.track(s, iou=track_milli / 1000, max_objects=K) for s in (pred, truth))
    best = objects.match(pred, truth, iou=iou, max_objects=K).best
    got = objects.switches(tt.prev, pt.track, best, iou)
    assert got.dtype == torch.int32 and got.shape == (len(match_milli), 3) and got.device.type == "cuda"
    return got.cpu().numpy()


def test_switches_by_hand():
    row = lambda *v: np.array(v, dtype=np.int32)
    truth, pred = np.zeros((4, 3, 8), dtype=np.int32), np.zeros((4, 3, 8), dtype=np.int32)
    truth[:, 1] = [row(1, 1, 1, 1, 0, 0, 0, 0), row(0, 1, 1, 1, 1, 0, 0, 0), row(0, 0, 1, 1, 1, 1, 0, 0), row(0, 0, 0, 1, 1, 1, 1, 0)]
    pred[:, 1] = [row(1, 1, 1, 0, 0, 0, 0, 0), row(0, 1, 1, 0, 0, 0, 0, 0), row(0, 0, 0, 0, 1, 1, 0, 0), row(0, 0, 0, 0, 1, 1, 1, 0)]
    assert ref.switches(pred, truth, 300, [500, 750], K=4).tolist() == [[4, 3, 1], [2, 0, 0]]
    assert _switches(pred, truth, 300, [500, 750], K=4).tolist() == [[4, 3, 1], [2, 0, 0]]
    assert _switches(truth, truth, 300, [500, 1000], K=4).tolist() == [[4, 3, 0], [4, 3, 0]]


@pytest.mark.parametrize("match_milli", [(500,), tuple(range(500, 951, 30))])
def test_switches_on_generator_stacks(match_milli):
    assert len(match_milli) in (1, 16)
    pred, truth = _generator_labels(8, 0.6), _generator_labels(8)
    want = ref.switches(pred.cpu().numpy(), truth.cpu().numpy(), 300, match_milli)
    assert want[0, 0] > want[0, 1] > want[0, 2] > 0                        # covered, continued and switched links all occur
    np.testing.assert_array_equal(_switches(pred, truth, 300, match_milli), want)


# ---------------------------------------------------------------- 8. one scratch buffer, two stacks, one stream
def test_scratch_is_reused_without_leaking_state():
    a = _up(_generator_labels(4)[:40])
    b = _up(np.stack([np.roll(_strips(64), 40 * f) for f in range(9)]))
    K = 64
    need = max(int(_lib.load().cgs_objects_track_scratch_bytes(int(s.shape[0]), K)) for s in (a, b))
    scratch = torch.full((need // 8 + 1,), -1, dtype=torch.int64, device=DEV)          # junk to start with
    outs = []
    for s in (a, b, a):
        n = int(s.shape[0])
        prev, trk = (torch.full((n, K), 77, dtype=torch.int32, device=DEV) for _ in range(2))
        totals, table = torch.full((4,), 77, dtype=torch.int32, device=DEV), torch.full((n * K, 8), 77, dtype=torch.int32, device=DEV)
        _lib.call("cgs_objects_track", s.data_ptr(), n, 64, 64, K, 300, n * K, prev.data_ptr(), trk.data_ptr(), totals.data_ptr(),
                  table.data_ptr(), None, None, scratch.data_ptr(), scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
        outs.append({"prev": prev, "track": trk, "totals": totals, "table": table})
    torch.cuda.synchronize()
    for s, out in zip((a, b, a), outs):
        _same({k: v.cpu().numpy() for k, v in out.items()}, ref.track(s.cpu().numpy(), 300))


# ---------------------------------------------------------------- 9. Handler and CLI
def _run(argv, capsys):
    capsys.readouterr()
    H = cli.main(argv + ["--model", "m"])
    return H, capsys.readouterr().out


def _results(out):
    return out.split("RESULTS [")[-1].split("]")[0]


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


def _files(folder):
    return {f: _read(os.path.join(folder, f)) for f in sorted(os.listdir(folder))}


@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The synthetic red-trees/ and G1 checkpoints of test_gpu_objects_match.py's fixture, 420 frames (160 evaluated), rebuilt here with
    every frame rolled by half its index: one pixel per evaluated frame, so that the masks persist from frame to frame.  The test
    paints its own truth into Y.npy once it has seen the masks."""
    root = str(tmp_path)
    for name, state in zip([str(s) for s in golden("g6_process.npz")["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "red-trees"))
    Xe = np.stack([np.roll(_structured(64, 64, 200 + k // 80)[0], k // 2, axis=1) for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    monkeypatch.chdir(root)
    return root, Xe[slice(100, 5000, 2)]


def _side(labels, kept, milli):
    """What one side of eval_tracks.json must hold: the checker's tracks through track_report."""
    t = ref.track(labels, milli, 64)
    return t, objects.track_report(t["totals"], t["table"][:, 2], int(t["table"][:, 6].astype(np.int64).sum()), int(t["table"][:, 7].astype(np.int64).sum()),
                                   int(np.maximum(kept - 64, 0).sum()))


def _switch_rows(pred_labels, truth_labels, track_milli, match_milli):
    return [{"iou": m / 1000, "covered": int(c[0]), "continued": int(c[1]), "switches": int(c[2]), "switch_rate": int(c[2]) / int(c[1]) if c[1] else None}
            for m, c in zip(match_milli, ref.switches(pred_labels, truth_labels, track_milli, match_milli))]


def test_cli_eval_tracks(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))
    truth = M[:, 0] > np.float32(np.percentile(M, 55))                     # the masks cut a little higher, as test_gpu_objects_match.py paints it
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    on = objects_ref.on_pixels(M[:, 0], thr)
    pred_labels, _, pred_kept, _, _ = objects_ref.label(on, 8, 4, 64)
    truth_labels, _, truth_kept, _, _ = objects_ref.label(truth, 8, 1, 64)
    (pt, pred_side), (tt, truth_side) = _side(pred_labels, pred_kept, 300), _side(truth_labels, truth_kept, 300)
    assert pred_side["links"] > 0 and pred_side["max_length"] >= 3 and truth_side["links"] > 0          # the masks do persist
    tracks_file, objects_file, match_file = (os.path.join(root, "m", f"eval_{k}.json") for k in ("tracks", "objects", "match"))
    head = {"connectivity": 8, "min_area": 4, "threshold": thr, "max_objects": 64, "track_iou": 0.3}
    line = lambda text, word: [ln for ln in text.split("\n") if ln.startswith(word)]

    common = ["-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4"]
    H0, base = _run(common, capsys)
    assert not os.path.exists(tracks_file) and "TRACKS" not in base and H0.tracks is None
    objects_json = _read(objects_file)
    H1, out = _run(common + ["--track-iou", "0.3"], capsys)
    assert _results(out) == _results(base) and line(out, "OBJECTS") == line(base, "OBJECTS") and len(line(base, "OBJECTS")) == 1
    assert _read(objects_file) == objects_json and H1.objects == H0.objects and not os.path.exists(match_file) and "MATCH" not in out
    assert line(out, "TRACKS") == [f"TRACKS conn=8 min_area=4 iou>=0.3: {pred_side['tracks']} tracks over {pred_side['objects']} objects, mean length "
                                   f"{pred_side['mean_length']:.6f}, longest {pred_side['max_length']}; truth {truth_side['tracks']} tracks over "
                                   f"{truth_side['objects']} objects"]
    assert out.index("OBJECTS") < out.index("TRACKS") < out.index("RESULTS")
    with open(tracks_file) as fp:
        report = json.load(fp)
    assert report == H1.tracks == {**head, "truth": truth_side, "mask": {"pred": pred_side}}

    milli = list(range(500, 951, 50))
    H2, base = _run(common + ["--match-iou", "0.5:0.95:10"], capsys)
    match_json = _read(match_file)
    H3, out = _run(common + ["--match-iou", "0.5:0.95:10", "--track-iou", "0.3"], capsys)
    assert _read(match_file) == match_json and _read(objects_file) == objects_json and line(out, "MATCH") == line(base, "MATCH")
    assert out.index("MATCH") < out.index("TRACKS") < out.index("RESULTS") and _results(out) == _results(base)
    with open(tracks_file) as fp:
        report = json.load(fp)
    rows = _switch_rows(pred_labels, truth_labels, 300, milli)
    assert rows[0]["covered"] > 0 and rows[0]["continued"] > 0
    assert report == H3.tracks == {**head, "truth": truth_side, "mask": {"pred": pred_side, "switches": rows}}

    H4, out = _run(["-crf"] + common + ["--match-iou", "0.5:0.95:10", "--track-iou", "0.3"], capsys)
    with open(tracks_file) as fp:
        report = json.load(fp)
    crf_on = H.crf(frames, M, truth)[:, 0]
    crf_labels, _, crf_kept, _, _ = objects_ref.label(crf_on, 8, 4, 64)
    assert report == H4.tracks and set(report) == set(head) | {"truth", "mask", "crf"} and report["mask"] == {"pred": pred_side, "switches": rows}
    assert report["crf"] == {"pred": _side(crf_labels, crf_kept, 300)[1], "switches": _switch_rows(crf_labels, truth_labels, 300, milli)}
    assert len(line(out, "TRACKS")) == 1


def test_cli_process_tracks(workdir, capsys):
    from PIL import Image
    root, frames = workdir
    os.makedirs("S")
    numbers = [1, 2, 3, 10, 11, 12, 20, 21, 100, 101]                      # plain string order would put f10 before f2
    stems = [f"f{k}" for k in numbers]
    for stem, frame in zip(stems, frames[:len(stems)]):
        Image.fromarray(frame).save(os.path.join("S", stem + ".png"))
    assert sorted(stems) != stems
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--mask-output-imgs", "R0"]))
    assert H.load_models()
    M = H.segment("S")                                                      # the masks of these frames, in os.listdir's order
    listed = [f.rsplit(".", 1)[0] for f in os.listdir("S")]
    thr = float(np.median(M))
    on = objects_ref.on_pixels(M[:, 0], thr, inclusive=True)
    labels, _, kept, _, _ = objects_ref.label(on, 8, 2, 64)
    order = [listed.index(s) for s in stems]                                # the frames in their natural order
    t, side = _side(labels[order], kept[order], 300)
    assert side["links"] > 0

    common = ["-process", "--source-imgs", "S", "--binarymaskthreshold", repr(thr), "-objects", "--min-area", "2"]
    _run(common + ["--mask-output-imgs", "R1"], capsys)
    _run(common + ["--mask-output-imgs", "R2", "--track-iou", "0.3"], capsys)
    r1, r2 = _files("R1"), _files("R2")
    assert set(r2) - set(r1) == {"tracks.json"} | {f"{s}-tracks-mask.png" for s in stems}
    assert all(r2[f] == r1[f] for f in r1) and "objects.json" in r1
    report = json.loads(r2["tracks.json"])
    rows = objects.track_rows(t["table"], side["tracks"])
    assert report == {"source": "thresholded-mask", "threshold": thr, "connectivity": 8, "min_area": 2, "max_objects": 64, "track_iou": 0.3,
                      "summary": side, "order": stems,
                      "frames": {s: [{"label": l + 1, "track": int(t["track"][j, l]), "prev": int(t["prev"][j, l])} for l in np.flatnonzero(t["track"][j])]
                                 for j, s in enumerate(stems)},
                      "tracks": [{"track": r["track"], "first": stems[r["first_frame"]], "last": stems[r["first_frame"] + r["length"] - 1],
                                  "length": r["length"], "area_sum": r["area_sum"], "area_min": r["area_min"], "area_max": r["area_max"],
                                  "link_iou": r["link_iou"]} for r in rows]}
    painted = ref.track(labels[order], 300, 64, want_paint=True)["track_labels"]
    for j, s in enumerate(stems):
        np.testing.assert_array_equal(np.array(Image.open(os.path.join("R2", f"{s}-tracks-mask.png"))), ref.colours(painted[j]))
