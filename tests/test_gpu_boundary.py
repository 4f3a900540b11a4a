"""Boundary scoring on the GPU (cgs_boundary_score, cgs_amd.boundary.score, -eval --boundary-tol) against the neighbour lookups and the
explicit distance lists of tests/boundary_ref.py.  Everything the kernel gives is integer: exact equality everywhere."""
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

import boundary_ref as ref  # noqa: E402
import objects_match_ref  # noqa: E402
import objects_ref  # noqa: E402
from cgs_amd import _lib, boundary, cli, handler, metrics  # noqa: E402
from test_gpu_objects_match import _results, _run, workdir  # noqa: E402, F401  (the small evaluation fixture of eval_match.json)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = (0, 1, 2, 3)
HAND = ref.hand_made()


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu(pred, truth, tol=TOL, want_dist2=True, **kw):
    """boundary.score on a stack (arrays are uploaded as they are), back on the host as the checker's (counts [n, 4 + 4 T], dist2)."""
    res = boundary.score(_up(pred), _up(truth), tol=tol, want_dist2=want_dist2, **kw)
    torch.cuda.synchronize()
    n, T = res.pred_px.shape[0], len(tol)
    assert all(t.shape == (n,) for t in res[:4]) and all(t.shape == (n, T) for t in res[4:8])
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" and t.is_contiguous() for t in res if t is not None)
    counts = np.empty((n, 4 + 4 * T), dtype=np.int32)
    for i in range(4):
        counts[:, i] = res[i].cpu().numpy()
        counts[:, 4 + i::4] = res[4 + i].cpu().numpy()
    return counts, (None if res.dist2 is None else res.dist2.cpu().numpy())


def _check(pred, truth, tol=TOL):
    """pred, truth: bool [n,h,w].  The kernel's answer must be the checker's; returns the checker's (counts, dist2)."""
    want = ref.score(pred, truth, boundary.tol_squared(tol))
    counts, dist2 = _gpu(pred, truth, tol)
    np.testing.assert_array_equal(counts, want[0], err_msg="counts")
    assert dist2.shape == want[1].shape
    np.testing.assert_array_equal(dist2, want[1], err_msg="dist2")
    return want


# ---------------------------------------------------------------- 1. the generator frames
def test_generator_frames():
    pred, truth = (np.stack(side) for side in zip(*(objects_match_ref.generator_frame(s) for s in range(6))))
    want = ref.score(pred, truth, boundary.tol_squared(TOL))[0]
    pred_px, truth_px, _, _, hit_pred, hit_truth, _, _ = ref.split_counts(want)
    # about the checker, not the kernel: the frames test something
    hits = [(int(hit_pred[:, k].sum()), int(hit_truth[:, k].sum())) for k in range(4)]
    assert hits == [(945, 945), (1373, 1401), (1456, 1470), (1492, 1567)] and (int(pred_px.sum()), int(truth_px.sum())) == (1930, 2026)
    assert all(hits[k][s] < hits[k + 1][s] for k in (0, 1) for s in (0, 1))                  # strictly more from 0 to 1 to 2 ...
    assert hits[3][0] < pred_px.sum() and hits[3][1] < truth_px.sum()                       # ... and still not everything at 3
    _check(pred, truth)


# ---------------------------------------------------------------- 2. identities that need no checker
def test_identities():
    pred, truth = (np.stack(side) for side in zip(*(objects_match_ref.generator_frame(s) for s in range(6))))
    rs = np.random.RandomState(11)
    pred = np.concatenate([pred, rs.rand(4, 64, 64) < 0.5])
    truth = np.concatenate([truth, rs.rand(4, 64, 64) < 0.6])
    res = boundary.score(_up(pred), _up(truth), tol=(0, 128))
    assert int(res.pred_px.min()) > 0 and int(res.truth_px.min()) > 0
    # tolerance 0: a hit is a pixel on both boundaries, from either side, and the two bands are the boundaries themselves
    assert torch.equal(res.hit_pred[:, 0], res.hit_truth[:, 0]) and torch.equal(res.hit_pred[:, 0], res.band_inter[:, 0])
    assert torch.equal(res.band_union[:, 0], res.pred_px + res.truth_px - res.band_inter[:, 0]) and int(res.hit_pred[:, 0].sum()) > 0
    # tolerance 128: everything is near, and the bands are the masks
    assert torch.equal(res.hit_pred[:, 1], res.pred_px) and torch.equal(res.hit_truth[:, 1], res.truth_px)
    for i in range(pred.shape[0]):
        inter, union = metrics.iou_counts(_up(pred[i]), _up(truth[i])).tolist()
        assert (int(res.band_inter[i, 1]), int(res.band_union[i, 1])) == (inter, union), i
    assert torch.equal(res.hd2_pred >= 0, torch.ones_like(res.hd2_pred, dtype=torch.bool))


# ---------------------------------------------------------------- 3. hand-made frames, alone and in one stack
@pytest.mark.parametrize("name", [f[0] for f in HAND])
def test_hand_made_frame(name):
    pred, truth = next((p, t) for n, p, t in HAND if n == name)
    tol = (0, 1, 89.0, 89.1)
    counts, dist2 = _check(pred[None], truth[None], tol)
    c = counts[0].tolist()
    ring = 2 * (64 + 64) - 4
    if name == "both_empty":
        assert c == [0, 0, -1, -1] + [0] * 16 and (dist2 == -1).all()
    elif name == "empty_vs_full":
        assert c[:4] == [0, ring, -1, -1] and c[4:8] == [0, 0, 0, ring] and c[16:20] == [0, 0, 0, 4096]
        assert (dist2[0, 0] == -1).all() and dist2[0, 1].max() == 31 * 31
    elif name == "full_vs_empty":
        assert c[:4] == [ring, 0, -1, -1] and c[4:8] == [0, 0, 0, ring] and c[16:20] == [0, 0, 0, 4096]
    elif name == "full_vs_full":
        assert c[:4] == [ring, ring, 0, 0] and c[4:8] == [ring] * 4 and c[16:20] == [ring, ring, 4096, 4096]
    elif name == "corners":
        assert c[:4] == [1, 1, 7938, 7938]
        assert c[12:16] == [0, 0, 0, 2] and c[16:20] == [1, 1, 0, 2]      # 89.0^2 = 7921 < 7938 = floor(89.1^2)
    elif name == "block_shifted":
        assert c[:4] == [8, 8, 1, 1] and c[4:8] == [4, 4, 4, 12] and c[8:12] == [8, 8, 6, 12]
    elif name == "checkerboard":
        assert c[:4] == [2048, 2048, 1, 1] and c[4:8] == [0, 0, 0, 4096] and c[8:12] == [2048, 2048, 0, 4096]
    elif name == "last_row_and_column":
        assert c[:4] == [127, 24, 63 * 63, 0] and c[4:8] == [24, 24, 24, 127]


def test_hand_made_stack():
    """All of them in one launch, and once more in reverse order: a frame's row holds that frame's counts."""
    pred, truth = np.stack([f[1] for f in HAND]), np.stack([f[2] for f in HAND])
    counts, dist2 = _check(pred, truth)
    back, back2 = _gpu(pred[::-1].copy(), truth[::-1].copy())
    np.testing.assert_array_equal(back[::-1], counts)
    np.testing.assert_array_equal(back2[::-1], dist2)


# ---------------------------------------------------------------- 4. shapes
@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (64, 1), (5, 7), (63, 64), (64, 63)])
def test_shapes(h, w):
    rs = np.random.RandomState(100 * h + w)
    pred, truth = rs.rand(3, h, w) < 0.5, rs.rand(3, h, w) < 0.5
    pred[0], truth[0] = True, True                                         # a full frame of this shape: the ring (or all of it)
    truth[1, h // 2, w // 2] = pred[1, h // 2, w // 2]                     # at least one pixel agrees ...
    pred[2, 0, 0], truth[2, 0, 0] = True, False                            # ... and the corner differs
    counts, _ = _check(pred, truth)
    assert counts[0, 0] == counts[0, 1] == (h * w if min(h, w) <= 2 else 2 * (h + w) - 4)


def test_views_and_one_frame():
    rs = np.random.RandomState(5)
    wide_p, wide_t = (torch.from_numpy(rs.rand(3, 64, 128) < 0.5).to(DEV) for _ in range(2))
    vp, vt = wide_p[:, :, ::2], wide_t[:, :, 1::2]
    assert not vp.is_contiguous() and not vt.is_contiguous()
    counts, dist2 = _gpu(vp, vt)
    want = ref.score(vp.cpu().numpy(), vt.cpu().numpy(), boundary.tol_squared(TOL))
    np.testing.assert_array_equal(counts, want[0])
    np.testing.assert_array_equal(dist2, want[1])                         # the whole plane, both sides
    tp, tt = wide_p[0, :, :40].t(), wide_t[0, :, :40].t()                  # one frame [40,64], transposed
    assert not tp.is_contiguous()
    counts, dist2 = _gpu(tp, tt)
    want = ref.score(tp.cpu().numpy()[None], tt.cpu().numpy()[None], boundary.tol_squared(TOL))
    np.testing.assert_array_equal(counts, want[0])
    np.testing.assert_array_equal(dist2, want[1])
    assert _gpu(tp, tt, want_dist2=False)[1] is None
    np.testing.assert_array_equal(_gpu(tp, tt, want_dist2=False)[0], want[0])


# ---------------------------------------------------------------- 5. more workgroups than one wave of CUs
def test_many_frames():
    rs = np.random.RandomState(9)
    pred, truth = rs.rand(300, 8, 8) < 0.45, rs.rand(300, 8, 8) < 0.45
    pred[7], truth[11], truth[299] = False, False, False
    assert len({p.tobytes() + t.tobytes() for p, t in zip(pred, truth)}) == 300
    _check(pred, truth, (0, 1, 1.5))


# ---------------------------------------------------------------- 6. tolerances
def test_tolerances():
    pred, truth = (np.stack(side) for side in zip(*(objects_match_ref.generator_frame(s) for s in (0, 1))))
    _check(pred, truth, (2,))
    sixteen = tuple(0.5 * k for k in range(15)) + (128,)
    counts, _ = _check(pred, truth, sixteen)
    assert len(set(counts[0, 4::4].tolist())) > 4                         # the tolerances are not all alike here
    mixed, _ = _check(pred, truth, (3, 0, 1.5))
    ordered, _ = _check(pred, truth, (0, 1.5, 3))
    np.testing.assert_array_equal(mixed[:, 4:].reshape(2, 3, 4), ordered[:, 4:].reshape(2, 3, 4)[:, [2, 0, 1]])


# ---------------------------------------------------------------- 7. input kinds
def test_input_kinds():
    rs = np.random.RandomState(21)
    on_p, on_t = rs.rand(2, 33, 47) < 0.5, rs.rand(2, 33, 47) < 0.5
    want = ref.score(on_p, on_t, boundary.tol_squared(TOL))
    for value in (2, 255):
        counts, dist2 = _gpu((on_p * value).astype(np.uint8), (on_t * 255).astype(np.uint8))
        np.testing.assert_array_equal(counts, want[0])
        np.testing.assert_array_equal(dist2, want[1])
    counts, _ = _gpu(on_p, (on_t * 2).astype(np.uint8))                    # bool against uint8
    np.testing.assert_array_equal(counts, want[0])
    # float32: values below, at and above the threshold, and a NaN
    thr = np.float32(0.3)
    prob = rs.choice(np.array([0.0, np.nextafter(thr, np.float32(0)), thr, np.nextafter(thr, np.float32(1)), 0.9], dtype=np.float32),
                     size=(2, 33, 47))
    prob[0, 3, 4], prob[1, 0, 0], prob[1, 32, 46] = np.nan, np.nan, thr
    for inclusive in (False, True):
        on = ref.on_pixels(prob, thr, inclusive)
        want_f = ref.score(on, on_t, boundary.tol_squared(TOL))
        counts, dist2 = _gpu(prob, on_t, thresh=float(thr), inclusive=inclusive)
        np.testing.assert_array_equal(counts, want_f[0], err_msg=f"inclusive={inclusive}")
        np.testing.assert_array_equal(dist2, want_f[1], err_msg=f"inclusive={inclusive}")
    assert (ref.on_pixels(prob, thr, True) != ref.on_pixels(prob, thr, False)).sum() > 100 and not ref.on_pixels(prob, thr, True)[0, 3, 4]


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors():
    z = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        boundary.score(z, z[:, :4])
    with pytest.raises(ValueError):
        boundary.score(torch.zeros(1, 65, 8, dtype=torch.uint8, device=DEV), torch.zeros(1, 65, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        boundary.score(z, z, tol=[0.5 * k for k in range(17)])
    with pytest.raises(ValueError):
        boundary.score(z.float(), z)
    with pytest.raises(_lib.CgsError):
        boundary.score(z.cpu(), z)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    tol2 = torch.zeros(17, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 4 + 4 * 17, dtype=torch.int32, device=DEV)
    args = lambda h, T: (z.data_ptr(), _lib.OBJ_U8, 0.0, z.data_ptr(), 1, h, 8, tol2.data_ptr(), T, out.data_ptr(), None, stream)
    assert lib.cgs_boundary_score(*args(65, 1)) == _lib.ERR_UNSUPPORTED and lib.cgs_boundary_score(*args(8, 17)) == _lib.ERR_BADARG
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                       # nothing was launched


# ---------------------------------------------------------------- 9. Handler and CLI
def test_cli_eval_boundary(workdir, capsys):
    root, frames = workdir
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    thr = float(np.median(M))                                        # a float32 value: half of the pixels are above it
    truth = M[:, 0] > np.float32(np.percentile(M, 55))               # the masks cut a little higher: outlines near, not on, the predicted ones
    Y = np.load(os.path.join(root, "red-trees", "Y.npy"))
    Y[slice(100, 5000, 2)] = truth[..., None]
    np.save(os.path.join(root, "red-trees", "Y.npy"), Y)
    tol = [0.0, 1.0, 2.0]
    on = ref.on_pixels(M[:, 0], thr)
    want = boundary.boundary_report(*ref.split_counts(ref.score(on, truth, boundary.tol_squared(tol))[0]), tol)
    first, last = want["per_tol"][0], want["per_tol"][-1]
    assert 0 < first["hit_pred"] < last["hit_pred"] < want["pred_px"] and want["hausdorff"]["frames"] > 0      # near misses at every tolerance
    out_file = os.path.join(root, "m", "eval_boundary.json")

    common = ["-crf", "-eval", "--eval-thresh", repr(thr), "-objects", "--min-area", "4"]
    H0, base = _run(common, capsys)
    assert not os.path.exists(out_file) and "BOUNDARY" not in base and H0.boundary is None
    with open(os.path.join(root, "m", "eval_objects.json"), "rb") as fp:
        objects_json = fp.read()
    H1, out = _run(common + ["--boundary-tol", "0-1-2"], capsys)
    assert out.count("\nBOUNDARY tol=0 (3 tolerances): mask f ") == 1 and out.index("OBJECTS") < out.index("BOUNDARY") < out.index("RESULTS")
    assert f"mask f {first['f']:.6f} boundary_iou {first['boundary_iou']:.6f}; crf f " in out and "; mask_objects f " in out
    assert _results(out) == _results(base)
    with open(os.path.join(root, "m", "eval_objects.json"), "rb") as fp:
        assert fp.read() == objects_json
    assert H1.objects == H0.objects
    with open(out_file) as fp:
        report = json.load(fp)
    assert report == H1.boundary and set(report) == {"tol", "tol2", "threshold", "mask", "crf", "mask_objects"}
    assert (report["tol"], report["tol2"], report["threshold"]) == (tol, [0, 1, 4], thr)
    assert report["mask"] == handler._json_safe(want)                      # the same integers through the same expressions
    # the other blocks: the stack each was given shows in its pixel counts and in tolerance 0, where a hit is a shared boundary pixel
    # and the bands are the boundaries -- no distances, so the checker's boundary() alone says what they must be
    bt = np.stack([ref.boundary(t) for t in truth])

    def cheap(block, on):
        bp = np.stack([ref.boundary(m) for m in on])
        row = block["per_tol"][0]
        assert (block["pred_px"], block["truth_px"]) == (int(bp.sum()), int(bt.sum()))
        assert (row["hit_pred"], row["hit_truth"], row["band_inter"], row["band_union"]) == (int((bp & bt).sum()),) * 3 + (int((bp | bt).sum()),)

    cheap(report["mask"], on)
    cheap(report["crf"], H.crf(frames, M, truth)[:, 0])
    cheap(report["mask_objects"], objects_ref.label(on, 8, 4, 64)[0] > 0)
