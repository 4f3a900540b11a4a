"""Dense-CRF refinement on the GPU (cgs_dense_crf2 / cgs_amd.crf.dense_crf / Handler.crf / -crf on the CLI) against the float64
restatement tests/crf_ref.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import crf_ref  # noqa: E402
from cgs_amd import _lib, cli, crf, handler  # noqa: E402  (attributes of the package: no second copy of a submodule under the alias)

pytestmark = pytest.mark.gpu
DEV = "cuda"
REF = crf.REFERENCE_PARAMS
ALT = (5, 30, 10, 3, 3, 5)


def _structured(h, w, seed):
    """A frame of flat blocks and repeated rows, and a sigmoid-of-signed-distance disc mask plus noise with exact 0.0 / 1.0 pixels."""
    rs = np.random.RandomState(seed)
    frame = np.zeros((h, w, 3), np.uint8)
    for _ in range(6):
        y0, x0 = rs.randint(0, h), rs.randint(0, w)
        frame[y0:y0 + rs.randint(4, h // 2 + 4), x0:x0 + rs.randint(4, w // 2 + 4)] = rs.randint(0, 256, 3)
    frame[h // 3] = rs.randint(0, 256, (w, 3))
    frame[h // 3 + 1:h // 3 + 4] = frame[h // 3]
    frame = np.clip(frame.astype(int) + rs.randint(-2, 3, frame.shape), 0, 255).astype(np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    sd = (min(h, w) / 3.0 - np.hypot(xs - w / 2.0, ys - h / 2.0)) / 3.0
    p = 1.0 / (1.0 + np.exp(-sd)) + rs.normal(0, 0.15, (h, w))
    p = np.clip(p, 0.0, 1.0).astype(np.float32)
    p[rs.rand(h, w) < 0.03] = 1.0
    p[rs.rand(h, w) < 0.03] = 0.0
    return frame, p


def _g2(golden, k):
    g = golden("g2_eval.npz")
    return g["X"][:k], g["Z"][:k, 0].astype(np.float32)


def _gpu(frames, p1, params, q=True):
    f = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    p = torch.from_numpy(np.ascontiguousarray(p1, dtype=np.float32)).to(DEV)
    out = crf.dense_crf(f, p, params, return_q=q)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) if q else out.cpu().numpy()


def _one_step_parity(frames, p1s, params, steps):
    it_all = params[5]
    qs = {t: _gpu(frames, p1s, params[:5] + (t,))[1] for t in sorted(set(steps) | {t + 1 for t in steps}) if t <= it_all}
    worst = 0.0
    for k in range(len(frames)):
        F = crf_ref.Frame(frames[k], p1s[k], params)
        if 0 in qs:
            np.testing.assert_allclose(qs[0][k], F.start(), rtol=0, atol=1e-6)
        for t in steps:
            want = F.step(qs[t][k].astype(np.float64))
            err = float(np.abs(qs[t + 1][k] - want).max())
            worst = max(worst, err)
            assert err <= 1e-5, (k, t, err)
    return worst


@pytest.mark.parametrize("params", [REF, ALT], ids=["reference", "alt"])
def test_one_step_parity_64(golden, params):
    X, Z = _g2(golden, 3)
    S = [_structured(64, 64, s) for s in range(3)]
    frames = np.concatenate([X, np.stack([f for f, _ in S])])
    p1s = np.concatenate([Z, np.stack([p for _, p in S])])
    steps = list(range(params[5]))
    _one_step_parity(frames, p1s, params, steps)


@pytest.mark.parametrize("params", [REF, ALT], ids=["reference", "alt"])
def test_one_step_parity_odd_shape(params):
    S = [_structured(37, 23, 10 + s) for s in range(2)]
    _one_step_parity(np.stack([f for f, _ in S]), np.stack([p for _, p in S]), params, list(range(params[5])))


def test_one_step_parity_128():
    f, p = _structured(128, 128, 20)
    _one_step_parity(f[None], p[None], REF[:5] + (10,), [0, 9])


def test_full_run_matches_oracle(golden):
    X, Z = _g2(golden, 2)
    S = [_structured(64, 64, 30 + s) for s in range(2)]
    frames = np.concatenate([X, np.stack([f for f, _ in S])])
    p1s = np.concatenate([Z, np.stack([p for _, p in S])])
    lab, q = _gpu(frames, p1s, REF)
    for k in range(len(frames)):
        wl, wq, d = crf_ref.Frame(frames[k], p1s[k], REF).run()
        sure = np.abs(d) >= 1e-2
        assert ((lab[k] != wl) & sure).sum() == 0, k
        assert np.abs(q[k] - wq).max() <= 1e-4, (k, np.abs(q[k] - wq).max())
    # zero iterations: the argmax of P, Q = P's softmax
    lab0, q0 = _gpu(frames, p1s, REF[:5] + (0,))
    np.testing.assert_array_equal(lab0, (p1s > np.float32(1) - p1s).astype(np.uint8))


def test_deterministic_and_batch_independent():
    rs = np.random.RandomState(5)
    n = 256
    frames = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    p1s = rs.uniform(0, 1, (n, 64, 64)).astype(np.float32)
    for k in range(0, n, 3):
        frames[k], p1s[k] = _structured(64, 64, 100 + k)
    a = _gpu(frames, p1s, REF)
    b = _gpu(frames, p1s, REF)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for k in (0, 77, 255):
        lone = _gpu(frames[k:k + 1], p1s[k:k + 1], REF)
        assert lone[0].tobytes() == a[0][k:k + 1].tobytes() and lone[1].tobytes() == a[1][k:k + 1].tobytes()


def test_bad_arguments_return_error_codes():
    lib = _lib.load()
    fr = torch.zeros((1, 128, 129, 3), dtype=torch.uint8, device=DEV)
    p = torch.zeros((1, 128, 129), dtype=torch.float32, device=DEV)
    lab = torch.zeros((1, 128, 129), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n, h, w, params, frames=fr.data_ptr(), labels=lab.data_ptr()):
        prm = _lib.CrfParams(*[float(v) for v in params[:5]], int(params[5]))
        return lib.cgs_dense_crf2(frames, p.data_ptr(), n, h, w, ctypes.byref(prm), labels, None, stream)
    assert call(1, 128, 129, REF) == _lib.ERR_UNSUPPORTED                # h * w > 16384
    assert call(0, 8, 8, REF) == _lib.ERR_BADARG
    assert call(1, 0, 8, REF) == _lib.ERR_BADARG
    assert call(1, 8, 8, (22, 0, 3.1, 8, 1.8, 10)) == _lib.ERR_BADARG
    assert call(1, 8, 8, (22, 12, -1, 8, 1.8, 10)) == _lib.ERR_BADARG
    assert call(1, 8, 8, (22, 12, 3.1, 8, 0, 10)) == _lib.ERR_BADARG
    assert call(1, 8, 8, (22, 12, 3.1, 8, 1.8, -1)) == _lib.ERR_BADARG
    assert call(1, 8, 8, REF, frames=None) == _lib.ERR_BADARG
    assert call(1, 8, 8, REF, labels=None) == _lib.ERR_BADARG
    torch.cuda.synchronize()
    with pytest.raises(_lib.CgsError):
        crf.dense_crf(fr, p)
    assert crf.dense_crf(fr[:, :64, :64].contiguous(), p[:, :64, :64].contiguous()).shape == (1, 64, 64)


# ---------------------------------------------------------------- CLI, end to end
def _setup_model(root, golden, g1):
    pc, pm = g1
    g = golden("g6_process.npz")
    for c in [str(s) for s in g["checkpoint_names"]]:
        os.makedirs(os.path.dirname(os.path.join(root, c)), exist_ok=True)
    cn = [str(s) for s in g["checkpoint_names"]]
    torch.save(pc, os.path.join(root, cn[0]))
    torch.save(pm, os.path.join(root, cn[1]))
    return g["frames"], [str(s) for s in g["names"]]


def _main(root, args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py")] + args + ["--model", "m"], cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_cli_process_crf(tmp_path, golden, g1, monkeypatch):
    from PIL import Image
    root = str(tmp_path)
    X, names = _setup_model(root, golden, g1)
    os.makedirs(os.path.join(root, "src"))
    for nm, x in zip(names, X):
        Image.fromarray(x).save(os.path.join(root, "src", nm + ".png"))
    _main(root, ["-process", "-crf", "--source-imgs", "src", "--mask-output-imgs", "o1"])
    assert sorted(os.listdir(os.path.join(root, "o1"))) == sorted(f"{s}-{c}.png" for s in names
                                                                  for c in ("raw-mask", "thresholded-mask", "crf-mask"))
    # the masks this build computes for the same files, in the same order, through the same engine
    monkeypatch.chdir(root)
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    files = os.listdir("src")
    frames = np.stack([np.array(Image.open(os.path.join("src", f)))[..., :3] for f in files])
    _, M, _ = H._sweep_masks(frames / 255.0, lambda c: torch.from_numpy(c).float().to(H.device), "x")
    want = _gpu(frames, M[:, 0], REF, q=False)
    for i, f in enumerate(files):
        stem = f.rsplit(".", 1)[0]
        got = _png(os.path.join("o1", f"{stem}-crf-mask.png"))
        np.testing.assert_array_equal(got[..., 0], want[i] * 255)
    # --binarymaskthreshold 0: the CRF column takes position 2 and its name
    _main(root, ["-process", "-crf", "--binarymaskthreshold", "0", "--source-imgs", "src", "--mask-output-imgs", "o2"])
    assert sorted(os.listdir("o2")) == sorted(f"{s}-{c}.png" for s in names for c in ("raw-mask", "thresholded-mask"))
    for i, f in enumerate(files):
        np.testing.assert_array_equal(_png(os.path.join("o2", f.rsplit(".", 1)[0] + "-thresholded-mask.png"))[..., 0], want[i] * 255)
    # -salience -process_salience -crf: six columns, by position; the concatenated strip holds them all
    _main(root, ["-process", "-salience", "-process_salience", "-crf", "--salience-thresh", "0.5", "--source-imgs", "src",
                 "--mask-output-imgs", "o3"])
    kinds = ("raw-mask", "thresholded-mask", "crf-mask", "saliency-map", "thresholded-saliency", "crf-saliency")
    assert sorted(os.listdir("o3")) == sorted(f"{s}-{c}.png" for s in names for c in kinds)
    _main(root, ["-process", "-salience", "-process_salience", "-crf", "-concatenated", "--salience-thresh", "0.5",
                 "--source-imgs", "src", "--mask-output-imgs", "o4"])
    strip = _png(os.path.join("o4", files[0].rsplit(".", 1)[0] + "_with_mask.png"))
    assert strip.shape == (64, 64 * 7, 3)
    np.testing.assert_array_equal(strip[:, 192:256, 0], want[0] * 255)
    np.testing.assert_array_equal(strip[:, 192:256], _png(os.path.join("o3", files[0].rsplit(".", 1)[0] + "-crf-mask.png")))


def test_cli_eval_crf(tmp_path, golden, g1, monkeypatch):
    root = str(tmp_path)
    _setup_model(root, golden, g1)
    os.makedirs(os.path.join(root, "red-trees"))
    rs = np.random.RandomState(11)
    Xe = np.stack([_structured(64, 64, 200 + k % 40)[0] for k in range(420)])
    Ye = np.zeros((420, 64, 64, 3), dtype=bool)
    Ye[:, 16:48, 8:40] = True
    Ye[:, 20:30, 10:20, 1] = rs.rand(10, 10) < 0.5
    np.save(os.path.join(root, "red-trees", "X.npy"), Xe)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Ye)
    out = _main(root, ["-eval", "-crf"])
    got = [float(v) for v in out.split("RESULTS [")[-1].split("]")[0].split(",")]
    monkeypatch.chdir(root)
    H = handler.Handler(cli.parse_args(["--model", "m"]))
    assert H.load_models()
    pick = slice(100, 5000, 2)
    frames, truth = Xe[pick], Ye[pick].all(axis=-1)
    _, M, _ = H._sweep_masks(frames, lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(H.device), "x")
    labels = _gpu(frames, M[:, 0], REF, q=False)
    assert len(got) == 2
    assert got[0] == handler.Handler.get_iou(M[:, 0] > H.args.eval_thresh, truth)
    assert got[1] == handler.Handler.get_iou(labels, truth)
    for i in range(0, len(frames), 50):
        for kind in ("mask", "img", "crf"):
            assert os.path.isfile(os.path.join("m", "crf", f"{i}_{kind}.png")), (i, kind)
    out = _main(root, ["-eval", "-salience", "-crf", "--salience-thresh", "0.5"])
    got2 = [float(v) for v in out.split("RESULTS [")[-1].split("]")[0].split(",")]
    assert len(got2) == 4 and got2[:2] == got
