"""The training loops' PNG sheets on the GPU (cgs_sheet_compose / cgs_amd.sheets / the CLI) against the numpy + PIL restatement
tests/sheet_ref.py and against the reference's own sheets (G15, tests/golden/make_golden_sheets.py)."""
import gzip
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REPO)

import sheet_ref  # noqa: E402
from loop_inputs import synthetic_frames  # noqa: E402
from test_sheet_host import g15, g15_critic_inputs, g15_segment_inputs, text_rendering_differs  # noqa: E402
from cgs_amd import _lib, cli, handler, sheets, video  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu_pixels(A, B, Z, **kw):
    out = sheets.compose(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(Z).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same_bytes(got, want, what):
    bad = got != want
    if bad.any():
        y, x, c = np.argwhere(bad)[0]
        print(f"{what}: {int(bad.sum())} differing bytes of {bad.size}; first at row {y} (tile row {y // 64}), column {x}, channel {c}: "
              f"{got[y, x, c]} != {want[y, x, c]}")
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- kernel vs restatement
def test_compose_on_the_reference_inputs_is_byte_exact(golden):
    g = g15(golden)
    A, B = g15_segment_inputs(g)
    want = sheet_ref.pixels(A, B, g["Z"])
    assert sheet_ref.column_hashes(want, 128) == [str(h) for h in g["segment_sha256"]]      # = the reference's file below its label band
    got = gpu_pixels(A, B, g["Z"])
    assert got.shape == (448, 4096, 3) and got.dtype == np.uint8
    assert_same_bytes(got, want, "G15")                     # every byte, the two zero rows included
    assert sheet_ref.column_hashes(got, 128) == [str(h) for h in g["segment_sha256"]]


def edge_masks(rs, n):
    """fp32 [n,64,64] in [0, 1]: exactly 0 and 1, k / 255 and its float32 neighbours (mixes on and next to byte boundaries), uniform."""
    k = rs.randint(0, 256, (n, 64, 64))
    exact = (k / 255.0).astype(np.float32)
    side = rs.randint(0, 3, (n, 64, 64))
    v = np.where(side == 1, np.nextafter(exact, np.float32(0)), np.where(side == 2, np.nextafter(exact, np.float32(1)), exact))
    v = np.where(rs.rand(n, 64, 64) < 0.5, rs.rand(n, 64, 64).astype(np.float32), v)
    v[:, :2] = 0
    v[:, 2:4] = 1
    return np.clip(v, 0, 1).astype(np.float32)


@pytest.mark.parametrize("n", [1, 3, 64, 512])
def test_compose_random_inputs_are_byte_exact(n):
    rs = np.random.RandomState(100 + n)
    A, B = (rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8) for _ in range(2))
    A[:, 4:6], B[:, 5:7] = 255, 0
    Z = edge_masks(rs, n)
    assert (Z == 0).any() and (Z == 1).any()
    want = sheet_ref.pixels(A, B, Z)
    got = gpu_pixels(A, B, Z)
    assert got.shape == (448, 64 * n, 3)
    assert_same_bytes(got, want, f"n={n}")
    # into a given buffer, and the mask as [n,1,64,64]
    out = torch.full((448, 64 * n, 3), 7, dtype=torch.uint8, device="cuda")
    r = sheets.compose(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(Z).cuda()[:, None], out=out)
    assert r.data_ptr() == out.data_ptr()
    assert_same_bytes(out.cpu().numpy(), want, f"n={n} (out=)")


def test_argument_errors():
    lib = _lib.load()
    A = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device="cuda")
    Z = torch.zeros(2, 64, 64, device="cuda")
    out = torch.full(sheets.sheet_shape(2), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda a, b, z, n, o: lib.cgs_sheet_compose(a, b, z, n, o, s)
    assert call(A.data_ptr(), A.data_ptr(), Z.data_ptr(), 0, out.data_ptr()) < 0
    assert call(A.data_ptr(), A.data_ptr(), Z.data_ptr(), -1, out.data_ptr()) < 0
    assert call(None, A.data_ptr(), Z.data_ptr(), 2, out.data_ptr()) < 0
    assert call(A.data_ptr(), None, Z.data_ptr(), 2, out.data_ptr()) < 0
    assert call(A.data_ptr(), A.data_ptr(), None, 2, out.data_ptr()) < 0
    assert call(A.data_ptr(), A.data_ptr(), Z.data_ptr(), 2, None) < 0
    assert call(A.data_ptr(), A.data_ptr(), Z.data_ptr(), 2, out.data_ptr() + 1) < 0
    torch.cuda.synchronize()
    assert bool((out == 9).all())                            # nothing was launched
    assert call(A.data_ptr(), A.data_ptr(), Z.data_ptr(), 2, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool(out.any())
    for bad in ((A.float(), A, Z), (A, A[:1], Z), (A, A, Z.double()), (A, A, Z[:, :32]), (A.cpu(), A, Z)):
        with pytest.raises((ValueError, _lib.CgsError)):
            sheets.compose(*bad)
    with pytest.raises(ValueError):
        sheets.compose(A, A, Z, out=out[:, :64])


# ---------------------------------------------------------------- the CLI, end to end
def run_train(root, g, g9, g1, extra, mp):
    """G15's segment command line in-process (the reference's phase-1 critic and the G1 masker as the two checkpoints, the
    generator's seeding hook around segmentation_training).  Returns (handler, what submit_segment was given at step 0)."""
    pm = g1[1]
    critic = {k[len("critic_after_p1/"):]: torch.from_numpy(v) for k, v in g9.items() if k.startswith("critic_after_p1/")}
    datasize, testsize = int(g["datasize"]), int(g["testsize"])
    for name, state in zip((str(s) for s in g["checkpoint_names"]), (critic, pm)):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "runs/data/straight"))
    with gzip.GzipFile(os.path.join(root, f"runs/data/straight/Treechop-trunk-{datasize}-[0.98-0.97-0.96-0.95].pickle"), "wb") as fp:
        pickle.dump(synthetic_frames(datasize + testsize, int(g["data_seed"])), fp)
    seed = int(g["seed"])
    real_seg, real_submit = handler.Handler.segmentation_training, sheets.SheetWriter.submit_segment
    first = {}

    def segmentation_training(self):
        self.start_trace()
        np.random.seed(seed)
        torch.manual_seed(seed)
        return real_seg(self)

    def submit_segment(self, path, A, B, Z, labels_host, labels_dev, inject):
        if not first:                                        # (test only) what step 0 handed over, cloned before the loop goes on
            first.update(path=path, A=A.cpu().numpy(), B=B.cpu().numpy(), Z=Z.cpu().numpy(), Y=[float(v) for v in labels_host],
                         values=[None if v is None else v.cpu().tolist() for v in labels_dev], inject=inject)
        return real_submit(self, path, A, B, Z, labels_host, labels_dev, inject)
    mp.chdir(root)
    mp.setattr(handler.Handler, "segmentation_training", segmentation_training)
    mp.setattr(sheets.SheetWriter, "submit_segment", submit_segment)
    argv = [a for a in json.loads(str(g["argv_json"]))]
    assert argv[-2:] == ["--visevery", "1"]
    H = cli.main(argv[:-2] + extra)
    torch.cuda.synchronize()
    return H, first


@pytest.fixture(scope="module")
def train_run(tmp_path_factory, golden, g1):
    g, g9 = g15(golden), golden("g9_train_loop.npz")
    mp = pytest.MonkeyPatch()
    try:
        root = str(tmp_path_factory.mktemp("sheets_on"))
        H, first = run_train(root, g, g9, g1, ["--visevery", "1"], mp)
        losses = torch.stack(H._trace["p2_loss"]).cpu().numpy()
    finally:
        mp.undo()
    return {"g": g, "g9": g9, "root": root, "first": first, "losses": losses, "H": H}


def test_train_writes_the_reference_listing(train_run):
    g, root = train_run["g"], train_run["root"]
    assert sorted(os.listdir(os.path.join(root, "m/segment"))) == json.loads(str(g["listing_json"]))
    assert json.loads(str(train_run["g9"]["listing_json"]))["segment"] == ["_loss.png", "e0_b0.png", "log.txt"]     # G9: --visevery 100
    assert {"pred_idx1_hist.png", "GT_idx1_hist.png"} <= set(os.listdir(os.path.join(root, "m")))                    # main.py:255-264
    assert train_run["first"]["path"] == "m/segment/e0_b0.png"


def test_train_sheet_vs_the_reference_sheet(train_run):
    from PIL import Image
    g, root, first = train_run["g"], train_run["root"], train_run["first"]
    A, B = g15_segment_inputs(g)
    ref = sheet_ref.pixels(A, B, g["Z"])                     # = the reference's e0_b0.png below its label band (hashes, checked here)
    assert sheet_ref.column_hashes(ref, 128) == [str(h) for h in g["segment_sha256"]]
    got = np.array(Image.open(os.path.join(root, "m/segment/e0_b0.png")))
    assert got.shape == ref.shape == (448, 4096, 3)
    np.testing.assert_array_equal(got[128:256], ref[128:256])                        # the A and B rows: the reference's bytes
    # replaced, injected and Z: the project's mask parity is 1e-3 and 255 x 1e-3 < 1 before truncation, so within 1 per byte
    d = np.abs(got[256:].astype(np.int32) - ref[256:].astype(np.int32))
    for k, name in enumerate(("replaced", "injected", "Z")):
        part = d[64 * k:64 * k + 64]
        print(f"e0_b0.png {name}: max |difference| {part.max()}, share of differing bytes {float((part > 0).mean()):.2e}")
    print(f"e0_b0.png rows 256-447: share of differing bytes {float((d > 0).mean()):.2e}")
    assert d.max() <= 1
    # the file is the restatement of what the engine handed over at step 0, labels included (same PIL on both sides)
    np.testing.assert_array_equal(first["A"], A)
    np.testing.assert_array_equal(first["B"], B)
    np.testing.assert_array_equal(first["Y"], g["Y"])                                # float64 targets from the host
    font, _ = video.resolve_font(sheets.FONT_SIZE)
    vals = first["values"]
    assert first["inject"] and len(vals) == 4
    for mine, name in zip(vals, ("pred", "negpred", "replacevalue", "injectvalue")):
        err = float(np.abs(np.array(mine) - g[name]).max())
        print(f"step 0 {name}: max |value - reference| {err:.1e}")
        assert err <= 1e-3
    want = sheet_ref.segment_sheet(first["A"], first["B"], first["Z"], first["Y"], *vals, font)
    assert_same_bytes(got, want, "e0_b0.png vs the restatement of the engine's tensors")


def test_losses_are_bit_identical_with_and_without_sheets(train_run, tmp_path, golden, g1):
    mp = pytest.MonkeyPatch()
    try:
        H, first = run_train(str(tmp_path), train_run["g"], train_run["g9"], g1, ["--visevery", "0"], mp)
        off = torch.stack(H._trace["p2_loss"]).cpu().numpy()
    finally:
        mp.undo()
    assert not first and H.sheet_drain_s == 0.0
    assert [f for f in os.listdir(tmp_path / "m/segment") if f.startswith("e")] == []          # --visevery 0: no sheets
    on = train_run["losses"]
    assert on.shape == off.shape and on.shape[0] == len(train_run["g9"]["p2_choice"])
    assert on.tobytes() == off.tobytes(), f"per-step losses differ in {int((on != off).sum())} of {on.size} values"
    # and the loop is the reference's: G9's loss tolerances hold with a sheet after every step
    g9 = train_run["g9"]
    want = np.concatenate((g9["p2_loss_critic_replace_inject"], 0.5 * g9["p2_loss_l1_mean"][:, None]), axis=1)
    e2 = np.abs(on[:, :4] - want) / np.abs(want)
    assert e2[:8].max() <= 1e-3


def test_critic_training_writes_its_sheet(tmp_path, golden, g1, monkeypatch):
    from PIL import Image
    g = g15(golden)
    pc, pm = g1
    ds, ts, seed = int(g["critic_datasize"]), int(g["critic_testsize"]), int(g["critic_seed"])
    monkeypatch.chdir(tmp_path)
    os.makedirs("runs/data/straight")
    with gzip.GzipFile(f"runs/data/straight/Treechop-trunk-{ds}-[0.98-0.97-0.96-0.95].pickle", "wb") as fp:
        pickle.dump(synthetic_frames(ds + ts, 9), fp)
    real_cp = handler.Handler.critic_pipe

    def critic_pipe(self, mode="train", test=0):
        self.critic.load_state_dict(pc)
        self.masker.load_state_dict(pm)
        np.random.seed(seed)
        torch.manual_seed(seed)
        return real_cp(self, mode, test)
    monkeypatch.setattr(handler.Handler, "critic_pipe", critic_pipe)
    cli.main(json.loads(str(g["critic_argv_json"])))
    assert sorted(os.listdir("m/critic")) == json.loads(str(g["critic_listing_json"]))
    got = np.array(Image.open("m/critic/e0_b0.png"))
    frames = np.concatenate(g15_critic_inputs(g), axis=1)
    assert got.shape == frames.shape
    for rows in (slice(16, 32), slice(48, 64)):              # outside the label bands: the batch the reference drew, byte for byte
        np.testing.assert_array_equal(got[rows], frames[rows])
    font, _ = video.resolve_font(sheets.FONT_SIZE)
    why = text_rendering_differs(g, font.getname())
    if why:
        print(why)
    else:
        np.testing.assert_array_equal(got[0:16], g["critic_bands"][0])   # the targets are the data's: the reference's text
    # the prediction band holds 3-digit strings of values that may differ from the reference's in the third decimal: reported only
    assert got[32:48].any()
    band = sheet_ref.critic_sheet(g15_critic_inputs(g), g["critic_Y"].tolist(), g["critic_pred"].tolist(), font)[32:48]
    differing = int((got[32:48] != band).any(axis=(0, 2)).reshape(-1, 64).any(axis=1).sum())
    print(f"critic sheet: {differing} of {len(g['critic_pred'])} prediction labels differ from the reference's strings")
