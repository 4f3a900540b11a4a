"""Frames of any size on the GPU (cgs_fit_down_u8, cgs_fit_up_joint, cgs_amd.fit, -process -fit) against tests/fit_ref.py: the box
average bit for bit in integers, the joint bilateral upsampling against float64 within 1e-5, its grey / hard outputs exactly consistent
with its own soft output, a step edge followed exactly, and the command line on the G6 fixture.

The 1e-5: an fp32 emulation of the formula in numpy (same tap order) stays within 3.3e-7 of float64; thirty times that leaves room for
the hardware exponential and the base-2 folding and is still far below one grey level (3.9e-3).  The largest error seen is printed."""
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

import fit_ref  # noqa: E402
from cgs_amd import _lib, cli, fit, handler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
UP_SIZES = ((65, 67), (96, 80), (128, 192))
SIGMAS = ((1.0, 16.0), (0.5, 2.0), (2.0, 64.0))
A, B = (200, 30, 30), (20, 60, 220)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)               # a copy: the shared cases are read-only


def _down(frames):
    return fit.down(_dev(frames)).cpu().numpy()


# ---------------------------------------------------------------- 1, 2: down
@pytest.mark.parametrize("n, h, w", [(3, 64, 64), (3, 65, 67), (3, 127, 64), (3, 128, 192), (3, 96, 80), (3, 360, 640), (1, 64, 4096),
                                     (1, 4096, 64)])
def test_down_bit_for_bit(n, h, w):
    rs = np.random.RandomState(h * 7 + w)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    got = _down(frames)
    assert got.shape == (n, 64, 64, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, fit_ref.down_ref(frames))
    if (h, w) == (64, 64):
        np.testing.assert_array_equal(got, frames)


def test_down_every_load_width():
    """The rows are read 16, 4 or 1 bytes at a time, by the alignment of the base and of 3 W: the same frames through all three (a view
    that starts 4 or 1 bytes into an allocation moves the base; 3 x 64 and 3 x 128 bytes are multiples of 16, 3 x 68 of 4 only)."""
    rs = np.random.RandomState(5)
    for h, w in ((70, 128), (64, 68), (66, 67)):
        frames = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
        want = fit_ref.down_ref(frames)
        for shift in (0, 4, 1):
            flat = torch.empty(frames.size + 16, dtype=torch.uint8, device=DEV)
            view = flat[shift:shift + frames.size].view(2, h, w, 3)
            view.copy_(_dev(frames))
            assert view.data_ptr() % 16 == shift and view.is_contiguous()
            np.testing.assert_array_equal(fit.down(view).cpu().numpy(), want, err_msg=f"{h}x{w} shift {shift}")


def test_down_accumulator_worst_case():
    """4096 x 4096: S reaches 255 x 4096^2, just under 2^32, and 2 S + H W does not fit 32 bits."""
    full = torch.full((1, 4096, 4096, 3), 255, dtype=torch.uint8, device=DEV)
    assert bool((fit.down(full) == 255).all())
    del full
    one = torch.zeros((1, 4096, 4096, 3), dtype=torch.uint8, device=DEV)
    one[0, -1, -1] = 255
    wy, wx = fit.box_weights(4096), fit.box_weights(4096)
    S = int(wy[63, 4095]) * int(wx[63, 4095]) * 255                      # the last cell, by hand from the weights: 64 x 64 x 255
    want = np.zeros((1, 64, 64, 3), dtype=np.uint8)
    want[0, 63, 63] = (2 * S + 4096 * 4096) // (2 * 4096 * 4096)
    assert S == 64 * 64 * 255 and want[0, 63, 63, 0] == 0
    np.testing.assert_array_equal(fit.down(one).cpu().numpy(), want)
    one[0, -64:, -64:] = 255                                             # the whole last cell, and half of the cell to its left
    one[0, -64:, -128:-64:2] = 255
    want[0, 63, 63], want[0, 63, 62] = 255, 128                          # 127.5 rounds half up
    np.testing.assert_array_equal(fit.down(one).cpu().numpy(), want)


def test_down_of_replicated_frames():
    rs = np.random.RandomState(2)
    x = rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)
    big = np.repeat(np.repeat(x, 2, axis=1), 3, axis=2)
    assert big.shape == (2, 128, 192, 3)
    np.testing.assert_array_equal(_down(big), x)


# ---------------------------------------------------------------- 3: up against float64
def _blocky(n, h, w, seed):
    """Blocks of random colour, 5 to 23 pixels a side and not aligned to the cells, with +-6 noise: the range weights span many decades."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, h, w, 3), dtype=np.int64)
    for f in range(n):
        by, bx = rs.randint(5, 24, 2)
        coarse = rs.randint(0, 256, (h // by + 2, w // bx + 2, 3))
        oy, ox = rs.randint(0, by), rs.randint(0, bx)
        out[f] = np.repeat(np.repeat(coarse, by, axis=0), bx, axis=1)[oy:oy + h, ox:ox + w]
    return np.clip(out + rs.randint(-6, 7, out.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(h, w):
    """Guide, map and the checker's low for one size: made once, shared, never written to."""
    guide = _blocky(2, h, w, 1000 * h + w)
    m = np.random.RandomState(h + w).rand(2, 64, 64).astype(np.float32)
    low = fit_ref.down_ref(guide)
    for a in (guide, m, low):
        a.setflags(write=False)
    return guide, m, low


@functools.lru_cache(maxsize=None)
def _want(h, w, sigma_s, sigma_r):
    guide, m, low = _case(h, w)
    out = fit_ref.up_ref(m, guide, low, sigma_s, sigma_r)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("sigma_s, sigma_r", SIGMAS)
@pytest.mark.parametrize("h, w", UP_SIZES)
def test_up_against_float64(h, w, sigma_s, sigma_r):
    guide, m, low = _case(h, w)
    soft = fit.up(_dev(m), _dev(guide), _dev(low), sigma_s=sigma_s, sigma_r=sigma_r).soft.cpu().numpy()
    assert soft.shape == (2, h, w) and soft.dtype == np.float32
    assert not np.isnan(soft).any() and soft.min() >= 0.0 and soft.max() <= 1.0
    err = float(np.abs(soft.astype(np.float64) - _want(h, w, sigma_s, sigma_r)).max())
    print(f"fit.up {h}x{w} sigma_s {sigma_s} sigma_r {sigma_r}: max |soft - float64| = {err:.3e}")
    assert err <= TOL
    # low=None computes the same low on the GPU
    again = fit.up(_dev(m), _dev(guide), sigma_s=sigma_s, sigma_r=sigma_r).soft.cpu().numpy()
    np.testing.assert_array_equal(again, soft)


# ---------------------------------------------------------------- 4: grey and hard follow soft exactly
@pytest.mark.parametrize("h, w", UP_SIZES)
def test_grey_and_hard_are_consistent_with_soft(h, w):
    guide, m, low = _case(h, w)
    g, l, md = _dev(guide), _dev(low), _dev(m)
    thr = float(np.float32(np.median(m)))
    r = fit.up(md, g, l, thresh=thr, want=("soft", "grey", "hard"))
    soft = r.soft.cpu().numpy()
    np.testing.assert_array_equal(r.grey.cpu().numpy(), (soft * np.float32(255.0)).astype(np.uint8))
    np.testing.assert_array_equal(r.hard.cpu().numpy(), (soft >= np.float32(thr)).astype(np.uint8))
    assert 0 < r.hard.sum().item() < soft.size
    # a threshold that some pixels hit exactly tells >= from >
    exact = float(np.sort(soft.ravel())[soft.size // 2])
    ge = fit.up(md, g, l, thresh=exact, want=("hard",))
    gt = fit.up(md, g, l, thresh=exact, inclusive=False, want=("hard",))
    assert ge.soft is None and ge.grey is None
    np.testing.assert_array_equal(ge.hard.cpu().numpy(), (soft >= np.float32(exact)).astype(np.uint8))
    np.testing.assert_array_equal(gt.hard.cpu().numpy(), (soft > np.float32(exact)).astype(np.uint8))
    assert int(ge.hard.sum()) > int(gt.hard.sum())
    only_grey = fit.up(md, g, l, want=("grey",))
    assert only_grey.soft is None and only_grey.hard is None
    np.testing.assert_array_equal(only_grey.grey.cpu().numpy(), r.grey.cpu().numpy())
    # labels: uint8 (any non-zero value) and bool give the bits of the same map as 0.0 / 1.0 floats
    lab = (m > 0.6)
    as_float = fit.up(_dev(lab.astype(np.float32)), g, l, thresh=0.5, want=("soft", "grey", "hard"))
    for labels in (_dev(lab.astype(np.uint8) * np.uint8(7)), _dev(lab)):
        as_label = fit.up(labels, g, l, thresh=0.5, want=("soft", "grey", "hard"))
        for a, b in zip(as_float, as_label):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- 5: a step edge is followed exactly
@pytest.mark.parametrize("h, w, edge, vertical", [(128, 192, 100, True), (192, 128, 100, False), (200, 330, 171, True)])
def test_edges_are_followed_exactly(h, w, edge, vertical):
    guide = np.empty((1, h, w, 3), dtype=np.uint8)
    left = (np.arange(w)[None, :] < edge) if vertical else (np.arange(h)[:, None] < edge)
    left = np.broadcast_to(left, (h, w))
    guide[0] = np.where(left[:, :, None], np.array(A, dtype=np.uint8), np.array(B, dtype=np.uint8))
    low = _down(guide)
    np.testing.assert_array_equal(low, fit_ref.down_ref(guide))
    dA = ((low.astype(np.int64) - np.array(A)) ** 2).sum(axis=-1)
    dB = ((low.astype(np.int64) - np.array(B)) ** 2).sum(axis=-1)
    m = (dA < dB).astype(np.float32)                                      # 1.0 in the cells whose colour is nearer A
    r = fit.up(_dev(m), _dev(guide), _dev(low), sigma_s=1.0, sigma_r=4.0, thresh=0.5, want=("soft", "hard"))
    soft, hard = r.soft.cpu().numpy()[0], r.hard.cpu().numpy()[0]
    assert (soft[left] == 1.0).all() and (soft[~left] == 0.0).all()
    np.testing.assert_array_equal(hard, left.astype(np.uint8))
    nearest = fit_ref.nearest_ref(m, h, w)[0]
    wrong = int(((nearest >= 0.5) != left).sum())
    print(f"edge at {edge} of {h}x{w}: nearest-cell upsampling gets {wrong} pixels wrong, the joint filter none")
    assert wrong > 0


# ---------------------------------------------------------------- 6: taps outside the grid are skipped, not clamped
def test_taps_outside_the_grid_are_skipped():
    h, w = 65, 67
    guide = np.full((1, h, w, 3), 117, dtype=np.uint8)
    low = np.full((1, 64, 64, 3), 117, dtype=np.uint8)
    m = np.zeros((1, 64, 64), dtype=np.float32)
    m[0, [0, 0, 63, 63], [0, 63, 0, 63]] = 1.0
    soft = fit.up(_dev(m), _dev(guide), _dev(low)).soft.cpu().numpy()[0].astype(np.float64)
    want = fit_ref.up_ref(m, guide, low, 1.0, 16.0)[0]
    qy, qx = fit.home_cells(h), fit.home_cells(w)
    border = ((qy < 3) | (qy > 60))[:, None] | ((qx < 3) | (qx > 60))[None, :]
    err = float(np.abs(soft - want)[border].max())
    print(f"fit.up skipped taps, 3-cell border of {h}x{w}: max |soft - float64| = {err:.3e}")
    assert err <= TOL and float(np.abs(soft - want).max()) <= TOL
    # clamping would count the corner cell up to nine times: the corner pixel's value tells the two apart by far more than TOL
    g = np.exp(-np.arange(-2, 3) ** 2 / 2.0)
    assert abs(want[0, 0] - (g[2] / g[2:].sum()) ** 2) < 2e-2 and abs((g[:3].sum() / g.sum()) ** 2 - want[0, 0]) > 0.1


def test_entry_argument_checks():
    """The C entry points refuse bad arguments before anything is launched."""
    lib = _lib.load()
    fr = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=DEV)
    mp = torch.zeros((1, 64, 64), dtype=torch.float32, device=DEV)
    so = torch.zeros((1, 64, 64), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.cgs_fit_down_u8(None, 1, 64, 64, fr.data_ptr(), st) == _lib.ERR_BADARG
    assert lib.cgs_fit_down_u8(fr.data_ptr(), 0, 64, 64, fr.data_ptr(), st) == _lib.ERR_BADARG
    assert lib.cgs_fit_down_u8(fr.data_ptr(), 1, 63, 64, fr.data_ptr(), st) == _lib.ERR_UNSUPPORTED
    assert lib.cgs_fit_down_u8(fr.data_ptr(), 1, 64, 4097, fr.data_ptr(), st) == _lib.ERR_UNSUPPORTED

    def up(map_=mp.data_ptr(), kind=_lib.FIT_MAP_F32, h=64, w=64, ss=1.0, sr=16.0, thr=0.5, soft=so.data_ptr(), hard=None):
        return lib.cgs_fit_up_joint(map_, kind, fr.data_ptr(), fr.data_ptr(), 1, h, w, ss, sr, thr, 1, soft, None, hard, st)
    assert up() == _lib.OK
    assert up(map_=None) == _lib.ERR_BADARG and up(kind=2) == _lib.ERR_BADARG
    assert up(ss=0.49) == _lib.ERR_BADARG and up(ss=float("nan")) == _lib.ERR_BADARG and up(ss=float("inf")) == _lib.ERR_BADARG
    assert up(sr=0.0) == _lib.ERR_BADARG and up(sr=float("nan")) == _lib.ERR_BADARG
    assert up(thr=float("nan"), hard=fr.data_ptr()) == _lib.ERR_BADARG
    assert up(map_=mp.data_ptr() + 1) == _lib.ERR_BADARG and up(soft=so.data_ptr() + 2) == _lib.ERR_BADARG
    assert up(h=63) == _lib.ERR_UNSUPPORTED and up(w=4097) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7: the command line, on fixture G6
@pytest.fixture()
def workdir(tmp_path, golden, g1, monkeypatch):
    """The G1 checkpoints under the names of G6, the G6 frames as S64/ and, replicated x2 per axis, as S128/."""
    from PIL import Image
    root = str(tmp_path)
    g = golden("g6_process.npz")
    for name, state in zip([str(s) for s in g["checkpoint_names"]], g1):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    frames, names = g["frames"], [str(s) for s in g["names"]]
    os.makedirs(os.path.join(root, "S64"))
    os.makedirs(os.path.join(root, "S128"))
    for nm, x in zip(names, frames):
        Image.fromarray(x).save(os.path.join(root, "S64", nm + ".png"))
        Image.fromarray(np.repeat(np.repeat(x, 2, axis=0), 2, axis=1)).save(os.path.join(root, "S128", nm + ".png"))
    monkeypatch.chdir(root)
    return root, frames, names


def _segment(argv, folder):
    H = handler.Handler(cli.parse_args(["--model", "m", "-process", "--source-imgs", folder] + argv))
    assert H.load_models()
    return H, H.segment(folder)


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_cli_process_fit(workdir):
    root, frames, names = workdir
    by_name = dict(zip(names, frames))
    order64 = [f.rsplit(".", 1)[0] for f in os.listdir("S64")]
    order = [f.rsplit(".", 1)[0] for f in os.listdir("S128")]
    _, M64 = _segment(["--mask-output-imgs", "R64"], "S64")
    plain = {s: M64[i] for i, s in enumerate(order64)}

    H, M = _segment(["-fit", "--mask-output-imgs", "R1"], "S128")
    assert M.shape == (len(names), 1, 64, 64) and M.dtype == np.float32
    for i, s in enumerate(order):                                          # the network saw exactly what plain -process shows it
        np.testing.assert_array_equal(M[i], plain[s], err_msg=s)
    assert sorted(os.listdir("R1")) == sorted([f"{s}-{k}.png" for s in names for k in ("raw-mask", "thresholded-mask")] + ["fit.json"])
    guide = _dev(np.stack([np.repeat(np.repeat(by_name[s], 2, axis=0), 2, axis=1) for s in order]))
    want = fit.up(_dev(M[:, 0]), guide, thresh=0.5, want=("grey", "hard"))
    grey, hard = want.grey.cpu().numpy(), want.hard.cpu().numpy()
    assert 0 < hard.mean() < 1
    for i, s in enumerate(order):
        raw, thr = _png(os.path.join("R1", f"{s}-raw-mask.png")), _png(os.path.join("R1", f"{s}-thresholded-mask.png"))
        assert raw.shape == thr.shape == (128, 128, 3)
        np.testing.assert_array_equal(raw, np.repeat(grey[i][:, :, None], 3, axis=2))
        np.testing.assert_array_equal(thr, np.repeat(hard[i][:, :, None], 3, axis=2) * np.uint8(255))
    with open(os.path.join("R1", "fit.json")) as fp:
        assert json.load(fp) == {"frame_size": [128, 128], "net_size": [64, 64], "sigma_spatial": 1.0, "sigma_range": 16.0, "radius": 2,
                                 "frames": len(names)}

    # other sigmas reach the kernel and the report; -concatenated: the frame, then the columns
    _, M2 = _segment(["-fit", "-concatenated", "--fit-spatial", "0.5", "--fit-range", "4", "--mask-output-imgs", "R2"], "S128")
    np.testing.assert_array_equal(M2, M)
    assert sorted(os.listdir("R2")) == sorted([f"{s}_with_mask.png" for s in names] + ["fit.json"])
    want2 = fit.up(_dev(M[:, 0]), guide, sigma_s=0.5, sigma_r=4.0, thresh=0.5, want=("grey", "hard"))
    for i, s in enumerate(order):
        strip = _png(os.path.join("R2", f"{s}_with_mask.png"))
        assert strip.shape == (128, 128 * 3, 3)
        np.testing.assert_array_equal(strip[:, :128], guide[i].cpu().numpy())
        np.testing.assert_array_equal(strip[:, 128:256, 1], want2.grey[i].cpu().numpy())
        np.testing.assert_array_equal(strip[:, 256:, 2], want2.hard[i].cpu().numpy() * np.uint8(255))
    with open(os.path.join("R2", "fit.json")) as fp:
        rep = json.load(fp)
    assert (rep["sigma_spatial"], rep["sigma_range"]) == (0.5, 4.0)

    # -crf: a third column, the CRF labels of the 64 x 64 grid brought up at 0.5; -objects keeps working in the 64 x 64 grid
    H3, M3 = _segment(["-fit", "-crf", "-concatenated", "-objects", "--mask-output-imgs", "R3"], "S128")
    np.testing.assert_array_equal(M3, M)
    low = fit.down(guide)
    labels = H3.crf(low.cpu().numpy() / 255.0, M, None)
    crf_up = fit.up(_dev(labels[:, 0]), guide, low, thresh=0.5, want=("hard",)).hard.cpu().numpy()
    for i, s in enumerate(order):
        strip = _png(os.path.join("R3", f"{s}_with_mask.png"))
        assert strip.shape == (128, 128 * 4, 3)
        np.testing.assert_array_equal(strip[:, 384:, 0], crf_up[i] * np.uint8(255))
        assert _png(os.path.join("R3", f"{s}-objects-mask.png")).shape == (64, 64, 3)
    with open(os.path.join("R3", "objects.json")) as fp:
        assert json.load(fp)["source"] == "crf-mask"
    _segment(["-fit", "-crf", "--mask-output-imgs", "R4"], "S128")
    assert sorted(os.listdir("R4")) == sorted([f"{s}-{k}.png" for s in names for k in ("raw-mask", "thresholded-mask", "crf-mask")]
                                              + ["fit.json"])
    assert all(_png(os.path.join("R4", f)).shape == (128, 128, 3) for f in os.listdir("R4") if f.endswith(".png"))

    # -fp16: the uint8 cells go to the fp16 path as the 64 x 64 files do; against the fp32 run within the fp16 path's bound on Z (2e-4)
    _, M16 = _segment(["-fit", "-fp16", "--mask-output-imgs", "R5"], "S128")
    _, P16 = _segment(["-fp16", "--mask-output-imgs", "R6"], "S64")
    for i, s in enumerate(order):
        np.testing.assert_array_equal(M16[i], P16[order64.index(s)], err_msg=s)
    d16 = float(np.abs(M16.astype(np.float64) - M).max())
    print(f"-process -fit -fp16 against fp32: |dM| max {d16:.2e}")
    assert 0 < d16 <= 2e-4


def test_cli_process_fit_refuses_mixed_sizes_and_plain_process_is_unchanged(workdir):
    from PIL import Image
    root, frames, names = workdir
    # plain -process on the 128 x 128 folder fails as it always has: a shape error out of the 64 x 64 engine
    with pytest.raises(_lib.CgsError) as plain:
        _segment(["--mask-output-imgs", "P1"], "S128")
    assert str(plain.value) == f"infer input: expected an NHWC image batch [>=0,64,64,3], got ({len(names)}, 128, 128, 3)"
    assert not os.path.exists("P1")
    # one file of another size: the ValueError names it, before any GPU work on the folder
    Image.fromarray(np.zeros((128, 130, 3), dtype=np.uint8)).save(os.path.join("S128", "zz_odd.png"))
    first = os.listdir("S128")[0]
    with pytest.raises(ValueError) as e:
        _segment(["-fit", "--mask-output-imgs", "P2"], "S128")
    named = "zz_odd.png" if first != "zz_odd.png" else os.listdir("S128")[1]
    assert named in str(e.value) and not os.path.exists("P2")
    os.remove(os.path.join("S128", "zz_odd.png"))
    Image.fromarray(np.zeros((63, 128, 3), dtype=np.uint8)).save(os.path.join("S128", "small.png"))
    os.makedirs("S63")
    os.replace(os.path.join("S128", "small.png"), os.path.join("S63", "small.png"))
    with pytest.raises(ValueError) as e:
        _segment(["-fit", "--mask-output-imgs", "P3"], "S63")
    assert "small.png" in str(e.value) and "h = 63" in str(e.value)
