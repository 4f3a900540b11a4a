"""The -viscritic / -vismasker videos on the GPU (cgs_vis_compose / cgs_amd.vis / the CLI) against the numpy + PIL restatement
tests/vis_ref.py and against the reference's own videos (G14, tests/golden/make_golden_vis.py)."""
import gzip
import hashlib
import io
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

import vis_ref  # noqa: E402
from loop_inputs import synthetic_eval_set, synthetic_frames  # noqa: E402
from cgs_amd import cli, video, vis  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_text_rendering(g):
    import PIL
    from PIL import features
    here = (PIL.__version__, features.version("freetype2"), bool(features.check("raqm")))
    there = (str(g["pil_version"]), str(g["freetype_version"]), bool(g["raqm"]))
    if here != there:
        print(f"label rectangles blanked on both sides: PIL / FreeType / raqm {here} here, {there} in the capture")
    return here == there


# ---------------------------------------------------------------- kernel vs restatement
def _edge_masks(rs, n):
    """fp32 [n,64,64] in [0, 1] that put many products x m on and next to integers: k / 255 exactly (in fp32), nextafter on both sides,
    0, 1 and uniform values."""
    k = rs.randint(0, 256, (n, 64, 64))
    exact = (k / 255.0).astype(np.float32)
    side = rs.randint(0, 3, (n, 64, 64))
    v = np.where(side == 1, np.nextafter(exact, np.float32(0)), np.where(side == 2, np.nextafter(exact, np.float32(1)), exact))
    v = np.where(rs.rand(n, 64, 64) < 0.2, rs.rand(n, 64, 64).astype(np.float32), v)
    v[:, :2] = 0
    v[:, 2:4] = 1
    return np.clip(v, 0, 1).astype(np.float32)


N_KERNEL = 150            # the plot windows clip at both ends (j < 32, j > N - 32) and are full in the middle


def _case(seed):
    rs = np.random.RandomState(seed)
    n = N_KERNEL
    X = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    X[:, 4:8] = 255                                                       # 255 x m with m next to k / 255
    values = np.stack((rs.rand(n), rs.randn(n) * 3))                      # many distinct labels, negative ones among them
    values[0, :5] = values[0].max()                                       # ties
    strings = vis.label_strings(values, n)
    for p in range(0, n, 7):                                              # 5-digit index labels: clipped at the right frame edge
        strings[p][0] = str(12345 + p)
    return X, _edge_masks(rs, n), values, strings


def _composer(X, masks, values, perm, strings):
    atlas, ids, _ = vis.pack_labels(strings)
    tables = vis.Tables(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (vis.plot_rows(values), ids, atlas)))
    return vis.Composer(X, masks, values, perm, tables=tables)


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("nontemporal", [False, True])
@pytest.mark.parametrize("permuted", [False, True])
def test_compose_bit_exact_vs_restatement(R, nontemporal, permuted):
    X, masks, values, strings = _case(11 + R)
    masks = masks if R == 2 else None
    perm = np.random.RandomState(3).permutation(N_KERNEL) if permuted else None
    want = vis_ref.frames(X, masks, values, perm, strings=strings)
    p = vis.plan(R == 2)
    assert want.shape == (N_KERNEL, p.height, p.width, 3) == (N_KERNEL, 4 * (64 * R + 64), 256, 3)
    from PIL import Image, ImageDraw
    clipped = ImageDraw.Draw(Image.new("RGB", (8, 8))).textbbox((vis_ref.label_positions(p.height)[0][0], 0), "12345")[2]
    assert clipped > 256, "the 5-digit index label does not reach the frame edge"
    comp = _composer(X, masks, values, perm, strings)
    assert comp.n == N_KERNEL and comp.frame_shape == want.shape[1:]
    got = comp.compose(0, N_KERNEL, nontemporal=nontemporal).cpu().numpy()
    bad = np.flatnonzero((got != want).reshape(N_KERNEL, -1).any(axis=1))
    print(f"R={R} nontemporal={nontemporal} permuted={permuted}: {int((got != want).sum())} differing bytes, frames {bad[:10].tolist()}")
    np.testing.assert_array_equal(got, want)
    # one frame from the middle of the stack, and ragged chunks through the pinned double buffer (21 x 7 + 3)
    np.testing.assert_array_equal(comp.compose(77, 1, nontemporal=nontemporal).cpu().numpy()[0], want[77])
    if nontemporal == vis.NONTEMPORAL:
        sink = io.BytesIO()
        assert video.stream_frames(comp, sink, chunk=7) == want.nbytes
        np.testing.assert_array_equal(np.frombuffer(sink.getvalue(), np.uint8).reshape(want.shape), want)


def test_default_tables_device_sources_and_argument_checks():
    X, masks, values, _ = _case(5)
    n = 40
    X, masks, values = X[:n], masks[:n], values[:, :n]
    perm = np.argsort(values[1])[::-1]
    want = vis_ref.frames(X, masks, values, perm)
    comp = vis.Composer(torch.from_numpy(X).cuda(), torch.from_numpy(masks).cuda()[:, None], values, perm)      # masks as [N,1,64,64]
    np.testing.assert_array_equal(comp.compose(0, n).cpu().numpy(), want)
    with pytest.raises(ValueError):
        comp.compose(n - 1, 2)                                   # past the end
    with pytest.raises(ValueError):
        vis.Composer(X, masks, values, np.zeros(n, np.int64))    # not a permutation
    with pytest.raises(ValueError):
        vis.Composer(X, masks[:-1], values)
    with pytest.raises(ValueError):
        vis.Composer(X.astype(np.float32), None, values)


# ---------------------------------------------------------------- the composer on the reference's recorded arrays
def test_composer_reproduces_the_reference_videos(golden):
    g = golden("g14_vis.npz")
    n = int(g["n"])
    X = synthetic_frames(int(g["datasize"]) + n, int(g["data_seed"]))[0][-n:]
    exact = _same_text_rendering(g)
    view = (lambda a: a) if exact else vis_ref.blank_labels
    for k, sorting in enumerate((None, g["sorting_pred"], g["sorting_gt"])):
        got = vis.Composer(X, g["masks"], g["values"], sorting).compose(0, n).cpu().numpy()
        ref = g["vismasker_frames"][k]
        print(f"-vismasker video {k}: {int((view(got) != view(ref)).sum())} differing bytes")
        np.testing.assert_array_equal(view(got), view(ref))
        crit = vis.Composer(X, None, g["values"], sorting).compose(0, n).cpu().numpy()
        if exact:
            assert [hashlib.sha256(f.tobytes()).hexdigest() for f in crit] == [str(h) for h in g["viscritic_sha256"][k]]
        else:       # as tests/test_vis_host.py: the -vismasker frame without its second tile
            cut = np.concatenate((ref[:, :256], ref[:, 512:]), axis=1)
            np.testing.assert_array_equal(vis_ref.blank_labels(crit), vis_ref.blank_labels(cut))


# ---------------------------------------------------------------- the CLI, end to end
STUB = """#!{python}
import os, shutil, sys
out = {out!r}
n = len([f for f in os.listdir(out) if f.endswith(".argv")])
with open(os.path.join(out, f"{{n}}.argv"), "w") as fp:
    fp.write("\\n".join(sys.argv))
with open(os.path.join(out, f"{{n}}.stdin"), "wb") as fp:
    shutil.copyfileobj(sys.stdin.buffer, fp)
"""


def _stub_ffmpeg(root):
    """A test-written `ffmpeg` first on PATH: it saves its argv and everything on stdin under root/ffmpeg_calls/."""
    bindir, calls = os.path.join(root, "bin"), os.path.join(root, "ffmpeg_calls")
    os.makedirs(bindir)
    os.makedirs(calls)
    exe = os.path.join(bindir, "ffmpeg")
    with open(exe, "w") as fp:
        fp.write(STUB.format(python=sys.executable, out=calls))
    os.chmod(exe, 0o755)
    return bindir, calls


def _run_cli(root, argv, g, g1):
    """The capture's command line in-process with the stub ffmpeg: (what write_videos was given, the sortings, the ffmpeg calls)."""
    pc, pm = g1
    n, datasize = int(g["n"]), int(g["datasize"])
    for name, state in zip((str(s) for s in g["checkpoint_names"]), (pc, pm)):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        torch.save(state, os.path.join(root, name))
    os.makedirs(os.path.join(root, "runs/data/straight"))
    with gzip.GzipFile(os.path.join(root, f"runs/data/straight/Treechop-trunk-{datasize}-[0.98-0.97-0.96-0.95].pickle"), "wb") as fp:
        pickle.dump(synthetic_frames(datasize + n, int(g["data_seed"])), fp)
    bindir, calls = _stub_ffmpeg(root)
    mp = pytest.MonkeyPatch()
    seen, sorts = [], []
    real_write, real_sortings = vis.write_videos, vis.sortings

    def spy_write(resultdir, visname, sortidx, X, masks, values, *a, **k):
        seen.append({"resultdir": resultdir, "X": np.array(X, copy=True), "masks": None if masks is None else np.array(masks, copy=True),
                     "values": np.array(values, copy=True)})
        return real_write(resultdir, visname, sortidx, X, masks, values, *a, **k)

    def spy_sortings(values, sortidx):
        out = real_sortings(values, sortidx)
        sorts.append(out)
        return out
    try:
        mp.chdir(root)
        mp.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
        mp.setattr(vis, "write_videos", spy_write)
        mp.setattr(vis, "sortings", spy_sortings)
        cli.main(argv)
    finally:
        mp.undo()
    assert len(seen) == 1 and len(sorts) == 1
    videos = []
    for k in range(len(os.listdir(calls)) // 2):
        with open(os.path.join(calls, f"{k}.argv")) as fp:
            a = fp.read().split("\n")
        with open(os.path.join(calls, f"{k}.stdin"), "rb") as fp:
            videos.append((a, fp.read()))
    return seen[0], sorts[0], videos


@pytest.fixture(scope="module", params=["vismasker", "viscritic"])
def cli_run(request, tmp_path_factory, golden, g1):
    g = golden("g14_vis.npz")
    argv = json.loads(str(g[f"argv_{request.param}_json"]))
    root = str(tmp_path_factory.mktemp(request.param))
    src, sorts, videos = _run_cli(root, argv, g, g1)
    return {"g": g, "R": 2 if request.param == "vismasker" else 1, "src": src, "sorts": sorts, "videos": videos, "root": root,
            "recs": json.loads(str(g[f"{request.param}_ffmpeg_json"]))}


def _streams(run):
    n, H = int(run["g"]["n"]), 4 * (64 * run["R"] + 64)
    out = []
    for argv, raw in run["videos"]:
        assert len(raw) == n * H * 256 * 3
        out.append(np.frombuffer(raw, np.uint8).reshape(n, H, 256, 3))
    return out


def test_cli_writes_the_three_videos_in_the_reference_order(cli_run):
    g, R, src = cli_run["g"], cli_run["R"], cli_run["src"]
    n, H = int(g["n"]), 4 * (64 * R + 64)
    assert len(cli_run["videos"]) == 3 and [s for s, _ in cli_run["sorts"]] == ["", "-pred-sorted", "-GT-sorted"]
    assert (src["masks"] is not None) == (R == 2) and src["X"].shape == (n, 64, 64, 3) and src["values"].shape == (2, n)
    assert src["values"].dtype == np.float64
    for (argv, raw), rec in zip(cli_run["videos"], cli_run["recs"]):
        pairs = set(zip(argv, argv[1:]))
        i = argv.index("-i")
        assert argv[i + 1:].count(rec["file"]) == 1                                  # m/curves.mp4, -pred-sorted, -GT-sorted
        assert ("-s", f"256x{H}") in pairs and ("-s", rec["input"]["s"]) in pairs
        assert argv[:i].count("-r") == 1 and argv[i:].count("-r") == 1 and pairs >= {("-r", "4")}
        assert len(raw) == n * H * 256 * 3                                           # n frames
    assert os.path.isdir(os.path.join(cli_run["root"], "m"))
    # every stream is the restatement of the arrays the handler itself produced
    for stream, (suffix, perm) in zip(_streams(cli_run), cli_run["sorts"]):
        want = vis_ref.frames(src["X"], src["masks"], src["values"], perm)
        print(f"R={R} video '{suffix}': {int((stream != want).sum())} differing bytes")
        np.testing.assert_array_equal(stream, want)


def test_cli_unsorted_video_vs_reference_capture(cli_run):
    g, R, src = cli_run["g"], cli_run["R"], cli_run["src"]
    n = int(g["n"])
    ref = g["vismasker_frames"][0]
    if R == 1:                                  # the -viscritic frame: the -vismasker frame without its second tile (hashes only stored)
        ref = np.concatenate((ref[:, :256], ref[:, 512:]), axis=1)
    got = _streams(cli_run)[0]
    assert got.shape == ref.shape
    np.testing.assert_array_equal(src["values"][0], g["values"][0])                  # the ground truth comes from the data
    print("max |pred - reference pred|", np.abs(src["values"][1] - g["values"][1]).max())
    exact = _same_text_rendering(g)
    if not exact:
        got, ref = vis_ref.blank_labels(got), vis_ref.blank_labels(ref)
    (ix, iy), (gx, gy), (px, py) = vis_ref.label_positions(got.shape[1])
    if R == 1:      # the index label sits 256 rows higher than in the frame the reference rows were cut from: its rectangle holds the
        got, ref = got.copy(), ref.copy()           # label here and the last three rows of the other one there -- not comparable
        for a in (got, ref):
            a[:, iy:iy + vis_ref.CELL_H, ix:] = 0
    # the prediction label may legitimately differ (predictions within 1e-3 of the reference's, rounded to 3 digits): it is compared
    # when both sides print the same string
    same_pred = all(vis_ref.label_strings(src["values"], p)[2] == vis_ref.label_strings(g["values"], p)[2] for p in range(n))
    rgb_got, rgb_ref = got[:, :256].copy(), ref[:, :256].copy()
    if not same_pred:
        print("prediction label strings differ from the capture's: its rectangle is not compared")
        for a in (rgb_got, rgb_ref):
            a[:, py:py + vis_ref.CELL_H, px:px + vis_ref.CELL_W] = 0
    np.testing.assert_array_equal(rgb_got, rgb_ref)                                  # the RGB tile, the ground-truth label on it
    np.testing.assert_array_equal(got[:, gy:py, gx:gx + vis_ref.CELL_W], ref[:, gy:py, gx:gx + vis_ref.CELL_W])
    top = 256 * R
    np.testing.assert_array_equal(got[:, top:top + 128], ref[:, top:top + 128])      # the ground-truth plot strip
    if R == 2:
        # masks within 1e-3 of the reference's by this project's contract: |x dm| <= 0.255 < 1 before truncation
        d = np.abs(got[:, 256:512].astype(np.int32) - ref[:, 256:512].astype(np.int32))
        print("masked tile: max |difference|", d.max(), "differing bytes", int((d > 0).sum()))
        assert d.max() <= 1


def test_cli_sorted_orders(cli_run):
    g, src = cli_run["g"], cli_run["src"]
    n = int(g["n"])
    (_, none), (_, pred), (_, gt) = cli_run["sorts"]
    assert none is None
    for perm, row in ((pred, 1), (gt, 0)):
        assert sorted(perm.tolist()) == list(range(n))
        assert (np.diff(src["values"][row][perm]) <= 0).all()                        # non-increasing
    assert len(set(g["values"][0].tolist())) == n                                    # no ties in the ground truth
    np.testing.assert_array_equal(gt, g["sorting_gt"])
    # prediction order: pairs the reference's predictions separate by more than 2e-3 keep their recorded order (ties and near-ties
    # are never compared)
    rank_here, rank_ref = np.argsort(pred), np.argsort(g["sorting_pred"])
    rp = g["values"][1]
    checked = 0
    for a in range(n):
        for b in range(n):
            if rp[a] - rp[b] > 2e-3:
                checked += 1
                assert rank_ref[a] < rank_ref[b] and rank_here[a] < rank_here[b]
    print("prediction pairs further apart than 2e-3:", checked)


def test_plain_eval_still_starts_no_ffmpeg(tmp_path, golden, g1, monkeypatch):
    root = str(tmp_path)
    pc, pm = g1
    for c, state in zip((str(s) for s in golden("g6_process.npz")["checkpoint_names"]), (pc, pm)):
        os.makedirs(os.path.dirname(os.path.join(root, c)), exist_ok=True)
        torch.save(state, os.path.join(root, c))
    g13 = golden("g13_test_video.npz")
    X, Yrgb = synthetic_eval_set(int(g13["n_set"]), int(g13["data_seed"]))
    os.makedirs(os.path.join(root, "red-trees"))
    np.save(os.path.join(root, "red-trees", "X.npy"), X)
    np.save(os.path.join(root, "red-trees", "Y.npy"), Yrgb)
    bindir, calls = _stub_ffmpeg(root)
    monkeypatch.chdir(root)
    monkeypatch.setenv("PATH", bindir + os.pathsep + os.environ.get("PATH", ""))
    cli.main(["-eval", "--model", "m"])
    assert os.listdir(calls) == []
    assert not [f for f in os.listdir(os.path.join(root, "m")) if f.endswith(".mp4")]
