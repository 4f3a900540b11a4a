"""CPU checks of the training loops' PNG sheets (main.py:203-226, 465-530): the numpy + PIL restatement tests/sheet_ref.py against
the reference's own sheets (G15, tests/golden/make_golden_sheets.py), the asynchronous writer of cgs_amd.sheets with a stand-in
composer, the file names, --visevery 0, the label rows and the C ABI entry."""
import ctypes
import json
import os
import sys
import threading

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
from cgs_amd import _lib, build, sheets, video  # noqa: E402

WAIT = 20.0           # seconds a helper thread is given before a test calls it stuck


def g15(golden):
    g = golden("g15_sheets.npz")
    g["Z"] = np.concatenate([golden(f"g15_sheets_z{k}.npz")["Z"] for k in (0, 1)])
    return g


def g15_segment_inputs(g):
    """(A, B) of step 0 of the capture, re-generated from its seed, frame indices and roll."""
    X = synthetic_frames(int(g["datasize"]) + int(g["testsize"]), int(g["data_seed"]))[0][:-int(g["testsize"])]
    return np.roll(X[g["a_frames"]], int(g["roll"]), axis=2), X[g["b_frames"]]


def g15_critic_inputs(g):
    X = synthetic_frames(int(g["critic_datasize"]) + int(g["critic_testsize"]), 9)[0][:-int(g["critic_testsize"])]
    return np.roll(X[g["critic_idx"]], int(g["critic_roll"]), axis=2)


def text_rendering_differs(g, font_name):
    """None when PIL, FreeType and the font are the capture's, else a sentence that says what differs."""
    import PIL
    from PIL import features
    here = (PIL.__version__, features.version("freetype2"), bool(features.check("raqm")), list(font_name))
    there = (str(g["pil_version"]), str(g["freetype_version"]), bool(g["raqm"]), json.loads(str(g["font"])))
    return None if here == there else f"PIL / FreeType / raqm / font {here} here, {there} in the capture: the label band is not compared"


def label_lists(g):
    return [g["Y"].tolist()] + [g[k].tolist() for k in ("pred", "negpred", "replacevalue", "injectvalue")]


# ---------------------------------------------------------------- the restatement against the reference's sheets
def test_sheet_ref_pixel_rows_equal_the_reference_segment_sheet(golden):
    g = g15(golden)
    A, B = g15_segment_inputs(g)
    got = sheet_ref.pixels(A, B, g["Z"])
    assert got.shape == (448, 4096, 3) and got.dtype == np.uint8 and not got[:128].any()
    for k, c in enumerate(g["full_columns"]):            # (diagnosis first: four image columns in full)
        np.testing.assert_array_equal(got[128:, 64 * c:64 * c + 64], g["segment_columns"][k])
    assert sheet_ref.column_hashes(got, 128) == [str(h) for h in g["segment_sha256"]]
    np.testing.assert_array_equal(got[128:192], np.concatenate(A, axis=1))          # uint8(255 * (k / 255)) == k
    np.testing.assert_array_equal(got[192:256], np.concatenate(B, axis=1))


def test_sheet_ref_label_band_equals_the_reference_segment_sheet(golden):
    g = g15(golden)
    font, _ = video.resolve_font(sheets.FONT_SIZE)
    why = text_rendering_differs(g, font.getname())
    if why:
        pytest.skip(why)
    A, B = g15_segment_inputs(g)
    got = sheet_ref.segment_sheet(A, B, g["Z"], *label_lists(g), font)
    np.testing.assert_array_equal(got[:128], g["segment_band"])
    assert got[:60].any() and not got[60:128].any()                                  # five text rows, the rest of the band black
    assert sheet_ref.column_hashes(got, 128) == [str(h) for h in g["segment_sha256"]]  # no text below the band


def test_sheet_ref_equals_the_reference_critic_sheet(golden):
    g = g15(golden)
    X = g15_critic_inputs(g)
    font, _ = video.resolve_font(sheets.FONT_SIZE)
    got = sheet_ref.critic_sheet(X, g["critic_Y"].tolist(), g["critic_pred"].tolist(), font)
    assert got.shape == (64, 64 * len(X), 3)
    frames = np.concatenate(X, axis=1)
    for rows in (slice(16, 32), slice(48, 64)):          # outside the two label bands: the frames, unconditionally
        np.testing.assert_array_equal(got[rows], frames[rows])
        for k, c in enumerate(g["full_columns"]):
            np.testing.assert_array_equal(g["critic_columns"][k][rows], frames[rows, 64 * c:64 * c + 64])
    why = text_rendering_differs(g, font.getname())
    if why:
        print(why)
        return
    np.testing.assert_array_equal(np.stack((got[0:16], got[32:48])), g["critic_bands"])
    assert sheet_ref.column_hashes(got) == [str(h) for h in g["critic_sha256"]]


def test_float32_facts_the_kernel_relies_on():
    k = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(sheet_ref.to_u8(k.astype(np.float32) / np.float32(255.0)), k)
    # evaluating the mix in another precision changes bytes: the byte-exact GPU test sees a contracted or re-ordered evaluation
    rs = np.random.RandomState(0)
    A, B = (rs.randint(0, 256, (8, 64, 64, 3)).astype(np.uint8) for _ in range(2))
    Z = rs.rand(8, 64, 64).astype(np.float32)
    a, b, z = A / 255.0, B / 255.0, Z[..., None].astype(np.float64)
    in_double = (255 * (a * (1 - z) + z * b)).astype(np.uint8)
    want = sheet_ref.pixels(A, B, Z)[256:320]
    share = float((np.concatenate(in_double, axis=1) != want).mean())
    print(f"bytes of `replaced` that differ when the mix is evaluated in float64: {share:.1e}")
    assert 0 < share < 1e-2


# ---------------------------------------------------------------- the writer: ring, order, errors
def fake_compose(A, B, Z, out=None):
    """A stand-in for the GPU composer on CPU tensors: the restatement's pixels."""
    return out.copy_(torch.from_numpy(sheet_ref.pixels(A.numpy(), B.numpy(), Z.numpy())))


def small_case(n, seed=0):
    rs = np.random.RandomState(seed)
    A, B = (torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)) for _ in range(2))
    Z = torch.from_numpy(rs.rand(n, 64, 64).astype(np.float32))
    Y = rs.rand(n)
    vals = [torch.from_numpy((rs.rand(n) * 2 - 0.5).astype(np.float32)) for _ in range(4)]
    return A, B, Z, Y, vals


class BlockedEncoder:
    def __init__(self, fail_at=None):
        self.gate, self.entered, self.paths, self.fail_at = threading.Event(), threading.Semaphore(0), [], fail_at

    def __call__(self, img, path):
        self.entered.release()
        assert self.gate.wait(WAIT)
        if self.fail_at is not None and len(self.paths) == self.fail_at:
            self.paths.append(path)
            raise OSError(f"cannot write {path}")
        self.paths.append(path)
        sheets.save_png(img, path)


def submit_in_thread(w, path, case):
    A, B, Z, Y, vals = case
    done = threading.Event()
    t = threading.Thread(target=lambda: (w.submit_segment(path, A, B, Z, Y, vals, True), done.set()), daemon=True)
    t.start()
    return t, done


@pytest.mark.parametrize("depth", [1, 3])
def test_writer_ring_blocks_only_when_every_slot_is_busy(tmp_path, depth):
    enc = BlockedEncoder()
    w = sheets.SheetWriter(depth=depth, compose=fake_compose, encode=enc)
    case = small_case(2)
    paths = [str(tmp_path / f"e0_b{k}.png") for k in range(depth + 2)]
    try:
        for k in range(depth):                           # exactly `depth` submits return while the encoder is held
            t, done = submit_in_thread(w, paths[k], case)
            assert done.wait(WAIT), f"submit {k} of {depth} blocked"
        assert enc.entered.acquire(timeout=WAIT)         # the thread holds the first sheet inside the encoder
        t, done = submit_in_thread(w, paths[depth], case)
        assert not done.wait(0.5), "a submit returned although every slot is with the writer thread"
        assert not os.listdir(tmp_path)
        enc.gate.set()                                   # releasing the encoder frees a slot: the blocked submit goes through
        assert done.wait(WAIT)
        w.submit_segment(paths[depth + 1], *case[:4], case[4], True)
    finally:
        enc.gate.set()
        w.close()
    assert enc.paths == paths == w.written               # files appear in submit order
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths)
    w.close()                                            # idempotent
    with pytest.raises(RuntimeError):
        w.submit_segment(paths[0], *case[:4], case[4], True)


def test_writer_error_surfaces_from_close_once(tmp_path):
    enc = BlockedEncoder(fail_at=1)
    enc.gate.set()
    w = sheets.SheetWriter(depth=2, compose=fake_compose, encode=enc)
    case = small_case(1)
    for k in range(4):
        w.submit_segment(str(tmp_path / f"e0_b{k}.png"), *case[:4], case[4], True)      # never raises, never hangs
    with pytest.raises(OSError, match="e0_b1.png"):
        w.close()
    w.close()                                            # the second close does nothing
    assert os.listdir(tmp_path) == ["e0_b0.png"]          # after the first failure nothing more is written


# ---------------------------------------------------------------- names, --visevery 0, label rows
def test_file_names_and_visevery():
    assert sheets.segment_path("m/segment/", 0, 0) == "m/segment/e0_b0.png"
    assert sheets.segment_path("m/critic/", 2, 300) == "m/critic/e2_b300.png"
    assert [b for b in range(7) if sheets.wanted(3, b)] == [0, 3, 6]
    assert [b for b in range(250) if sheets.wanted(100, b)] == [0, 100, 200]
    assert not any(sheets.wanted(0, b) for b in range(5))                 # this build's own meaning of --visevery 0: no sheets
    assert sheets.CRITIC_EVERY == 100 and sheets.FONT_SIZE == 10
    assert sheets.sheet_shape(64) == (448, 4096, 3) and sheets.sheet_shape(1) == (448, 64, 3)


def test_label_rows_with_and_without_inject():
    Y, p, q, r, s = ([float(k)] * 3 for k in range(5))
    assert sheets.segment_rows(Y, p, q, r, s) == [(0, Y), (12, p), (24, q), (36, r), (48, s)]
    assert sheets.segment_rows(Y, p, q, r, None) == [(0, Y), (12, p), (24, q), (36, r)]
    assert sheets.critic_rows(Y, p) == [(1, Y), (33, p)]
    assert sheets.label_text(0.12345678) == "0.123" and sheets.label_text(1.0) == "1.0" and sheets.label_text(-0.0004) == "-0.0"


@pytest.mark.parametrize("inject", [True, False])
def test_writer_files_equal_the_restatement(tmp_path, inject):
    from PIL import Image
    font, _ = video.resolve_font(sheets.FONT_SIZE)
    n = 3
    A, B, Z, Y, vals = small_case(n, seed=4)
    w = sheets.SheetWriter(depth=2, compose=fake_compose)
    X = A.numpy()
    try:
        w.submit_segment(str(tmp_path / "e0_b0.png"), A, B, Z, Y, vals if inject else vals[:3] + [None], inject)
        w.submit_critic(str(tmp_path / "c.png"), A, vals[0], vals[1])
    finally:
        w.close()
    lists = [Y.tolist()] + [v.tolist() for v in vals]
    want = sheet_ref.segment_sheet(X, B.numpy(), Z.numpy(), *lists[:4], lists[4] if inject else None, font)
    got = np.array(Image.open(tmp_path / "e0_b0.png"))
    np.testing.assert_array_equal(got, want)
    assert got[48:60].any() == inject                    # the injectvalue row is drawn only with inject
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / "c.png")), sheet_ref.critic_sheet(X, lists[1], lists[2], font))


# ---------------------------------------------------------------- C ABI
def test_sheet_entry_is_declared_built_and_validates_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert "int cgs_sheet_compose(" in text and "main.py:465-496" in text
    assert "sheet.hip" in build.SOURCES and "cgs_sheet_compose" in _lib.SIGNATURES
    assert "CGS_SHEET_ROWS = 7" in text and _lib.SHEET_ROWS == 7 and f"CGS_SHEET_MAX_N = 1 << 20" in text and _lib.SHEET_MAX_N == 1 << 20
    with open(os.path.join(REPO, "INTEGRATION.md")) as fp:
        assert "`cgs_sheet_compose`" in fp.read()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16              # a non-null, 16-byte aligned address: nothing below reaches the GPU
    call = lambda **kw: lib.cgs_sheet_compose(*[{**dict(A=p, B=p, Z=p, n=1, out=p, stream=None), **kw}[k]
                                                for k in ("A", "B", "Z", "n", "out", "stream")])
    assert call(A=None) == _lib.ERR_BADARG and call(B=None) == _lib.ERR_BADARG and call(Z=None) == _lib.ERR_BADARG
    assert call(out=None) == _lib.ERR_BADARG
    assert call(n=0) == _lib.ERR_BADARG and call(n=-3) == _lib.ERR_BADARG and call(n=(1 << 20) + 1) == _lib.ERR_BADARG
    assert call(out=p + 4) == _lib.ERR_BADARG and call(A=p + 8) == _lib.ERR_BADARG and call(B=p + 1) == _lib.ERR_BADARG
    assert call(Z=p + 2) == _lib.ERR_BADARG
    with pytest.raises(_lib.CgsError):                       # the composer has no CPU path
        sheets.compose(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64))
