"""Host side of the overlay video (cgs_amd.overlay) and the properties of its checker tests/overlay_ref.py.  No GPU: the kernel itself is
checked in tests/test_gpu_overlay.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import overlay_ref  # noqa: E402
from cgs_amd import _lib, build, overlay  # noqa: E402


# ---------------------------------------------------------------- the checker against hand-worked cases
def test_tint_by_hand():
    guide = np.array([[[[100, 100, 100], [0, 0, 255], [255, 255, 255], [7, 8, 9]]]], dtype=np.uint8)
    grey = np.array([[[255, 255, 0, 128]]], dtype=np.uint8)
    out = overlay_ref.compose_ref(guide, grey, None, (0, 255, 0), 128, 0, "overlay")[0, 0]
    # q = 128 x 255 = 32640 = half of 65280: (100 x 32640 + 0 + 32640) // 65280 = 50, (100 x 32640 + 255 x 32640 + 32640) // 65280 = 178
    np.testing.assert_array_equal(out[0], [50, 178, 50])
    np.testing.assert_array_equal(out[1], [0, 128, 128])              # (255 x 32640 + 32640) // 65280 = 128
    np.testing.assert_array_equal(out[2], [255, 255, 255])            # grey 0: the frame
    q = 128 * 128
    np.testing.assert_array_equal(out[3], [(7 * (65280 - q) + 32640) // 65280, (8 * (65280 - q) + 255 * q + 32640) // 65280,
                                           (9 * (65280 - q) + 32640) // 65280])
    full = overlay_ref.compose_ref(guide, grey, None, (1, 2, 3), 256, 0, "overlay")[0, 0]
    np.testing.assert_array_equal(full[0], [1, 2, 3])                 # alpha256 256 at grey 255: the colour itself
    np.testing.assert_array_equal(full[2], [255, 255, 255])
    none = overlay_ref.compose_ref(guide, grey, None, (1, 2, 3), 0, 0, "overlay")
    np.testing.assert_array_equal(none, guide)


def test_outline_by_hand():
    hard = np.zeros((1, 7, 7), dtype=np.uint8)
    hard[0, 1:6, 1:6] = 1
    one = overlay_ref.outline_ref(hard, 1)[0]
    ring = np.zeros((7, 7), dtype=bool)
    ring[1:6, 1:6] = True
    ring[2:5, 2:5] = False
    np.testing.assert_array_equal(one, ring)                          # the inner 4-neighbour boundary
    two = overlay_ref.outline_ref(hard, 2)[0]
    assert two.sum() == 24 and not two[3, 3]                          # all but the centre: Manhattan distance <= 1 of an off pixel...
    diamond = np.zeros((1, 9, 9), dtype=np.uint8)
    diamond[0, 1:8, 1:8] = 1
    got = overlay_ref.outline_ref(diamond, 2)[0]
    assert got[2, 2] and not got[3, 3] and got[2, 4] and not got[3, 4]       # ...by Manhattan, not chessboard, distance
    assert overlay_ref.outline_ref(hard, 0) is None and overlay_ref.outline_ref(None, 3) is None


def test_the_frames_edge_counts_as_on():
    on = np.ones((1, 6, 8), dtype=np.uint8)
    for t in range(1, 5):
        assert not overlay_ref.outline_ref(on, t).any()               # a full mask has no outline pixel anywhere
    half = np.zeros((1, 6, 8), dtype=np.uint8)
    half[0, :, :4] = 1                                                # a mask cut by three edges of the frame
    line = overlay_ref.outline_ref(half, 1)[0]
    want = np.zeros((6, 8), dtype=bool)
    want[:, 3] = True                                                 # only the side that faces off pixels
    np.testing.assert_array_equal(line, want)
    board = (np.add.outer(np.arange(6), np.arange(8)) & 1).astype(np.uint8)[None]
    np.testing.assert_array_equal(overlay_ref.outline_ref(board, 1), board != 0)


def test_layouts_of_the_reference():
    rs = np.random.RandomState(0)
    guide, grey = rs.randint(0, 256, (2, 4, 6, 3)).astype(np.uint8), rs.randint(0, 256, (2, 4, 6)).astype(np.uint8)
    hard = (rs.rand(2, 4, 6) > 0.5).astype(np.uint8)
    one = overlay_ref.compose_ref(guide, grey, hard, (9, 9, 9), 100, 1, "overlay")
    two = overlay_ref.compose_ref(guide, grey, hard, (9, 9, 9), 100, 1, "side")
    three = overlay_ref.compose_ref(guide, grey, hard, (9, 9, 9), 100, 1, "triple")
    assert one.shape == (2, 4, 6, 3) and two.shape == (2, 4, 12, 3) and three.shape == (2, 4, 18, 3)
    np.testing.assert_array_equal(two[:, :, :6], guide)
    np.testing.assert_array_equal(two[:, :, 6:], one)
    np.testing.assert_array_equal(three[:, :, :12], two)
    np.testing.assert_array_equal(three[:, :, 12:, 1], grey)
    edge = overlay_ref.outline_ref(hard, 1)
    assert (one[edge] == 9).all()


# ---------------------------------------------------------------- host helpers and registration
def test_parse_color():
    assert overlay.parse_color("0,255,0") == (0, 255, 0) and overlay.parse_color(" 1, 2 ,3") == (1, 2, 3)
    assert overlay.parse_color((4, 5, 6)) == (4, 5, 6)
    for bad in ("", "1,2", "1,2,3,4", "1,2,x", "256,0,0", "-1,0,0", "1.5,0,0", (1, 2), (1, 2, 3.0), 7):
        with pytest.raises(ValueError):
            overlay.parse_color(bad)


def test_alpha_outline_and_panels():
    assert [overlay.to_alpha256(a) for a in (0, 0.5, 1, 0.001, 0.999)] == [0, 128, 256, 0, 256]
    for bad in (-0.01, 1.01, float("nan"), "half", None):
        with pytest.raises(ValueError):
            overlay.to_alpha256(bad)
    assert [overlay.check_outline(t) for t in range(5)] == list(range(5))
    for bad in (-1, 5, 1.0, True):
        with pytest.raises(ValueError):
            overlay.check_outline(bad)
    assert [overlay.panels(x) for x in ("overlay", "side", "triple")] == [1, 2, 3]
    with pytest.raises(ValueError):
        overlay.panels("quad")
    assert (overlay.COLOR, overlay.ALPHA, overlay.OUTLINE, overlay.LAYOUT) == ((0, 255, 0), 0.5, 1, "overlay")


def test_registered_in_build_and_signature_table():
    assert "overlay.hip" in build.SOURCES
    assert "cgs_overlay_compose" in _lib.SIGNATURES and len(_lib.SIGNATURES["cgs_overlay_compose"][1]) == 15
    assert (_lib.OVERLAY_ONLY, _lib.OVERLAY_SIDE, _lib.OVERLAY_TRIPLE, _lib.OVERLAY_MAX_OUTLINE, _lib.OVERLAY_NONTEMPORAL) == (1, 2, 3, 4, 1)
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        header = fp.read()
    assert "int cgs_overlay_compose(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, int32_t n, int32_t h, int32_t w" in header
    assert "CGS_OVERLAY_ONLY = 1, CGS_OVERLAY_SIDE = 2, CGS_OVERLAY_TRIPLE = 3, CGS_OVERLAY_MAX_OUTLINE = 4" in header


def test_the_documents_name_the_entry_and_the_edge_convention():
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(REPO, doc)) as fp:
            assert "cgs_overlay_compose" in fp.read(), doc
    with open(os.path.join(REPO, "DESIGN.md")) as fp:
        assert "counts as on" in fp.read()


# ---------------------------------------------------------------- argument errors come before the library is touched
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_compose_argument_errors(no_library):
    guide = torch.zeros((2, 64, 70, 3), dtype=torch.uint8)
    grey = torch.zeros((2, 64, 70), dtype=torch.uint8)
    cases = [(dict(guide=guide.float()), "guide"), (dict(guide=guide[:, :63]), "guide"), (dict(grey=grey[:1]), "grey"),
             (dict(grey=grey.float()), "grey"), (dict(grey=grey.numpy()), "grey"), (dict(hard=grey.float()), "hard"),
             (dict(hard=grey[:, :, :64]), "hard"), (dict(color=(0, 0, 256)), "colour"), (dict(color="green"), "colour"),
             (dict(alpha256=257), "alpha256"), (dict(alpha256=-1), "alpha256"), (dict(alpha256=0.5), "alpha256"),
             (dict(outline=5), "outline"), (dict(outline=-1), "outline"), (dict(layout="quad"), "layout"),
             (dict(out=torch.zeros((2, 64, 70, 3), dtype=torch.uint8), layout="side"), "out")]
    for kw, word in cases:
        args = dict(guide=guide, grey=grey)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            overlay.compose(**args)
        assert word in str(e.value), (kw, str(e.value))


def test_no_cpu_path():
    with pytest.raises(_lib.CgsError):
        overlay.compose(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), torch.zeros((1, 64, 64), dtype=torch.uint8))
