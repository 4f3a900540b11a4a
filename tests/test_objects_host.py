"""CPU checks of -objects' host side: the checker of tests/objects_ref.py against scipy.ndimage.label, the CLI's refusals, table_rows,
the argument checks of cgs_amd.objects and of the entry point.  Nothing here needs a GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import objects_ref  # noqa: E402
from cgs_amd import _lib, build, cli, objects  # noqa: E402


def test_checker_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    frames = dict(objects_ref.patterns())
    rs = np.random.RandomState(1)
    frames.update({"5x7": rs.rand(5, 7) < 0.5, "37x64": rs.rand(37, 64) < 0.5, "64x33": rs.rand(64, 33) < 0.45, "1x1": np.ones((1, 1), dtype=bool)})
    for name, on in frames.items():
        for conn in (4, 8):
            want, n = ndimage.label(on, structure=np.ones((3, 3), dtype=bool) if conn == 8 else None)
            labels, kept_mask, kept, found, table = objects_ref.label_frame(on, conn, 1, max_objects=4096)
            assert kept == found == n, (name, conn)
            np.testing.assert_array_equal(labels, want, err_msg=f"{name} {conn}")
            np.testing.assert_array_equal(kept_mask, on)
            for k in range(1, n + 1):                                  # the table against scipy's numbering, object by object
                ys, xs = np.nonzero(want == k)
                first = int((ys * on.shape[1] + xs).min())
                assert table[k - 1].tolist() == [len(ys), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum(), first]
            assert not table[n:].any()


def test_checker_filter_and_cap():
    on = objects_ref.randoms()[1]
    labels1, _, kept1, found1, table1 = objects_ref.label_frame(on, 8, 1, max_objects=64)
    labels4, mask4, kept4, found4, table4 = objects_ref.label_frame(on, 8, 4, max_objects=8)
    assert (kept1, found1, kept4, found4) == (40, 40, 11, 40)
    big = [k for k in range(1, 41) if table1[k - 1, 0] >= 4]           # renumbered 1..11 in the same order
    assert len(big) == 11
    for new, old in enumerate(big, start=1):
        np.testing.assert_array_equal(labels4 == new, labels1 == old)
        if new <= 8:
            assert table4[new - 1].tolist() == table1[old - 1].tolist()
    np.testing.assert_array_equal(mask4, np.isin(labels1, big))
    assert labels4.max() == 11 and table4.shape == (8, 8)              # labels number every kept object, the table holds the first 8


def test_cli_objects_flags_parse_and_refuse():
    a = cli.parse_args([])
    assert a.objects is False and a.min_area == 1 and a.connectivity == 8
    a = cli.parse_args(["-eval", "-objects"])
    assert a.objects and a.min_area == 1 and a.connectivity == 8
    a = cli.parse_args(["-process", "-objects", "--min-area", "4", "--connectivity", "4"])
    assert (a.objects, a.min_area, a.connectivity) == (True, 4, 4)
    assert cli.parse_args(["-test", "-objects"]).eval
    assert cli.parse_args(["-process", "-crf", "-objects", "--binarymaskthreshold", "0"]).objects       # the CRF mask is binary
    for bad in (["-objects"], ["-train", "-objects"], ["-eval", "--min-area", "2"], ["-process", "--connectivity", "4"],
                ["-eval", "--min-area", "1"], ["-eval", "--connectivity", "8"],                # given, even at the default value
                ["-eval", "-objects", "--min-area", "0"], ["-eval", "-objects", "--min-area", "-3"],
                ["-eval", "-objects", "--connectivity", "6"], ["-process", "-objects", "--connectivity", "0"],
                ["-process", "-objects", "--binarymaskthreshold", "0"]):
        with pytest.raises(ValueError):
            cli.parse_args(bad)
    with pytest.raises(ValueError):
        cli.main(["-objects", "--source-imgs", "nowhere"])             # before a Handler (a GPU) is asked for


def test_table_rows():
    on = np.zeros((2, 6, 9), dtype=bool)
    on[0, 1, 2:5] = on[0, 2, 4] = True                                 # an L of 4 pixels
    on[0, 4, 8] = True
    _, _, kept, found, table = objects_ref.label(on, 8, 1, 3)
    rows = objects.table_rows(table, kept, width=9)
    assert rows == [[{"label": 1, "area": 4, "bbox": [2, 1, 4, 2], "centroid": [3.25, 1.25], "first": [2, 1]},
                     {"label": 2, "area": 1, "bbox": [8, 4, 8, 4], "centroid": [8.0, 4.0], "first": [8, 4]}], []]
    assert objects.table_rows(torch.from_numpy(table), torch.from_numpy(kept), width=9) == rows
    # more objects than rows: the rows there are
    _, _, kept, found, table = objects_ref.label(on, 8, 1, 1)
    assert kept.tolist() == [2, 0] and [len(r) for r in objects.table_rows(table, kept, width=9)] == [1, 0]
    # the default width is the project's 64
    t = np.zeros((1, 2, 8), dtype=np.int32)
    t[0, 0] = [1, 5, 3, 5, 3, 5, 3, 3 * 64 + 5]
    assert objects.table_rows(t, [1])[0][0]["first"] == [5, 3]
    for bad in ((table[0], kept), (table, kept[:1]), (np.zeros((2, 3, 7), dtype=np.int32), kept)):
        with pytest.raises(ValueError):
            objects.table_rows(*bad)


def test_label_argument_errors():
    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    for bad in (dict(connectivity=6), dict(min_area=0), dict(max_objects=0), dict(min_area=1.5), dict(thresh=0.5)):
        with pytest.raises(ValueError):
            objects.label(m, **bad)
    with pytest.raises(ValueError):
        objects.label(m.float())                                       # a float mask without thresh
    with pytest.raises(ValueError):
        objects.label(m.float(), thresh=float("nan"))
    with pytest.raises(ValueError):
        objects.label(m.double(), thresh=0.5)
    with pytest.raises(ValueError):
        objects.label(m.to(torch.int32))
    for shape in ((8,), (1, 2, 8, 8), (2, 65, 8), (2, 8, 65), (0, 8, 8), (2, 0, 8)):
        with pytest.raises(ValueError):
            objects.label(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        objects.label(np.zeros((2, 8, 8), dtype=bool))


def test_no_cpu_path():
    """A tensor in host memory: CgsError, with or without a GPU in the machine."""
    with pytest.raises(_lib.CgsError):
        objects.label(torch.zeros(2, 8, 8, dtype=torch.bool))
    with pytest.raises(_lib.CgsError):
        objects.label(torch.rand(8, 8), thresh=0.5, inclusive=True)


def test_objects_entry_point_is_declared_and_checks_its_arguments():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_objects_label\s*\(", text)
    assert "objects.hip" in build.SOURCES and "cgs_objects_label" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cgs_abi_version() == 1
    # argument checks come before anything is launched: safe without a GPU (the pointers are never followed)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    ok = dict(src=p, kind=0, thresh=0.0, n=1, h=4, w=4, conn=8, min_area=1, max_objects=1, labels=None, mask=None, count=p, table=None)

    def call(**kw):
        a = {**ok, **kw}
        return lib.cgs_objects_label(a["src"], a["kind"], a["thresh"], a["n"], a["h"], a["w"], a["conn"], a["min_area"], a["max_objects"],
                                     a["labels"], a["mask"], a["count"], a["table"], None)

    for bad in (dict(src=None), dict(count=None), dict(n=0), dict(h=0), dict(w=-1), dict(kind=3), dict(kind=-1), dict(conn=6), dict(conn=0),
                dict(min_area=0), dict(max_objects=0), dict(max_objects=-5)):
        assert call(**bad) == _lib.ERR_BADARG, bad
    assert lib.cgs_objects_label(None, 0, 0.0, 1, 4, 4, 8, 1, 1, None, None, None, None, None) == _lib.ERR_BADARG
    assert call(h=65) == _lib.ERR_UNSUPPORTED and call(w=65) == _lib.ERR_UNSUPPORTED and call(h=65, w=4096) == _lib.ERR_UNSUPPORTED
    assert call(h=65, conn=6) == _lib.ERR_BADARG                      # a bad argument is reported before an unsupported size
