"""The LDS bank model (tools/lds_banks.py) on the staging stores and the patch reads of features.0's sparse weight gradient
(csrc/wgrad_sparse.h).  CPU only: the model is the instruction table of the hardware guide, applied to the kernel's addresses."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import lds_banks as lb  # noqa: E402


def test_instruction_table_basics():
    lin = list(range(64))
    assert lb.cycles("ds_read_b32", lin) == (2, 2)
    assert lb.cycles("ds_read_b64", [2 * a for a in lin]) == (2, 2)
    assert lb.cycles("ds_read_b128", [4 * a for a in lin]) == (4, 4)
    assert lb.cycles("ds_write_b32", lin) == (2, 2)
    assert lb.cycles("ds_write_b64", [2 * a for a in lin]) == (4, 4)
    assert lb.cycles("ds_write_b128", [4 * a for a in lin]) == (8, 8)
    assert lb.cycles("ds_read_b32", [7] * 64) == (2, 2)                         # identical dwords broadcast
    assert lb.cycles("ds_read_b32", [32 * a for a in lin]) == (64, 2)           # one bank, 32 dwords per group
    assert lb.cycles("ds_write_b64", [4 * a for a in lin]) == (8, 4)            # 16-byte pitch: 8 bank pairs for 16 lanes
    assert lb.cycles("ds_write_b32", [None] * 32 + lin[:32]) == (1, 1)          # an empty group costs nothing


def test_grouped_staging_stores_were_an_8_way_conflict():
    """The finding: four pixels per thread put the 16 lanes of a ds_write_b64 group 16 dwords apart."""
    assert lb.total_cycles(lb.enc0_stores_grouped()) == (640, 80)


def test_shipped_staging_stores():
    t, free = lb.total_cycles(lb.enc0_stores("swap"))
    assert free == 80
    assert t <= 2 * free
    assert t == 80                                                              # the swapped halves cover the 32 banks once
    assert lb.total_cycles(lb.enc0_stores("b64+b64")) == (160, 80)              # one pixel per lane alone: 2-way


def test_every_pixel_slot_is_stored_once():
    for form in ("swap", "b64+b64"):
        seen = {}
        for instr, addrs in lb.enc0_stores(form):
            for a in addrs:
                if a is not None:
                    for k in range(2):
                        seen[a + k] = seen.get(a + k, 0) + 1
        want = {r * lb.ENC0_RS + 4 * (x + 1) + k for r in range(lb.ENC0_TRA) for x in range(lb.ENC0_W) for k in range(4)}
        assert set(seen) == want and set(seen.values()) == {1}


def test_patch_reads_of_the_3x3_kernels_are_2_way():
    """read_patch_a with Geo::pc / Geo::PWA as shipped (csrc/conv_tile.h): recorded, not fixed."""
    assert lb.geo_pwa(64) == 70 and lb.geo_pwa(32) == 36
    assert lb.total_cycles(lb.patch_reads(64, 256)) == (512, 256)
    assert lb.total_cycles(lb.patch_reads(32, 128)) == (320, 128)
    assert lb.total_cycles(lb.patch_reads(32, 128, pwa=40)) == (192, 128)
    pc3 = lambda c: c + (c >> 1)
    assert lb.total_cycles(lb.patch_reads(64, 256, pc3, pc3(65) + 1)) == (256, 256)


@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_reads_conflict_free_uniform_positions(p):
    assert lb.total_cycles(lb.enc0_reads(lambda k, cx, co: p)) == (576, 576)


def test_reads_conflict_free_random_positions():
    for seed in range(200):
        assert lb.total_cycles(lb.enc0_reads(lb.random_positions(seed))) == (576, 576), seed
