"""Batched byte planes with a base per item, the parts that need no GPU: declarations and exports, the table and workspace sizes,
the order of the host-side checks (the plan, then the filters with the item's index), the model's pad, and the Python wrapper's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bplanes_lib as BP
import planes_batch_lib as BL
import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_split_bbatch_dev", "trc_planes_join_bbatch_dev", "trc_planes_bbatch_table_bytes", "trc_planes_bbatch_work_bytes",
           "trc_planes_bbatch_range_work_bytes", "trc_encode_bplanes_batch_dev", "trc_decode_bplanes_batch_dev")


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("planes_bases", "planes_split_bbatch", "planes_join_bbatch"):
        assert hasattr(trc, name), name


def test_table_and_work_bytes():
    L = trc.lib()
    for count, chunks in ((1, 1), (5, 9), (32, 32), (33, 1000), (1000, 5000)):
        assert L.trc_planes_bbatch_table_bytes(count, chunks) == L.trc_planes_batch_table_bytes(count, chunks) + BL.up256(8 * count) > 0
    assert L.trc_planes_bbatch_table_bytes(0, 5) == 0 and L.trc_planes_bbatch_table_bytes(5, 4) == 0
    items = trc.planes_items([(0x10000 * (i + 1), n) for i, n in enumerate((4096, 20, 100000))])
    for codec in (trc.RCA, trc.ANS4S):
        w = L.trc_planes_batch_work_bytes(codec, items, 3, 4, 256)
        assert L.trc_planes_bbatch_work_bytes(codec, items, 3, 4, 256) == w + 256 > 256
        r = L.trc_planes_batch_range_work_bytes(codec, items, 3, 4, 256, 1, 2)
        assert L.trc_planes_bbatch_range_work_bytes(codec, items, 3, 4, 256, 1, 2) == r + 256 > 256
        assert L.trc_planes_bbatch_work_bytes(codec, items, 3, 3, 256) == 0 and L.trc_planes_bbatch_range_work_bytes(codec, items, 3, 4, 256, 2, 2) == 0


def test_checks_come_in_order_without_a_device():
    """the plan, then the filters (the item's index in the message), then pointers: all before a device is looked for"""
    L = trc.lib()
    items = trc.planes_items([(0x10000, 4096), (0x20000, 20), (0x30000, 1000)])
    bases = trc.planes_bases([0x40000, None, 0x50008], 3)
    bad_plan = trc.planes_items([(0x10000, 4096), (0x20000, 21), (0x30000, 1000)])
    tail = (3, 4, 256, 0x100000, 4096, 0x200000, 1 << 20, None)
    jtail = (3, 0, 3, 4, 256, 0x200000, 1 << 20, None)
    f_bad = trc.planes_filters([1, 0, 3], 3)
    assert L.trc_planes_split_bbatch_dev(bad_plan, bases, f_bad, *tail) == -1 and "item 1 has 21 bytes" in err()
    assert L.trc_planes_split_bbatch_dev(items, bases, f_bad, *tail) == -1 and "item 2: filter 3" in err()
    assert L.trc_planes_join_bbatch_dev(0x100000, 4096, items, bases, f_bad, *jtail) == -1 and "item 2: filter 3" in err()
    assert L.trc_planes_split_bbatch_dev(items, bases, trc.planes_filters([1, 2, 0], 3), *tail) == -1 and "item 1" in err() and "base" in err()   # NULL
    assert L.trc_planes_split_bbatch_dev(items, bases, trc.planes_filters([1, 0, 2], 3), *tail) == -1 and "item 2" in err() and "base" in err()   # off 16
    assert L.trc_planes_split_bbatch_dev(items, None, trc.planes_filters([0, 0, 1], 3), *tail) == -1 and "item 2" in err()
    assert L.trc_planes_join_bbatch_dev(0x100000, 4096, items, bases, trc.planes_filters([1, 2, 0], 3), 3, 0, 1, 4, 256, 0x200000, 16, None) == -3  # the table


def test_model_pads_with_zeros_and_ignores_the_base_of_an_unfiltered_item():
    items, bases = BP.gen_batch(4, [5, 300, 256, 7], 3)
    filters = [1, 0, 2, 1]
    v = BP.virtual_batch(items, bases, filters, 4, 256)
    pl, first = BL.plan([d.size for d in items], 4, 256)
    assert v.size == pl["n_virtual"]
    for i, d in enumerate(items):
        g = v[first[i] * 1024:first[i] * 1024 + d.size]
        assert np.array_equal(BP.inverse(g, bases[i], 4, filters[i]), d)
        if i + 1 < len(items):
            assert not v[first[i] * 1024 + d.size:first[i + 1] * 1024].any()
    other = [b ^ 0xFF for b in bases]
    assert np.array_equal(BP.virtual_batch(items, [bases[0], other[1], bases[2], bases[3]], filters, 4, 256), v)
