"""Batched byte planes with a filter per item, the parts that need no GPU: the numpy model VF against the two models it is built
from, declarations and exports, and a bad filter id, which the calls report after the plan and before they look at a pointer.
The item pointers here are made-up device addresses: nothing dereferences them."""
import os
import re

import numpy as np
import pytest

import fplanes_batch_lib as FBL
import fplanes_lib as FL
import planes_batch_lib as BL
import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_split_fbatch_dev", "trc_planes_join_fbatch_dev", "trc_encode_fplanes_batch_dev", "trc_decode_fplanes_batch_dev")
BASE = 0x7f0000000000                                         # a made-up, 256-byte aligned device address
E_ARG = -1
ORDER = [1, 7, 8, 9, 255, 256, 257, 320, 513, 1025]            # elements per item
CHUNKS = (256, 320, 4096)


def err():
    return trc.lib().trc_last_error().decode()


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_all_none_is_the_virtual_buffer(esize):
    items = FBL.gen_items(esize, ORDER, 10 * esize)
    for chunk in CHUNKS:
        assert np.array_equal(FBL.virtual_filtered(items, [FL.NONE] * len(items), esize, chunk), BL.virtual(items, esize, chunk))


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_one_item_is_the_filter_model(esize):
    for chunk in CHUNKS:
        for i, m in enumerate(ORDER + [3 * chunk + 5]):
            item = FL.gen(FBL.KINDS[i % 2], esize, m, 0, 100 * esize + i)
            for f in FL.FILTERS:
                assert np.array_equal(FBL.virtual_filtered([item], [f], esize, chunk), FL.forward(item, esize, f, chunk)), (chunk, m, f)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_pad_is_zero_and_items_invert_alone(esize):
    items = FBL.gen_items(esize, ORDER, 20 * esize)
    sizes = [d.size for d in items]
    for chunk in CHUNKS:
        pl, first = BL.plan(sizes, esize, chunk)
        for name, filters in FBL.assignments(len(items), chunk).items():
            vf = FBL.virtual_filtered(items, filters, esize, chunk)
            assert vf.size == pl["n_virtual"], (chunk, name)
            pads = 0
            for i, n in enumerate(sizes):
                end = first[i + 1] * chunk * esize if i + 1 < len(sizes) else vf.size
                pad = vf[first[i] * chunk * esize + n:end]
                assert not pad.any(), "chunk %d %s: the pad behind item %d is not zero" % (chunk, name, i)
                pads += pad.size
                # ... and item i back from its own chunks alone
                assert np.array_equal(FBL.item_of(vf, i, sizes, filters[i], esize, chunk), items[i]), (chunk, name, i)
                if filters[i] != FL.NONE:
                    assert np.array_equal(FL.inverse(vf[first[i] * chunk * esize:end], esize, filters[i], chunk)[:n], items[i])
            assert pads == pl["pad_elems"] * esize
        # filtering V instead of the items is another thing: the pad's first element would carry the item's last
        v = FL.forward(BL.virtual(items, esize, chunk), esize, FL.ZDELTA, chunk)
        assert not np.array_equal(v, FBL.virtual_filtered(items, [FL.ZDELTA] * len(items), esize, chunk))


def test_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("planes_split_fbatch", "planes_join_fbatch", "planes_filters"):
        assert hasattr(trc, name), name


def filters_of(values):
    return trc.planes_filters(values, len(values))


def test_bad_filter_is_reported_without_a_device():
    L = trc.lib()
    esize, chunk = 2, 256
    sizes = [2 * 300, 2 * 1000, 2 * 7, 2 * 256]
    items = trc.planes_items([(BASE + 0x100000 * i, n) for i, n in enumerate(sizes)])
    pl, _ = BL.plan(sizes, esize, chunk)
    tb = L.trc_planes_batch_table_bytes(4, pl["chunks"])
    work = L.trc_planes_batch_work_bytes(trc.RCA, items, 4, esize, chunk)
    assert tb and work
    bad = filters_of([1, 0, 3, 2])
    planes, table, out = BASE + 0x1000000, BASE + 0x2000000, BASE + 0x3000000
    calls = {
        "split": lambda f: L.trc_planes_split_fbatch_dev(items, f, 4, esize, chunk, planes, pl["pitch"], table, tb, None),
        "join": lambda f: L.trc_planes_join_fbatch_dev(planes, pl["pitch"], items, f, 4, 0, 4, esize, chunk, table, tb, None),
        "encode": lambda f: L.trc_encode_fplanes_batch_dev(trc.RCA, items, f, 4, esize, chunk, None, 0, None, out, out + 0x100000, out + 0x200000,
                                                            planes, work, None),
        "decode": lambda f: L.trc_decode_fplanes_batch_dev(trc.RCA, out, out + 0x100000, items, f, 4, 0, 1, esize, chunk, None, 0, planes, work, None),
    }
    for name, call in calls.items():
        assert call(bad) == E_ARG, name
        assert re.search(r"\bitem 2\b", err()) and "filter 3" in err(), name + ": " + err()
    # every entry is validated, the last one and the ones outside a decoded range included
    assert calls["split"](filters_of([0, 0, 0, 255])) == E_ARG and re.search(r"\bitem 3\b", err())
    assert calls["decode"](filters_of([0, 0, 0, 7])) == E_ARG and re.search(r"\bitem 3\b", err())
    # the plan comes first ...
    assert L.trc_planes_split_fbatch_dev(items, bad, 4, 3, chunk, planes, pl["pitch"], table, tb, None) == E_ARG and "esize" in err()
    assert L.trc_encode_fplanes_batch_dev(trc.RCA, items, bad, 0, esize, chunk, None, 0, None, out, out, out, planes, work, None) == E_ARG and "items" in err()
    # ... and pointers and buffers after the filters: a NULL table or workspace with a bad filter is still the filter's error
    assert L.trc_planes_split_fbatch_dev(items, bad, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "filter 3" in err()
    assert L.trc_encode_fplanes_batch_dev(trc.RCA, items, bad, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "filter 3" in err()
    # with good filters the same calls get as far as their buffers
    good = filters_of([1, 0, 2, 2])
    assert L.trc_planes_split_fbatch_dev(items, good, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "aligned" in err()
    assert L.trc_encode_fplanes_batch_dev(trc.RCA, items, good, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "filter" not in err()


def test_planes_filters_helper():
    assert trc.planes_filters(None, 3) is None
    assert list(trc.planes_filters(trc.FILTER_XOR, 3)) == [2, 2, 2]
    assert list(trc.planes_filters([0, 1, 2], 3)) == [0, 1, 2]
    for bad in ([0, 1], [0, 1, 2, 0], [0, 1, 256], [0, -1, 0]):
        with pytest.raises(trc.TrcError):
            trc.planes_filters(bad, 3)
