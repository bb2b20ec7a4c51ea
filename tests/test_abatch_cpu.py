"""The batch advisor, the parts that need no GPU: trc_planes_advise_batch on the numpy model's histograms of a mixed batch against
advise_lib item by item, its failures, and the two size functions.  The item pointers here are made-up device addresses: nothing
dereferences them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abatch_lib as ABL
import advise_lib as AL
import fplanes_lib as FL
import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_hist_batch_bytes", "trc_planes_hist_batch_dev", "trc_planes_advise_batch", "trc_planes_advise_batch_work_bytes",
           "trc_planes_advise_batch_dev")
BASE = 0x7f0000000000                                         # a made-up, 256-byte aligned device address
E_ARG = -1
CHUNK = 256
MIXED = (("weights", 4105), ("monotone", 2049), ("bitflip", 5220), ("random", 4105), ("walk", 300), ("wrap", 1), ("random", 7), ("monotone", 257))
SLAB = 8 << 20
_cache = {}


def err():
    return trc.lib().trc_last_error().decode()


def batch(esize):
    """-> (items as the library takes them, elements per item, model histograms [count, 3, esize, 256]): computed once, left unchanged"""
    if esize not in _cache:
        datas = [AL.gen(kind, esize, m, 0, 31 * esize + 7 + i) for i, (kind, m) in enumerate(MIXED)]
        h = ABL.hist(datas, esize, CHUNK, AL.ALL)
        h.setflags(write=False)
        _cache[esize] = ([d.size for d in datas], [m for _, m in MIXED], h)
    sizes, ms, h = _cache[esize]
    return trc.planes_items([(None, n) for n in sizes]), ms, h          # (the host function looks at no pointer)


def test_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("planes_hist_batch_bytes", "planes_hist_batch", "planes_advise_batch", "planes_advise_batch_dev"):
        assert hasattr(trc, name), name


@pytest.mark.parametrize("filters", (7, 3, 5, 6, 1, 2, 4))
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_advice_per_item_is_the_single_advisor(esize, filters):
    items, ms, h = batch(esize)
    hf = ABL.masked(h, filters)
    want = ABL.advise(hf, filters, esize, ms)
    if filters == 7:
        assert [w[0] for w in want[:4]] == [FL.NONE, FL.ZDELTA, FL.XOR, FL.NONE], "the model itself"
    got, advice = trc.planes_advise_batch(hf, filters, esize, items, len(ms))
    ABL.assert_advice(got, advice, want, filters, esize, ms, "esize %d filters %d" % (esize, filters))
    for i, a in enumerate(advice):                             # ... and field for field what the unbatched call returns
        one = trc.planes_advise(hf[i], filters, esize, ms[i])
        assert all(np.array_equal(a[k], one[k]) for k in one), i
    # advice = NULL
    got, none = trc.planes_advise_batch(hf, filters, esize, items, len(ms), advice=False)
    assert none is None and got == [w[0] for w in want]


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_a_bad_row_names_its_item_and_writes_no_choice(esize):
    items, ms, h = batch(esize)
    count = len(ms)
    L = trc.lib()
    out = (C.c_uint8 * count)(*([0xEE] * count))
    for i, f, k in ((0, 0, 0), (3, 1, esize - 1), (count - 1, 2, 1)):
        bad = h.copy()
        b = int(np.argmax(bad[i, f, k]))
        bad[i, f, k, b] -= 1                                   # the row sums to m[i] - 1
        assert L.trc_planes_advise_batch(bad.ctypes.data, 7, esize, items, count, out, None) == E_ARG
        assert re.search(r"\bitem %d\b" % i, err()), err()
        assert list(out) == [0xEE] * count, "a failed call wrote to filters_out"
        bad[i, f, k, b] += 2                                   # ... to m[i] + 1
        assert L.trc_planes_advise_batch(bad.ctypes.data, 7, esize, items, count, out, None) == E_ARG and re.search(r"\bitem %d\b" % i, err())
        assert list(out) == [0xEE] * count
        if f:                                                  # the row is not looked at where its filter is not requested
            assert L.trc_planes_advise_batch(bad.ctypes.data, 1, esize, items, count, out, None) == 0 and list(out) == [0] * count
            out = (C.c_uint8 * count)(*([0xEE] * count))
    # an item that is no whole number of elements
    sizes = [m * esize for m in ms]
    sizes[2] += 1
    assert L.trc_planes_advise_batch(h.ctypes.data, 7, esize, trc.planes_items([(None, n) for n in sizes]), count, out, None) == E_ARG
    assert re.search(r"\bitem 2\b", err()) and list(out) == [0xEE] * count


def test_argument_errors():
    esize = 4
    items, ms, h = batch(esize)
    count = len(ms)
    L = trc.lib()
    out = (C.c_uint8 * count)(*([0xEE] * count))
    adv = (trc.PlanesAdvice * count)()
    assert L.trc_planes_advise_batch(h.ctypes.data, 7, esize, items, count, out, adv) == 0 and list(out)[:4] == [0, 1, 2, 0]
    out = (C.c_uint8 * count)(*([0xEE] * count))
    for bad_esize in (0, 1, 3, 16):
        assert L.trc_planes_advise_batch(h.ctypes.data, 7, bad_esize, items, count, out, adv) == E_ARG and "esize" in err()
    for filters in (0, 8, 15):
        assert L.trc_planes_advise_batch(h.ctypes.data, filters, esize, items, count, out, adv) == E_ARG and "filters" in err()
    assert L.trc_planes_advise_batch(h.ctypes.data, 7, esize, items, 0, out, adv) == E_ARG and "items" in err()
    assert L.trc_planes_advise_batch(None, 7, esize, items, count, out, adv) == E_ARG
    assert L.trc_planes_advise_batch(h.ctypes.data, 7, esize, items, count, None, adv) == E_ARG
    assert list(out) == [0xEE] * count
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_advise_batch(h, 7, 3, items, count)


def test_hist_batch_bytes():
    for esize in FL.ESIZES:
        assert [trc.planes_hist_batch_bytes(c, esize) for c in (1, 5, 400, 1 << 20)] == [c * 3 * esize * 256 * 8 for c in (1, 5, 400, 1 << 20)]
        assert trc.planes_hist_batch_bytes(1, esize) == trc.planes_hist_bytes(esize)
        assert trc.planes_hist_batch_bytes(0, esize) == 0
    assert [trc.planes_hist_batch_bytes(3, e) for e in (0, 1, 3, 16)] == [0, 0, 0, 0]


def fake_items(count, n):
    return trc.planes_items([(BASE + 0x100000 * i, n) for i in range(count)])


def test_advise_batch_work_bytes(monkeypatch):
    L = trc.lib()
    monkeypatch.delenv("TRC_PLANES_ADVISE_SLAB_ITEMS", raising=False)
    work = L.trc_planes_advise_batch_work_bytes
    for esize in FL.ESIZES:
        n = 1000 * esize                                       # 4 chunks of 256 per item
        slab = SLAB // trc.planes_hist_bytes(esize)            # 682 / 341 / 170 items
        small, full, large = work(fake_items(10, n), 10, esize, CHUNK), work(fake_items(1000, n), 1000, esize, CHUNK), work(fake_items(10000, n), 10000, esize, CHUNK)
        assert small == SLAB + L.trc_planes_batch_table_bytes(10, 40)
        assert full == large == SLAB + L.trc_planes_batch_table_bytes(slab, 4 * slab), "the workspace grows with count beyond a full slab"
        # what the plan rejects
        assert work(fake_items(10, n), 0, esize, CHUNK) == 0 and work(fake_items(10, n), 10, esize, 100) == 0
        assert work(fake_items(10, n + 1), 10, esize, CHUNK) == 0 and work(fake_items(10, 0), 10, esize, CHUNK) == 0
    assert work(fake_items(10, 1000), 10, 3, CHUNK) == 0
    # ... and, as the other work-bytes functions, a pointer the call would reject
    items = fake_items(10, 1000)
    items[4].d_ptr = BASE + 8
    assert work(items, 10, 2, CHUNK) == 0
    items[4].d_ptr = None
    assert work(items, 10, 2, CHUNK) == 0
    # the test aid: 5 items per slab -- 10 items and 10 000 items need the same
    monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", "5")
    assert work(fake_items(10, 4000), 10, 4, CHUNK) == work(fake_items(10000, 4000), 10000, 4, CHUNK) == SLAB + L.trc_planes_batch_table_bytes(5, 20)


def test_the_device_calls_check_the_plan_and_the_filters_first():
    """the order of the checks, as far as it shows without a device: the plan, then the bit set, then the range, then pointers"""
    L = trc.lib()
    esize = 2
    items = fake_items(4, 600)
    hist, table = BASE + 0x1000000, BASE + 0x2000000
    tb = L.trc_planes_batch_table_bytes(4, 8)

    def call(filters=7, count=4, fi=0, ic=4, esize=esize, chunk=CHUNK, items=items, hist=hist, table=table, tb=tb):
        return L.trc_planes_hist_batch_dev(filters, items, count, fi, ic, esize, chunk, hist, table, tb, None)
    assert call(filters=0, esize=3) == E_ARG and "esize" in err()
    assert call(filters=8, chunk=100) == E_ARG and "chunk" in err()
    assert call(filters=8, fi=3, ic=2, hist=None) == E_ARG and "filters" in err()
    assert call(fi=3, ic=2, hist=None) == E_ARG and "items [3" in err()
    assert call(fi=5, ic=0) == E_ARG
    assert call(fi=4, ic=0, hist=None, table=None, tb=0) == 0                 # item_count 0: TRC_OK, nothing looked at
    bad = fake_items(4, 600)
    bad[1].d_ptr = BASE + 8
    assert call(items=bad, hist=hist + 4) == E_ARG and re.search(r"\bitem 1\b", err())
    assert call(hist=hist + 4, table=None) == E_ARG and "8-byte" in err()
    assert call(table=table + 16) == E_ARG and "table" in err()
    assert call(tb=tb - 1) == -3
    out = (C.c_uint8 * 4)(*([0xEE] * 4))
    assert L.trc_planes_advise_batch_dev(0, items, 4, 3, CHUNK, out, None, None, 0, None) == E_ARG and "esize" in err()
    assert L.trc_planes_advise_batch_dev(0, items, 4, esize, CHUNK, out, None, None, 0, None) == E_ARG and "filters" in err()
    assert L.trc_planes_advise_batch_dev(7, items, 4, esize, CHUNK, out, None, None, 0, None) == E_ARG and "workspace" in err()
    assert L.trc_planes_advise_batch_dev(7, items, 4, esize, CHUNK, out, None, table, 1024, None) == -3
    assert list(out) == [0xEE] * 4
