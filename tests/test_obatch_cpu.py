"""Batched byte planes with a filter, a stride and a predictor order per item, the parts that need no GPU: the numpy model VO
against the models it is built from; declarations and exports; a bad order, which every call reports after the plan, the filters
and the strides and before it looks at a pointer; the one-layout refusals; the order advisor of a batch on histograms in host
memory; the TRCU container (trc_planes_obatch_bound / _check / _info on containers assembled by hand, `trcfile l`).  The item
pointers here are made-up device addresses: nothing dereferences them."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import obatch_lib as OBL
import oplanes_lib as OL
import planes_batch_lib as BL
import planes_container_lib as CL
import splanes_batch_lib as SBL
import splanes_lib as SL
import trc
from test_oplanes_cpu import shaped
from test_planes_container_cpu import ELEMS, inner_container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_split_obatch_dev", "trc_planes_join_obatch_dev", "trc_encode_oplanes_batch_dev", "trc_decode_oplanes_batch_dev",
           "trc_planes_hist_obatch_dev", "trc_planes_hist_obatch_bytes", "trc_planes_advise_obatch", "trc_planes_advise_obatch_dev",
           "trc_planes_advise_obatch_work_bytes", "trc_planes_obatch_bound", "trc_planes_obatch_check", "trc_planes_obatch_info",
           "trc_planes_obatch_pack_dev", "trc_decode_oplanes_batch_packed_dev", "trc_encode_oplanes_batch_host", "trc_decode_oplanes_batch_host",
           "trc_encode_aoplanes_batch_host")
BASE = 0x7f0000000000                                         # a made-up, 256-byte aligned device address
ANY = 2**64 - 1
E_ARG = -1
SIZES = [1, 7, 8, 9, 17, 25, 255, 256, 257, 320, 513, 1025]    # elements per item
CHUNKS = (256, 320, 4096)


def err():
    return trc.lib().trc_last_error().decode()


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", SL.ESIZES)
def test_order_one_is_the_strided_batch_model(esize):
    count = len(SIZES)
    items = OBL.gen_items(esize, SIZES, 10 * esize)
    for chunk in CHUNKS:
        for sname, strides in OBL.stride_assignments(count).items():
            for fname, filters in OBL.filter_assignments(count).items():
                assert np.array_equal(OBL.virtual_filtered(items, filters, strides, [1] * count, esize, chunk),
                                      SBL.virtual_filtered(items, filters, strides, esize, chunk)), (chunk, sname, fname)
        # an order on an item without the zigzag delta has no effect
        f = [0, 2] * (count // 2)
        assert np.array_equal(OBL.virtual_filtered(items, f, [3] * count, [3] * count, esize, chunk), SBL.virtual_filtered(items, f, [3] * count, esize, chunk))


@pytest.mark.parametrize("esize", SL.ESIZES)
def test_one_item_is_the_order_model(esize):
    for chunk in CHUNKS:
        for i, m in enumerate(SIZES + [3 * chunk + 5]):
            item = OL.gen(OL.KINDS[i % 4], esize, m, 0, 100 * esize + i, 1 + i % 8)
            for k in (1, 2, 3):
                for s in (1, 3, 8):
                    want = OL.forward(item, esize, k, chunk, s)
                    assert np.array_equal(OBL.virtual_filtered([item], [SL.ZDELTA], [s], [k], esize, chunk), want), (chunk, m, k, s)
                    assert np.array_equal(want, OL.scalar_forward(item, esize, k, chunk, s)) or m > 600, (chunk, m, k, s)


@pytest.mark.parametrize("esize", SL.ESIZES)
def test_pad_is_zero_and_items_invert_alone(esize):
    count = len(SIZES)
    for chunk in CHUNKS:
        for sname, strides in OBL.stride_assignments(count).items():
            items = OBL.gen_items(esize, SIZES, 20 * esize, lambda i: strides[i])
            sizes = [d.size for d in items]
            pl, first = BL.plan(sizes, esize, chunk)
            for oname, orders in OBL.order_assignments(count, chunk).items():
                for fname, filters in OBL.filter_assignments(count).items():
                    vo = OBL.virtual_filtered(items, filters, strides, orders, esize, chunk)
                    assert vo.size == pl["n_virtual"], (chunk, sname, oname, fname)
                    pads = 0
                    for i, n in enumerate(sizes):
                        end = first[i + 1] * chunk * esize if i + 1 < count else vo.size
                        pad = vo[first[i] * chunk * esize + n:end]
                        assert not pad.any(), "chunk %d %s %s %s: the pad behind item %d is not zero" % (chunk, sname, oname, fname, i)
                        pads += pad.size
                        assert np.array_equal(OBL.item_of(vo, i, sizes, filters[i], strides[i], orders[i], esize, chunk), items[i]), (chunk, sname, oname, fname, i)
                    assert pads == pl["pad_elems"] * esize
    a = OBL.order_assignments(20, 1)
    assert a["cycle"][:7] == [1, 2, 3, 1, 2, 3, 1] and set(a["random"]) == {1, 2, 3} and a["2"] == [2] * 20 and a["3"] == [3] * 20


def test_estimate_table():
    """the helper behind profiles/planes/obatch_notes.md at a quarter of its size: an order per item is estimated shorter than every
    uniform choice, and the picks are the issue's: 3, 1, 1, none, 3"""
    rows, (none, today, order2, best), picks = OBL.estimate_table(m=1 << 16)
    assert picks == [3, 1, 1, 0, 3]
    assert best < order2 < today < none and best < 0.85 * today
    for r in rows:
        assert min(r[2:]) <= r[2] and min(r[2:]) <= r[3]          # no item is worse than under today's choices


# ---- declarations ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_OBATCH_MAGIC\s+0x55435254u", txt) and struct.pack("<I", OBL.MAGIC) == b"TRCU" == struct.pack("<I", trc.OBATCH_MAGIC)
    for name in ("planes_split_obatch", "planes_join_obatch", "planes_hist_obatch", "planes_advise_obatch", "planes_advise_obatch_dev", "planes_obatch_bound",
                 "planes_obatch_check", "planes_obatch_info", "is_planes_obatch", "planes_orders"):
        assert hasattr(trc, name), name
    assert hasattr(trc.PlanesBatchCoder, "ordered")
    assert list(trc.planes_orders(2, 3)) == [2, 2, 2] and trc.planes_orders(None, 3) is None
    L = trc.lib()
    for esize in (2, 4, 8):
        assert L.trc_planes_hist_obatch_bytes(5, esize) == 5 * L.trc_planes_hist_order_bytes(esize) == 5 * 4 * esize * 256 * 8
        assert 3 * L.trc_planes_hist_obatch_bytes(5, esize) == 4 * L.trc_planes_hist_batch_bytes(5, esize)
    assert L.trc_planes_hist_obatch_bytes(5, 3) == 0 and L.trc_planes_hist_obatch_bytes(0, 4) == 0


def test_header_struct(tmp_path):
    src = tmp_path / "sz.c"
    fields = ("magic", "version", "zero", "zero2", "count")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(trc_planes_obatch_hdr), ' + ", ".join("offsetof(trc_planes_obatch_hdr, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [16, 0, 4, 5, 6, 8]


# ---- refusals before a device is needed --------------------------------------------------------------------------------------
def test_bad_order_is_reported_without_a_device():
    L = trc.lib()
    esize, chunk = 2, 256
    sizes = [2 * 300, 2 * 1000, 2 * 7, 2 * 256]
    items = trc.planes_items([(BASE + 0x100000 * i, n) for i, n in enumerate(sizes)])
    pl, _ = BL.plan(sizes, esize, chunk)
    tb = L.trc_planes_batch_table_bytes(4, pl["chunks"])
    work = L.trc_planes_batch_work_bytes(trc.RCA, items, 4, esize, chunk)
    assert tb and work
    good_f, bad_f = trc.planes_filters([1, 0, 1, 2], 4), trc.planes_filters([1, 0, 3, 2], 4)
    good_s, bad_s = trc.planes_strides([4, 8, 3, 2], 4), trc.planes_strides([1, 1, 9, 2], 4)
    planes, table, out = BASE + 0x1000000, BASE + 0x2000000, BASE + 0x3000000
    tot = (C.c_uint64 * 8)(*[10] * 8)
    host_out = np.full(8192, 0xA5, dtype=np.uint8)
    calls = {
        "split": lambda f, s, o: L.trc_planes_split_obatch_dev(items, f, s, o, 4, esize, chunk, planes, pl["pitch"], table, tb, None),
        "join": lambda f, s, o: L.trc_planes_join_obatch_dev(planes, pl["pitch"], items, f, s, o, 4, 0, 4, esize, chunk, table, tb, None),
        "encode": lambda f, s, o: L.trc_encode_oplanes_batch_dev(trc.RCA, items, f, s, o, 4, esize, chunk, None, 0, None, out, out + 0x100000, out + 0x200000,
                                                                  planes, work, None),
        "decode": lambda f, s, o: L.trc_decode_oplanes_batch_dev(trc.RCA, out, out + 0x100000, items, f, s, o, 4, 0, 1, esize, chunk, None, 0, planes, work, None),
        "pack": lambda f, s, o: L.trc_planes_obatch_pack_dev(trc.RCA, items, f, s, o, 4, esize, chunk, None, 0, None, out, out + 0x100000, out + 0x200000,
                                                             planes, 1 << 20, out + 0x300000, None),
        "packed": lambda f, s, o: L.trc_decode_oplanes_batch_packed_dev(trc.RCA, out, 1 << 20, items, f, s, o, 4, 0, 1, esize, chunk, 0, tot, planes, work, None),
        "host": lambda f, s, o: -1 if L.trc_encode_oplanes_batch_host(trc.RCA, items, f, s, o, 4, esize, chunk, 0, trc.ITEMS_HOST, host_out.ctypes.data,
                                                                       host_out.size) == 0 else 0,
    }
    for bad, text in (([1, 1, 0, 2], "order 0"), ([2, 1, 4, 2], "order 4")):
        od = trc.planes_orders(bad, 4)
        for name, call in calls.items():
            for s in (good_s, None):
                assert call(good_f, s, od) == E_ARG, name
                assert re.search(r"\bitem 2\b", err()) and text in err(), name + ": " + err()
    # every entry is validated: the last one, one outside a decoded range, one on an item without the zigzag delta
    assert calls["split"](good_f, good_s, trc.planes_orders([1, 1, 1, 255], 4)) == E_ARG and re.search(r"\bitem 3\b", err())
    assert calls["decode"](good_f, good_s, trc.planes_orders([1, 1, 1, 0], 4)) == E_ARG and re.search(r"\bitem 3\b", err())
    assert calls["encode"](good_f, good_s, trc.planes_orders([1, 4, 1, 1], 4)) == E_ARG and re.search(r"\bitem 1\b", err())
    # the plan comes first, then the filters, then the strides, then the orders ...
    bad_o = trc.planes_orders([2, 1, 4, 2], 4)
    assert L.trc_planes_split_obatch_dev(items, good_f, good_s, bad_o, 4, 3, chunk, planes, pl["pitch"], table, tb, None) == E_ARG and "esize" in err()
    for name, call in calls.items():
        assert call(bad_f, bad_s, bad_o) == E_ARG and "filter 3" in err(), name + ": " + err()
        assert call(good_f, bad_s, bad_o) == E_ARG and "stride 9" in err(), name + ": " + err()
        assert call(good_f, good_s, bad_o) == E_ARG and "order 4" in err(), name + ": " + err()
    # ... and pointers and buffers after the orders: NULL everywhere with a bad order is still the order's error
    assert L.trc_planes_split_obatch_dev(items, good_f, good_s, bad_o, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "order 4" in err()
    assert L.trc_planes_join_obatch_dev(None, pl["pitch"], items, good_f, good_s, bad_o, 4, 0, 4, esize, chunk, None, 0, None) == E_ARG and "order 4" in err()
    assert L.trc_encode_oplanes_batch_dev(trc.RCA, items, good_f, good_s, bad_o, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "order 4" in err()
    assert L.trc_decode_oplanes_batch_dev(trc.RCA, None, None, items, good_f, good_s, bad_o, 4, 0, 1, esize, chunk, None, 0, None, 0, None) == E_ARG and "order 4" in err()
    assert L.trc_planes_obatch_pack_dev(trc.RCA, items, good_f, good_s, bad_o, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None, None) == E_ARG and "order 4" in err()
    assert L.trc_decode_oplanes_batch_packed_dev(trc.RCA, None, 0, items, good_f, good_s, bad_o, 4, 0, 1, esize, chunk, 0, None, None, 0, None) == E_ARG and "order 4" in err()
    # with good orders the same calls get as far as their buffers, and name themselves as the calls whose kernels they launch
    good_o = trc.planes_orders([3, 1, 2, 1], 4)
    assert L.trc_planes_split_obatch_dev(items, good_f, good_s, good_o, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "aligned" in err()
    assert err().startswith("planes_split_obatch:")
    for o in (None, trc.planes_orders(1, 4), trc.planes_orders([1, 3, 1, 3], 4)):      # (orders above 1 on items without the zigzag delta)
        assert L.trc_planes_split_obatch_dev(items, good_f, good_s, o, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG
        assert err().startswith("planes_split_sbatch:"), err()
        assert L.trc_planes_join_obatch_dev(None, pl["pitch"], items, good_f, good_s, o, 4, 0, 4, esize, chunk, None, 0, None) == E_ARG
        assert err().startswith("planes_join_sbatch:"), err()
        assert L.trc_planes_split_obatch_dev(items, good_f, trc.planes_strides(1, 4), o, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG
        assert err().startswith("planes_split_fbatch:"), err()
        assert L.trc_planes_split_obatch_dev(items, trc.planes_filters(0, 4), good_s, o, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG
        assert err().startswith("planes_split_batch:"), err()
    assert L.trc_encode_oplanes_batch_dev(trc.RCA, items, good_f, good_s, good_o, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "order" not in err()
    assert (host_out == 0xA5).all()
    # the histograms and the advisor: the plan, the bit set, the strides, then pointers
    awork = L.trc_planes_advise_obatch_work_bytes(items, 4, esize, chunk)
    assert awork and awork >= L.trc_planes_advise_batch_work_bytes(items, 4, esize, chunk)
    cf, co = (C.c_uint8 * 4)(*[0xEE] * 4), (C.c_uint8 * 4)(*[0xEE] * 4)
    assert L.trc_planes_hist_obatch_dev(15, items, good_s, 4, 0, 4, 3, chunk, out, table, tb, None) == E_ARG and "esize" in err()
    for orders_set in (0, 16):
        assert L.trc_planes_hist_obatch_dev(orders_set, items, bad_s, 4, 0, 4, esize, chunk, out, table, tb, None) == E_ARG and "orders 0x" in err()
        assert L.trc_planes_advise_obatch_dev(orders_set, items, bad_s, 4, esize, chunk, cf, co, None, planes, awork, None) == E_ARG and "orders 0x" in err()
    assert L.trc_planes_hist_obatch_dev(15, items, bad_s, 4, 0, 4, esize, chunk, None, None, 0, None) == E_ARG and "stride 9" in err() and re.search(r"\bitem 2\b", err())
    assert L.trc_planes_advise_obatch_dev(15, items, bad_s, 4, esize, chunk, cf, co, None, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_planes_hist_obatch_dev(15, items, good_s, 4, 3, 2, esize, chunk, out, table, tb, None) == E_ARG and "items [3, 3 + 2) of 4" in err()
    assert L.trc_planes_hist_obatch_dev(15, items, good_s, 4, 4, 0, esize, chunk, None, None, 0, None) == 0          # an empty range: nothing to do
    assert L.trc_planes_hist_obatch_dev(15, items, good_s, 4, 0, 4, esize, chunk, None, table, tb, None) == E_ARG and "8-byte aligned" in err()
    assert L.trc_planes_advise_obatch_dev(15, items, good_s, 4, esize, chunk, cf, co, None, planes, awork - 1, None) == -3
    assert list(cf) == [0xEE] * 4 and list(co) == [0xEE] * 4


def test_one_layout_per_content_and_the_low_nibble_coders():
    L = trc.lib()
    data = [np.arange(600, dtype=np.uint8), np.arange(512, dtype=np.uint8)]
    items = trc.planes_items([(d.ctypes.data, d.size) for d in data])
    out = np.full(8192, 0xA5, dtype=np.uint8)

    def host(codec, f, s, o):
        return L.trc_encode_oplanes_batch_host(codec, items, trc.planes_filters(f, 2), trc.planes_strides(s, 2), trc.planes_orders(o, 2), 2, 2, 256, 0,
                                               trc.ITEMS_HOST, out.ctypes.data, out.size)
    # no zigzag-delta item has an order above 1: that content is a TRCT or TRCB container
    for f, s, o in (([1, 2], [2, 3], [1, 1]), ([1, 2], [2, 3], [1, 3]), ([0, 2], None, [3, 3]), (None, [3, 3], [2, 2]), ([1, 1], [2, 2], None)):
        assert host(trc.RCA, f, s, o) == 0 and "trc_encode_splanes_batch_host" in err() and "trc_encode_planes_batch_host" in err(), (f, s, o, err())
    for codec in (trc.RCA4, trc.RC4SS):
        assert host(codec, [1, 2], [2, 3], [2, 1]) == 0 and "low four bits" in err()
        assert trc.planes_obatch_bound(codec, [600, 512], 2, 256, 0) == 0
    assert (out == 0xA5).all()
    assert trc.planes_obatch_bound(trc.RCA, [600, 512], 2, 256, 0) == trc.planes_batch_bound(trc.RCA, [600, 512], 2, 256, 0) + 48
    assert trc.planes_obatch_bound(trc.RCA, [600] * 17, 2, 256, 0) == trc.planes_batch_bound(trc.RCA, [600] * 17, 2, 256, 0) + 80
    assert trc.planes_obatch_bound(trc.RCA, [600, 511], 2, 256, 0) == 0
    assert trc.planes_obatch_prefix(16) == 48 == OBL.prefix_bytes(16) and trc.planes_obatch_prefix(17) == 80 == OBL.prefix_bytes(17)
    for f, s, o in (([1, 0], [1, 5], [1, 3]), ([1, 2], [2, 2], None), ([2, 2], [2, 2], [3, 3])):
        pc = L.trc_planes_obatch_pack_dev(trc.RCA, items, trc.planes_filters(f, 2), trc.planes_strides(s, 2), trc.planes_orders(o, 2), 2, 2, 256, None, 0, None,
                                          None, None, None, None, 0, None, None)
        assert pc == E_ARG and "trc_planes_sbatch_pack_dev" in err() and "trc_planes_batch_pack_dev" in err(), err()


# ---- the order advisor of a batch -------------------------------------------------------------------------------------------
def test_advise_obatch_is_the_order_advisor_per_item():
    esize, chunk = 4, 256
    strides = [1, 1, 1, 1, 4, 3]
    datas = [d[:4 * m] for (_, _, d), m in zip(OBL.table_batch(1 << 12), (4096, 3000, 1025, 4096, 4096))] + [OL.gen("random", esize, 777, 0, 5)]
    count = len(datas)
    hist = np.stack([OL.hist4(d, esize, chunk, s) for d, s in zip(datas, strides)])
    items = trc.planes_items([(BASE + 0x100000 * i, d.size) for i, d in enumerate(datas)])
    for orders_set in (15, 7, 6, 9, 1, 8):
        f, o, adv = trc.planes_advise_obatch(hist, orders_set, esize, items, count)
        want = [OL.advise(h, orders_set, esize, d.size // esize) for h, d in zip(hist, datas)]
        assert [k if ff else 0 for ff, k in zip(f, o)] == want, orders_set
        assert all(ff == (SL.ZDELTA if k else SL.NONE) and oo == max(k, 1) for ff, oo, k in zip(f, o, want))
        for i in range(count):
            one = trc.planes_advise_order(hist[i], orders_set, esize, datas[i].size // esize)
            assert all(np.array_equal(adv[i][key], one[key]) for key in one), (orders_set, i)
    f, o, _ = trc.planes_advise_obatch(hist, 15, esize, items, count)
    picks = [k if ff else 0 for ff, k in zip(f, o)]              # smooth series: above 1; integer columns: 1; weights: no filter
    assert picks[0] >= 2 and picks[1:4] == [1, 1, 0] and picks[4] >= 2, picks
    assert trc.planes_advise_obatch(hist, 15, esize, items, count, advice=False)[2] is None


def test_advise_obatch_edge_and_errors():
    L = trc.lib()
    esize, m = 2, 1 << 16
    flat = shaped(m, 0)

    def hist(r0, r1, r2, r3):
        return np.concatenate([r.reshape(-1) for r in (r0, r1, r2, r3)])
    # an item at the 1/64 edge, on either side of it (test_oplanes_cpu.py finds the edge the same way)
    tot0 = OL.estimates(hist(flat, flat, flat, flat), esize, m)[0]
    delta = next(dl for dl in range(1, 256) if tot0 - OL.estimates(hist(flat, flat, shaped(m, dl), flat), esize, m)[2] >= tot0 / 64)
    below, at = hist(flat, flat, shaped(m, delta - 1), flat), hist(flat, flat, shaped(m, delta), flat)
    t = shaped(m, 200)
    h = np.stack([below, at, hist(flat, t, t, t), hist(flat, flat, flat, flat)])
    items = trc.planes_items([(BASE + 0x100000 * i, 2 * m) for i in range(4)])
    f, o, _ = trc.planes_advise_obatch(h, 15, esize, items, 4)
    assert (f, o) == ([0, 1, 1, 0], [1, 2, 1, 1])
    assert [OL.advise(x, 15, esize, m) for x in h] == [0, 2, 1, 0]
    f, o, _ = trc.planes_advise_obatch(h, 14, esize, items, 4)             # order 0 not requested: the argmin stands, ties to the lower order
    assert (f, o) == ([1, 1, 1, 1], [2, 2, 1, 1])
    # a row that does not sum to its item's elements: the item is named, nothing is written
    cf, co = (C.c_uint8 * 4)(*[0xEE] * 4), (C.c_uint8 * 4)(*[0xEE] * 4)
    adv = (trc.PlanesOrderAdvice * 4)()
    before = bytes(adv)
    bad = h.copy()
    bad[2, (3 * esize + 1) * 256 + 7] += 1
    assert L.trc_planes_advise_obatch(bad.ctypes.data, 15, esize, items, 4, cf, co, adv) == E_ARG
    assert re.search(r"\bitem 2\b", err()) and "order 3 plane 1" in err(), err()
    assert list(cf) == [0xEE] * 4 and list(co) == [0xEE] * 4 and bytes(adv) == before
    assert L.trc_planes_advise_obatch(bad.ctypes.data, 7, esize, items, 4, cf, co, adv) == 0 and list(cf) == [0, 1, 1, 0]      # ... and is not read where not requested
    items[1].n = 2 * m + 1
    assert L.trc_planes_advise_obatch(h.ctypes.data, 15, esize, items, 4, cf, co, None) == E_ARG and re.search(r"\bitem 1\b", err())
    items[1].n = 2 * m
    for orders_set in (0, 16):
        assert L.trc_planes_advise_obatch(h.ctypes.data, orders_set, esize, items, 4, cf, co, None) == E_ARG and "orders" in err()
    assert L.trc_planes_advise_obatch(h.ctypes.data, 15, 3, items, 4, cf, co, None) == E_ARG and "esize 3" in err()
    assert L.trc_planes_advise_obatch(h.ctypes.data, 15, esize, items, 0, cf, co, None) == E_ARG and "0 items" in err()
    for args in ((None, items, cf, co), (h.ctypes.data, None, cf, co), (h.ctypes.data, items, None, co), (h.ctypes.data, items, cf, None)):
        assert L.trc_planes_advise_obatch(args[0], 15, esize, args[1], 4, args[2], args[3], None) == E_ARG and "null" in err()
    with pytest.raises(trc.TrcError, match="histogram words"):
        trc.planes_advise_obatch(h[:3], 15, esize, items, 4)


# ---- the TRCU container by hand ------------------------------------------------------------------------------------------------
def make(esize=2, count=5, chunk=256, filters=None, strides=None, orders=None, inner_count=None, front_kw=None, **prefix_kw):
    """a TRCU container of `count` items by hand: the prefix of obatch_lib, the TRCB front of planes_container_lib, sections with stub
    payloads.  The keyword arguments are the defects of the checker's tests; strides and orders given are stored as they are"""
    filters = [(i + 1) % 3 for i in range(count)] if filters is None else filters
    raw = strides is not None or orders is not None
    strides = [1 if f == 0 else 1 + (3 * i) % 8 for i, f in enumerate(filters)] if strides is None else strides
    orders = [1 + (i // 3 + 1) % 3 if f == 1 else 1 for i, f in enumerate(filters)] if orders is None else orders
    sizes = [m * esize for m in ELEMS[:count]]
    nc = [-(-m // chunk) for m in ELEMS[:count]]
    M = (sum(nc) - nc[-1]) * chunk + ELEMS[count - 1]
    clens = [chunk if i % 3 == 0 else 40 + i for i in range(sum(nc))]
    clens[-1] = min(clens[-1], M - (sum(nc) - 1) * chunk)
    inner = inner_container(esize, trc.RCA, M, chunk, clens)
    front = CL.front(sizes, filters, esize, chunk, CL.inner_offset(count) + len(inner), count=inner_count, **(front_kw or {}))
    pre = OBL.prefix(filters, strides, orders, raw=raw, **prefix_kw)
    assert pre.size == trc.planes_obatch_prefix(count)
    return np.concatenate([pre, front, np.frombuffer(inner, dtype=np.uint8)]), filters, strides, orders


def check(buf, buflen=None, count=ANY):
    return trc.lib().trc_planes_obatch_check(buf.ctypes.data, buf.size if buflen is None else buflen, count)


@pytest.mark.parametrize("esize", (2, 4, 8))
@pytest.mark.parametrize("count", (1, 5, 8, 9))
def test_check_accepts(esize, count):
    buf, filters, strides, orders = make(esize, count)
    assert max(orders) > 1 and all(o == 1 for f, o in zip(filters, orders) if f != 1)
    assert check(buf) == 0, err()
    assert check(buf, count=count) == 0
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
    trc.planes_obatch_check(buf, count)
    h, n, f, s, o = trc.planes_obatch_info(buf)
    prefix = trc.planes_obatch_prefix(count)
    assert (h["count"], h["esize"], h["chunk"], h["size"]) == (count, esize, 256, buf.size - prefix)
    assert n == [m * esize for m in ELEMS[:count]] and f == filters and s == strides and o == orders
    # behind the prefix: a batch container as it stands; the same bytes from the start are neither that nor a TRCT container
    L = trc.lib()
    assert L.trc_planes_batch_check(buf[prefix:].ctypes.data, buf.size - prefix, count) == 0
    assert L.trc_planes_batch_check(buf.ctypes.data, buf.size, ANY) == E_ARG and "magic" in err()
    assert L.trc_planes_sbatch_check(buf.ctypes.data, buf.size, ANY) == E_ARG and "magic" in err()
    assert trc.is_planes_obatch(buf) and not trc.is_planes_obatch(buf[prefix:]) and not trc.is_planes_sbatch(buf)


def test_check_rejects_each_defect():
    good, filters, strides, orders = make(4, 5)
    assert check(good) == 0 and filters == [1, 2, 0, 1, 2] and strides == [1, 4, 1, 2, 5] and orders == [2, 1, 1, 3, 1]
    for kw, why in ((dict(magic=CL.MAGIC), "magic"),
                    (dict(magic=trc.SBATCH_MAGIC), "magic"),
                    (dict(version=2), "version"),
                    (dict(zero=1), "reserved"),
                    (dict(zero2=1), "reserved"),
                    (dict(strides=[1, 4, 1, 0, 5], orders=orders), "item 3: stride 0"),
                    (dict(strides=[1, 4, 1, 2, 9], orders=orders), "item 4: stride 9"),
                    (dict(strides=strides, orders=[2, 1, 1, 0, 1]), "item 3: order 0"),
                    (dict(strides=strides, orders=[4, 1, 1, 3, 1]), "item 0: order 4"),
                    (dict(strides=[1, 4, 3, 2, 5], orders=orders), "item 2: stride 3 on an item without a filter"),
                    (dict(strides=strides, orders=[2, 1, 2, 3, 1]), "item 2: order 2 on an item without the zigzag delta"),
                    (dict(strides=strides, orders=[2, 3, 1, 3, 1]), "item 1: order 3 on an item without the zigzag delta"),
                    (dict(strides=strides, orders=[1, 1, 1, 1, 1]), "no item has an order above 1"),
                    (dict(stride_pad=1), "stride padding"),
                    (dict(order_pad=1), "order padding"),
                    (dict(inner_count=4), "items"),
                    (dict(front_kw=dict(version=2)), "batch container: version"),
                    (dict(front_kw=dict(zero2=1)), "batch container: reserved")):
        buf = make(4, 5, **kw)[0]
        assert check(buf) == E_ARG, why
        assert err().startswith("ordered batch container:") and why in err(), (why, err())
    bad = good.copy(); bad[8:16] = np.frombuffer(struct.pack("<Q", 0), np.uint8)
    assert check(bad) == E_ARG and "0 items" in err()
    bad = good.copy(); bad[8:16] = np.frombuffer(struct.pack("<Q", 21), np.uint8)      # more strides and orders than the batch has items
    assert check(bad) == E_ARG and err().startswith("ordered batch container:")
    assert check(good, buflen=good.size - 1) == E_ARG and "the buffer holds" in err()        # truncated
    assert check(good, buflen=12) == E_ARG and "shorter than the header" in err()
    assert check(good, buflen=24) == E_ARG and "shorter than the strides and orders" in err()
    assert check(good, buflen=40) == E_ARG and "shorter than the strides and orders" in err()
    assert check(good, buflen=trc.planes_obatch_prefix(5) + 40) == E_ARG and "shorter than the header" in err()
    assert check(good, count=4) == E_ARG and "caller expects 4" in err()
    with pytest.raises(trc.TrcError, match="ordered batch container"):
        trc.planes_obatch_check(bad)
    # the host decoders refuse what does not check, before a device is needed; each takes its own container only
    L = trc.lib()
    sizes = [4 * m for m in ELEMS[:5]]
    dst = np.zeros(max(sizes), dtype=np.uint8)
    it = trc.planes_items([(dst.ctypes.data, n) for n in sizes])
    bad = good.copy(); bad[4] = 2
    assert L.trc_decode_oplanes_batch_host(bad.ctypes.data, bad.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "version" in err()
    assert L.trc_decode_planes_batch_host(good.ctypes.data, good.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "magic" in err()
    assert L.trc_decode_splanes_batch_host(good.ctypes.data, good.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "magic" in err()
    prefix = trc.planes_obatch_prefix(5)
    assert L.trc_decode_oplanes_batch_host(good[prefix:].ctypes.data, good.size - prefix, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "magic" in err()
    out = np.full(64, 0xA5, dtype=np.uint8)
    assert L.trc_decode_xplanes_host(good.ctypes.data, good.size, out.ctypes.data, 8) == 0 and (out == 0xA5).all()
    it[3].n += 4
    assert L.trc_decode_oplanes_batch_host(good.ctypes.data, good.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "item 3" in err()


def test_info_with_a_short_table():
    buf, filters, strides, orders = make(2, 9)
    h, n, f, s, o = trc.planes_obatch_info(buf, cap=4)
    assert h["count"] == 9 and n == [2 * m for m in ELEMS[:4]] and f == filters[:4] and s == strides[:4] and o == orders[:4]
    h, n, f, s, o = trc.planes_obatch_info(buf, cap=100)
    assert len(n) == 9 and len(f) == 9 and s == strides and o == orders
    L = trc.lib()
    hdr = trc.PlanesBatchHdr()
    nn, ff, ss, oo = (C.c_uint64 * 6)(*[7] * 6), (C.c_uint8 * 6)(*[7] * 6), (C.c_uint8 * 6)(*[77] * 6), (C.c_uint8 * 6)(*[78] * 6)
    assert L.trc_planes_obatch_info(buf.ctypes.data, buf.size, C.byref(hdr), nn, ff, ss, oo, 4) == 0
    assert list(nn[4:]) == [7, 7] and list(ff[4:]) == [7, 7] and list(ss[4:]) == [77, 77] and list(oo[4:]) == [78, 78]
    assert list(ss[:4]) == strides[:4] and list(oo[:4]) == orders[:4]
    assert hdr.size == buf.size - trc.planes_obatch_prefix(9)
    bad = buf.copy(); bad[0] = 0
    assert L.trc_planes_obatch_info(bad.ctypes.data, bad.size, C.byref(hdr), nn, ff, ss, oo, 4) == E_ARG and "magic" in err()
    assert L.trc_planes_obatch_info(buf.ctypes.data, buf.size, None, nn, ff, ss, oo, 4) == E_ARG


def test_trcfile_lists_the_container_without_a_gpu(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2 and "order advisor" in u.stderr
    path = tmp_path / "batch.trcu"
    buf, filters, strides, orders = make(4, 5)
    buf.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 0, l.stderr
    lines = l.stdout.splitlines()
    assert lines[0] == "5 items, esize 4, chunk 256, codec %d, %d -> %d bytes" % (trc.RCA, 4 * sum(ELEMS[:5]), buf.size)
    assert lines[1:] == ["item %d: %d bytes, filter %s, stride %d, order %d" % (i, 4 * ELEMS[i], "nzx"[f], s, o)
                         for i, (f, s, o) in enumerate(zip(filters, strides, orders))]
    bad = buf.copy(); bad[16 + 16] = 9
    bad.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 2 and "ordered batch container" in l.stderr and "order 9" in l.stderr
