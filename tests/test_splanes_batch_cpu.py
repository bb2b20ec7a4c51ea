"""Batched byte planes with a filter and a stride per item, the parts that need no GPU: the numpy model VS against the models it is
built from; declarations and exports; a bad stride, which every call reports after the plan and the filters and before it looks at
a pointer; the TRCT container (trc_planes_sbatch_check / _info on containers assembled by hand, `trcfile l`); and the order-0
estimates behind the torch helper's inequalities.  The item pointers here are made-up device addresses: nothing dereferences them."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fplanes_batch_lib as FBL
import planes_batch_lib as BL
import planes_container_lib as CL
import splanes_batch_lib as SBL
import splanes_lib as SL
import trc
from test_planes_container_cpu import ELEMS, inner_container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_split_sbatch_dev", "trc_planes_join_sbatch_dev", "trc_encode_splanes_batch_dev", "trc_decode_splanes_batch_dev",
           "trc_planes_hist_sbatch_dev", "trc_planes_advise_sbatch_dev", "trc_planes_sbatch_bound", "trc_planes_sbatch_check",
           "trc_planes_sbatch_info", "trc_planes_sbatch_pack_dev", "trc_decode_splanes_batch_packed_dev", "trc_encode_splanes_batch_host",
           "trc_decode_splanes_batch_host")
BASE = 0x7f0000000000                                         # a made-up, 256-byte aligned device address
ANY = 2**64 - 1
E_ARG = -1
ORDER = [1, 7, 8, 9, 255, 256, 257, 320, 513, 1025]            # elements per item
CHUNKS = (256, 320, 4096)
MAGIC = 0x54435254                                             # "TRCT"


def err():
    return trc.lib().trc_last_error().decode()


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", SL.ESIZES)
def test_stride_one_is_the_filtered_batch_model(esize):
    items = FBL.gen_items(esize, ORDER, 10 * esize)
    for chunk in CHUNKS:
        for name, filters in FBL.assignments(len(items), chunk).items():
            assert np.array_equal(SBL.virtual_filtered(items, filters, [1] * len(items), esize, chunk),
                                  FBL.virtual_filtered(items, filters, esize, chunk)), (chunk, name)
        # a stride on an item without a filter has no effect
        assert np.array_equal(SBL.virtual_filtered(items, [0] * len(items), [7] * len(items), esize, chunk), BL.virtual(items, esize, chunk))


@pytest.mark.parametrize("esize", SL.ESIZES)
def test_one_item_is_the_strided_filter_model(esize):
    for chunk in CHUNKS:
        for i, m in enumerate(ORDER + [3 * chunk + 5]):
            item = SL.gen(("random", "wrap", "interleaved")[i % 3], esize, m, 0, 100 * esize + i, 1 + i % 8)
            for f in SL.FILTERS:
                for s in (1, 2, 3, 5, 8):
                    assert np.array_equal(SBL.virtual_filtered([item], [f], [s], esize, chunk), SL.forward(item, esize, f, chunk, s)), (chunk, m, f, s)


@pytest.mark.parametrize("esize", SL.ESIZES)
def test_pad_is_zero_and_items_invert_alone(esize):
    items = FBL.gen_items(esize, ORDER, 20 * esize)
    sizes = [d.size for d in items]
    count = len(items)
    for chunk in CHUNKS:
        pl, first = BL.plan(sizes, esize, chunk)
        for sname, strides in SBL.stride_assignments(count, chunk).items():
            for fname, filters in SBL.filter_assignments(count).items():
                vs = SBL.virtual_filtered(items, filters, strides, esize, chunk)
                assert vs.size == pl["n_virtual"], (chunk, sname, fname)
                pads = 0
                for i, n in enumerate(sizes):
                    end = first[i + 1] * chunk * esize if i + 1 < count else vs.size
                    pad = vs[first[i] * chunk * esize + n:end]
                    assert not pad.any(), "chunk %d %s %s: the pad behind item %d is not zero" % (chunk, sname, fname, i)
                    pads += pad.size
                    assert np.array_equal(SBL.item_of(vs, i, sizes, filters[i], strides[i], esize, chunk), items[i]), (chunk, sname, fname, i)
                assert pads == pl["pad_elems"] * esize
    a = SBL.stride_assignments(20, 1)
    assert a["cycle"][:10] == [1, 2, 3, 4, 5, 6, 7, 8, 1, 2] and set(a["random"]) <= set(range(1, 9)) and len(set(a["random"])) > 4


def test_table_batch_estimates():
    """the torch helper's inequalities hold for the model's order-0 estimates already: the [rows, 4] table behind the delta at stride
    4 is estimated shorter than behind the stride-1 delta and than unfiltered, by more than any directory or model could give back"""
    arrays, filters, strides = SBL.table_batch()
    assert (filters, strides) == ([1, 1, 0], [4, 1, 1]) and arrays[0].shape == (4096, 4) and arrays[0].dtype == np.dtype("<i4")
    table = np.ascontiguousarray(arrays[0]).reshape(-1).view(np.uint8)
    m, esize, chunk = table.size // 4, 4, 512

    def bits(data):
        return SL.bits_per_byte(SL.plane_hist(data, esize), m, esize) * table.size

    strided, plain, none = bits(SL.forward(table, esize, SL.ZDELTA, chunk, 4)), bits(SL.forward(table, esize, SL.ZDELTA, chunk, 1)), bits(table)
    assert strided < 0.8 * none and strided < 0.8 * plain, (strided, plain, none)
    assert np.all(np.diff(arrays[1].astype(np.int64)) > 0), "the id column is sorted"


# ---- declarations ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_SBATCH_MAGIC\s+0x54435254u", txt) and struct.pack("<I", MAGIC) == b"TRCT" == struct.pack("<I", trc.SBATCH_MAGIC)
    for name in ("planes_split_sbatch", "planes_join_sbatch", "planes_hist_sbatch", "planes_sbatch_check", "planes_sbatch_info", "planes_strides"):
        assert hasattr(trc, name), name
    assert hasattr(trc.PlanesBatchCoder, "strided")


def test_planes_strides_helper():
    assert trc.planes_strides(None, 3) is None
    assert list(trc.planes_strides(4, 3)) == [4, 4, 4]
    assert list(trc.planes_strides([1, 2, 8], 3)) == [1, 2, 8]
    for bad in ([1, 2], [1, 2, 3, 4], [1, 2, 256], [1, -1, 1]):
        with pytest.raises(trc.TrcError):
            trc.planes_strides(bad, 3)


# ---- refusals before a device is needed --------------------------------------------------------------------------------------
def test_bad_stride_is_reported_without_a_device():
    L = trc.lib()
    esize, chunk = 2, 256
    sizes = [2 * 300, 2 * 1000, 2 * 7, 2 * 256]
    items = trc.planes_items([(BASE + 0x100000 * i, n) for i, n in enumerate(sizes)])
    pl, _ = BL.plan(sizes, esize, chunk)
    tb = L.trc_planes_batch_table_bytes(4, pl["chunks"])
    work = L.trc_planes_batch_work_bytes(trc.RCA, items, 4, esize, chunk)
    awork = L.trc_planes_advise_batch_work_bytes(items, 4, esize, chunk)
    assert tb and work and awork
    good_f, bad_f = trc.planes_filters([1, 0, 2, 2], 4), trc.planes_filters([1, 0, 3, 2], 4)
    planes, table, out = BASE + 0x1000000, BASE + 0x2000000, BASE + 0x3000000
    tot = (C.c_uint64 * 8)(*[10] * 8)
    chosen = (C.c_uint8 * 4)(*[0xEE] * 4)
    host_out = np.full(8192, 0xA5, dtype=np.uint8)
    calls = {
        "split": lambda f, s: L.trc_planes_split_sbatch_dev(items, f, s, 4, esize, chunk, planes, pl["pitch"], table, tb, None),
        "join": lambda f, s: L.trc_planes_join_sbatch_dev(planes, pl["pitch"], items, f, s, 4, 0, 4, esize, chunk, table, tb, None),
        "encode": lambda f, s: L.trc_encode_splanes_batch_dev(trc.RCA, items, f, s, 4, esize, chunk, None, 0, None, out, out + 0x100000, out + 0x200000,
                                                               planes, work, None),
        "decode": lambda f, s: L.trc_decode_splanes_batch_dev(trc.RCA, out, out + 0x100000, items, f, s, 4, 0, 1, esize, chunk, None, 0, planes, work, None),
        "hist": lambda f, s: L.trc_planes_hist_sbatch_dev(7, items, s, 4, 0, 4, esize, chunk, out, table, tb, None),
        "advise": lambda f, s: L.trc_planes_advise_sbatch_dev(7, items, s, 4, esize, chunk, chosen, None, planes, awork, None),
        "pack": lambda f, s: L.trc_planes_sbatch_pack_dev(trc.RCA, items, f, s, 4, esize, chunk, None, 0, None, out, out + 0x100000, out + 0x200000,
                                                          planes, 1 << 20, out + 0x300000, None),
        "packed": lambda f, s: L.trc_decode_splanes_batch_packed_dev(trc.RCA, out, 1 << 20, items, f, s, 4, 0, 1, esize, chunk, 0, tot, planes, work, None),
        "host": lambda f, s: -1 if L.trc_encode_splanes_batch_host(trc.RCA, items, f, s, 4, esize, chunk, 0, trc.ITEMS_HOST, host_out.ctypes.data,
                                                                    host_out.size) == 0 else 0,
    }
    for bad, text in (([1, 1, 0, 2], "stride 0"), ([1, 1, 9, 2], "stride 9")):
        st = trc.planes_strides(bad, 4)
        for name, call in calls.items():
            assert call(good_f, st) == E_ARG, name
            assert re.search(r"\bitem 2\b", err()) and text in err(), name + ": " + err()
    # every entry is validated: the last one, one outside a decoded range, one on an item without a filter
    assert calls["split"](good_f, trc.planes_strides([1, 1, 1, 255], 4)) == E_ARG and re.search(r"\bitem 3\b", err())
    assert calls["decode"](good_f, trc.planes_strides([1, 1, 1, 0], 4)) == E_ARG and re.search(r"\bitem 3\b", err())
    assert calls["encode"](good_f, trc.planes_strides([1, 9, 1, 1], 4)) == E_ARG and re.search(r"\bitem 1\b", err())
    # the plan comes first, then the filters ...
    bad_s = trc.planes_strides([1, 1, 9, 2], 4)
    assert L.trc_planes_split_sbatch_dev(items, good_f, bad_s, 4, 3, chunk, planes, pl["pitch"], table, tb, None) == E_ARG and "esize" in err()
    for name in ("split", "join", "encode", "decode", "pack", "packed", "host"):
        assert calls[name](bad_f, bad_s) == E_ARG and "filter 3" in err(), name + ": " + err()
    # ... and pointers and buffers after the strides: NULL everywhere with a bad stride is still the stride's error
    assert L.trc_planes_split_sbatch_dev(items, good_f, bad_s, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_planes_join_sbatch_dev(None, pl["pitch"], items, good_f, bad_s, 4, 0, 4, esize, chunk, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_encode_splanes_batch_dev(trc.RCA, items, good_f, bad_s, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_decode_splanes_batch_dev(trc.RCA, None, None, items, good_f, bad_s, 4, 0, 1, esize, chunk, None, 0, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_planes_hist_sbatch_dev(7, items, bad_s, 4, 0, 4, esize, chunk, None, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_planes_advise_sbatch_dev(7, items, bad_s, 4, esize, chunk, None, None, None, 0, None) == E_ARG and "stride 9" in err()
    assert L.trc_planes_sbatch_pack_dev(trc.RCA, items, good_f, bad_s, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None, None) == E_ARG and "stride 9" in err()
    assert L.trc_decode_splanes_batch_packed_dev(trc.RCA, None, 0, items, good_f, bad_s, 4, 0, 1, esize, chunk, 0, None, None, 0, None) == E_ARG and "stride 9" in err()
    # with good strides the same calls get as far as their buffers
    good_s = trc.planes_strides([4, 8, 3, 2], 4)
    assert L.trc_planes_split_sbatch_dev(items, good_f, good_s, 4, esize, chunk, None, pl["pitch"], None, 0, None) == E_ARG and "aligned" in err()
    assert L.trc_encode_splanes_batch_dev(trc.RCA, items, good_f, good_s, 4, esize, chunk, None, 0, None, None, None, None, None, 0, None) == E_ARG and "stride" not in err()
    assert list(chosen) == [0xEE] * 4 and (host_out == 0xA5).all()


def test_one_layout_per_content_and_the_low_nibble_coders():
    L = trc.lib()
    data = [np.arange(600, dtype=np.uint8), np.arange(512, dtype=np.uint8)]
    items = trc.planes_items([(d.ctypes.data, d.size) for d in data])
    out = np.full(8192, 0xA5, dtype=np.uint8)

    def host(codec, f, s):
        return L.trc_encode_splanes_batch_host(codec, items, trc.planes_filters(f, 2), trc.planes_strides(s, 2), 2, 2, 256, 0, trc.ITEMS_HOST,
                                               out.ctypes.data, out.size)
    # no item with a filter has a stride above 1: that content is a TRCB container
    for f, s in (([1, 2], [1, 1]), ([1, 0], [1, 5]), (None, [3, 3]), ([1, 2], None)):
        assert host(trc.RCA, f, s) == 0 and "trc_encode_planes_batch_host" in err(), (f, s, err())
    for codec in (trc.RCA4, trc.RC4SS):
        assert host(codec, [1, 2], [2, 3]) == 0 and "low four bits" in err()
        assert trc.planes_sbatch_bound(codec, [600, 512], 2, 256, 0) == 0
    assert (out == 0xA5).all()
    assert trc.planes_sbatch_bound(trc.RCA, [600, 512], 2, 256, 0) == trc.planes_batch_bound(trc.RCA, [600, 512], 2, 256, 0) + 32
    assert trc.planes_sbatch_bound(trc.RCA, [600] * 17, 2, 256, 0) == trc.planes_batch_bound(trc.RCA, [600] * 17, 2, 256, 0) + 48
    assert trc.planes_sbatch_bound(trc.RCA, [600, 511], 2, 256, 0) == 0
    assert trc.planes_sbatch_prefix(16) == 32 and trc.planes_sbatch_prefix(17) == 48
    pc = L.trc_planes_sbatch_pack_dev(trc.RCA, items, trc.planes_filters([1, 0], 2), trc.planes_strides([1, 5], 2), 2, 2, 256, None, 0, None,
                                      None, None, None, None, 0, None, None)
    assert pc == E_ARG and "trc_planes_batch_pack_dev" in err()


# ---- the TRCT container by hand ------------------------------------------------------------------------------------------------
def make(esize=2, count=5, chunk=256, filters=None, strides=None, magic=MAGIC, version=1, zero=0, zero2=0, hdr_count=None, pad=0, inner_count=None, front_kw=None):
    """a TRCT container of `count` items by hand: the prefix, the TRCB front of planes_container_lib, sections with stub payloads.
    The keyword arguments are the defects of the checker's tests; pad: the value of the stride padding"""
    filters = [(i + 1) % 3 for i in range(count)] if filters is None else filters
    strides = [1 if f == 0 else 1 + (3 * i) % 8 for i, f in enumerate(filters)] if strides is None else strides
    sizes = [m * esize for m in ELEMS[:count]]
    nc = [-(-m // chunk) for m in ELEMS[:count]]
    M = (sum(nc) - nc[-1]) * chunk + ELEMS[count - 1]
    clens = [chunk if i % 3 == 0 else 40 + i for i in range(sum(nc))]
    clens[-1] = min(clens[-1], M - (sum(nc) - 1) * chunk)
    inner = inner_container(esize, trc.RCA, M, chunk, clens)
    front = CL.front(sizes, filters, esize, chunk, CL.inner_offset(count) + len(inner), count=inner_count, **(front_kw or {}))
    prefix = struct.pack("<IBBHQ", magic, version, zero, zero2, count if hdr_count is None else hdr_count) + bytes(strides) + bytes([pad] * (-count % 16))
    assert len(prefix) == trc.planes_sbatch_prefix(count)
    return np.concatenate([np.frombuffer(prefix, dtype=np.uint8), front, np.frombuffer(inner, dtype=np.uint8)]), filters, strides


def check(buf, buflen=None, count=ANY):
    return trc.lib().trc_planes_sbatch_check(buf.ctypes.data, buf.size if buflen is None else buflen, count)


def test_header_struct(tmp_path):
    src = tmp_path / "sz.c"
    fields = ("magic", "version", "zero", "zero2", "count")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(trc_planes_sbatch_hdr), ' + ", ".join("offsetof(trc_planes_sbatch_hdr, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [16, 0, 4, 5, 6, 8]


@pytest.mark.parametrize("esize", (2, 4, 8))
@pytest.mark.parametrize("count", (1, 5, 8, 9))
def test_check_accepts(esize, count):
    buf, filters, strides = make(esize, count)
    assert check(buf) == 0, err()
    assert check(buf, count=count) == 0
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
    trc.planes_sbatch_check(buf, count)
    h, n, f, s = trc.planes_sbatch_info(buf)
    prefix = trc.planes_sbatch_prefix(count)
    assert (h["count"], h["esize"], h["chunk"], h["size"]) == (count, esize, 256, buf.size - prefix)
    assert n == [m * esize for m in ELEMS[:count]] and f == filters and s == strides
    # behind the prefix: a batch container as it stands; the same bytes from the start are not one
    assert trc.lib().trc_planes_batch_check(buf[prefix:].ctypes.data, buf.size - prefix, count) == 0
    assert trc.lib().trc_planes_batch_check(buf.ctypes.data, buf.size, ANY) == E_ARG and "magic" in err()
    assert trc.is_planes_sbatch(buf) and not trc.is_planes_sbatch(buf[prefix:])


def test_check_rejects_each_defect():
    good, filters, strides = make(4, 5)
    assert check(good) == 0 and filters == [1, 2, 0, 1, 2] and strides == [1, 4, 1, 2, 5]
    for kw, why in ((dict(magic=CL.MAGIC), "magic"),
                    (dict(version=2), "version"),
                    (dict(zero=1), "reserved"),
                    (dict(zero2=1), "reserved"),
                    (dict(strides=[1, 4, 1, 0, 5]), "item 3: stride 0"),
                    (dict(strides=[1, 4, 1, 2, 9]), "item 4: stride 9"),
                    (dict(strides=[1, 4, 3, 2, 5]), "item 2: stride 3 on an item without a filter"),
                    (dict(pad=1), "stride padding"),
                    (dict(inner_count=4), "items"),
                    (dict(front_kw=dict(version=2)), "batch container: version"),
                    (dict(front_kw=dict(zero2=1)), "batch container: reserved")):
        buf = make(4, 5, **kw)[0]
        assert check(buf) == E_ARG, why
        assert err().startswith("strided batch container:") and why in err(), (why, err())
    bad = good.copy(); bad[8:16] = np.frombuffer(struct.pack("<Q", 0), np.uint8)
    assert check(bad) == E_ARG and "0 items" in err()
    bad = good.copy(); bad[8:16] = np.frombuffer(struct.pack("<Q", 21), np.uint8)      # more strides than the batch has items
    assert check(bad) == E_ARG and err().startswith("strided batch container:")
    assert check(good, buflen=good.size - 1) == E_ARG and "the buffer holds" in err()        # truncated
    assert check(good, buflen=12) == E_ARG and "shorter than the header" in err()
    assert check(good, buflen=24) == E_ARG and "shorter than the strides" in err()
    assert check(good, buflen=trc.planes_sbatch_prefix(5) + 40) == E_ARG and "shorter than the header" in err()
    assert check(good, count=4) == E_ARG and "caller expects 4" in err()
    with pytest.raises(trc.TrcError, match="strided batch container"):
        trc.planes_sbatch_check(bad)
    # the host decoders refuse what does not check, before a device is needed; each takes its own container only
    L = trc.lib()
    sizes = [4 * m for m in ELEMS[:5]]
    dst = np.zeros(max(sizes), dtype=np.uint8)
    it = trc.planes_items([(dst.ctypes.data, n) for n in sizes])
    bad = good.copy(); bad[4] = 2
    assert L.trc_decode_splanes_batch_host(bad.ctypes.data, bad.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "version" in err()
    assert L.trc_decode_planes_batch_host(good.ctypes.data, good.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "magic" in err()
    prefix = trc.planes_sbatch_prefix(5)
    assert L.trc_decode_splanes_batch_host(good[prefix:].ctypes.data, good.size - prefix, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "magic" in err()
    out = np.full(64, 0xA5, dtype=np.uint8)
    assert L.trc_decode_xplanes_host(good.ctypes.data, good.size, out.ctypes.data, 8) == 0 and (out == 0xA5).all()
    it[3].n += 4
    assert L.trc_decode_splanes_batch_host(good.ctypes.data, good.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "item 3" in err()


def test_info_with_a_short_table():
    buf, filters, strides = make(2, 9)
    h, n, f, s = trc.planes_sbatch_info(buf, cap=4)
    assert h["count"] == 9 and n == [2 * m for m in ELEMS[:4]] and f == filters[:4] and s == strides[:4]
    h, n, f, s = trc.planes_sbatch_info(buf, cap=100)
    assert len(n) == 9 and len(f) == 9 and s == strides
    L = trc.lib()
    hdr = trc.PlanesBatchHdr()
    nn, ff, ss = (C.c_uint64 * 6)(*[7] * 6), (C.c_uint8 * 6)(*[7] * 6), (C.c_uint8 * 6)(*[77] * 6)
    assert L.trc_planes_sbatch_info(buf.ctypes.data, buf.size, C.byref(hdr), nn, ff, ss, 4) == 0
    assert list(nn[4:]) == [7, 7] and list(ff[4:]) == [7, 7] and list(ss[4:]) == [77, 77] and list(ss[:4]) == strides[:4]
    assert hdr.size == buf.size - trc.planes_sbatch_prefix(9)
    bad = buf.copy(); bad[0] = 0
    assert L.trc_planes_sbatch_info(bad.ctypes.data, bad.size, C.byref(hdr), nn, ff, ss, 4) == E_ARG and "magic" in err()


def test_trcfile_lists_the_container_without_a_gpu(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    path = tmp_path / "batch.trct"
    buf, filters, strides = make(4, 5)
    buf.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 0, l.stderr
    lines = l.stdout.splitlines()
    assert lines[0] == "5 items, esize 4, chunk 256, codec %d, %d -> %d bytes" % (trc.RCA, 4 * sum(ELEMS[:5]), buf.size)
    assert lines[1:] == ["item %d: %d bytes, filter %s, stride %d" % (i, 4 * ELEMS[i], "nzx"[f], s) for i, (f, s) in enumerate(zip(filters, strides))]
    bad = buf.copy(); bad[16 + 1] = 9
    bad.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 2 and "strided batch container" in l.stderr and "stride 9" in l.stderr
