"""Batched byte planes, the parts that need no GPU: declarations and exports, trc_planes_batch_plan_host against the numpy plan,
the size functions, and every argument the calls reject.  The item pointers here are made-up device addresses: nothing
dereferences them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import planes_batch_lib as BL
import planes_lib as PL
import trc
from planes_matrix_lib import ASSIGNED, LOW4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trc_planes_batch_plan_host", "trc_planes_batch_work_bytes", "trc_planes_batch_range_work_bytes",
           "trc_planes_split_batch_dev", "trc_planes_join_batch_dev", "trc_planes_batch_table_bytes",
           "trc_encode_planes_batch_dev", "trc_decode_planes_batch_dev")
BASE = 0x7f0000000000                                         # a made-up, 16-byte aligned device address
E_ARG = -1


def items_of(sizes, ptrs=None):
    return trc.planes_items([(BASE + 0x100000 * i if ptrs is None else ptrs[i], n) for i, n in enumerate(sizes)])


def plan_rc(sizes, esize, chunk, count=None, items=None):
    p = trc.PlanesBatchPlan()
    return trc.lib().trc_planes_batch_plan_host(items_of(sizes) if items is None else items, len(sizes) if count is None else count,
                                                esize, chunk, C.byref(p), None)


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_BATCH_MAX\s+1048576u", txt) and trc.PLANES_BATCH_MAX == 1048576
    for name in ("PlanesBatchCoder", "planes_items", "planes_batch_plan", "planes_split_batch", "planes_join_batch"):
        assert hasattr(trc, name), name


def test_header_structs_compile_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "trc_hip.h"\n'
                   "_Static_assert(sizeof(trc_planes_item) == 16, \"item\");\n"
                   "_Static_assert(sizeof(trc_planes_batch_plan) == 40, \"plan\");\n"
                   "int main(void) { trc_planes_item it = { 0, 2 }; trc_planes_batch_plan p;\n"
                   "  return trc_planes_batch_plan_host(&it, 1, 2, TRC_CHUNK_MIN, &p, 0) + (int)trc_planes_batch_table_bytes(1, 1); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(trc.PlanesItem) == 16 and C.sizeof(trc.PlanesBatchPlan) == 40


def random_lists():
    """50 seeded (sizes, esize, chunk): one to forty items of one element to a few chunks, whole chunks and single elements among them"""
    out = []
    for seed in range(50):
        rng = np.random.default_rng(seed)
        esize = int(rng.choice(PL.ESIZES))
        chunk = int(rng.choice([256, 320, 4096, 65536]))
        count = int(rng.integers(1, 41))
        m = [int(x) for x in rng.integers(1, 3 * chunk + 2, count)]
        for i in range(count):
            r = rng.integers(0, 6)
            m[i] = 1 if r == 0 else chunk * int(rng.integers(1, 4)) if r == 1 else m[i]
        out.append(([x * esize for x in m], esize, chunk))
    return out


def test_plan_against_numpy():
    L = trc.lib()
    for sizes, esize, chunk in random_lists():
        want, want_first = BL.plan(sizes, esize, chunk)
        got, first = trc.planes_batch_plan(items_of(sizes), len(sizes), esize, chunk)
        assert got == want and first == want_first, (sizes, esize, chunk)
        assert got["n_virtual"] == got["m_total"] * esize and got["pitch"] == L.trc_planes_pitch(got["n_virtual"], esize)
        assert got["pad_elems"] == sum(-(n // esize) % chunk for n in sizes[:-1])
        # the pointers are not the plan's business: a caller who decodes a few items plans with the others NULL
        null = trc.planes_items([(None, n) for n in sizes])
        assert trc.planes_batch_plan(null, len(sizes), esize, chunk) == (want, want_first)
    # one item: the figures of the plain call on it
    got, first = trc.planes_batch_plan(items_of([2 * 1000]), 1, 2, 256)
    assert got == {"m_total": 1000, "n_virtual": 2000, "chunks": 4, "pitch": L.trc_planes_pitch(2000, 2), "pad_elems": 0} and first == [0, 4]


def test_work_bytes():
    L = trc.lib()
    for sizes, esize, chunk in random_lists()[:20]:
        items, count = items_of(sizes), len(sizes)
        pl, first = BL.plan(sizes, esize, chunk)
        assert L.trc_planes_batch_table_bytes(count, pl["chunks"]) >= 32 * count + 4 * pl["chunks"]
        for codec in (trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS):
            w = L.trc_planes_batch_work_bytes(codec, items, count, esize, chunk)
            assert w % 256 == 0 and w >= L.trc_planes_work_bytes(codec, pl["n_virtual"], esize, chunk) + L.trc_planes_batch_table_bytes(count, pl["chunks"])
            assert w >= L.trc_planes_work_bytes(codec, pl["n_virtual"], esize, chunk) > 0
            for fi, ic in {(0, 1), (count - 1, 1), (count // 2, count - count // 2), (0, count)}:
                chunks = first[fi + ic] - first[fi]
                r = L.trc_planes_batch_range_work_bytes(codec, items, count, esize, chunk, fi, ic)
                assert r % 256 == 0 and r >= L.trc_planes_range_work_bytes(codec, pl["n_virtual"], esize, chunk, chunks) + L.trc_planes_batch_table_bytes(ic, chunks)
                assert L.trc_planes_range_work_bytes(codec, pl["n_virtual"], esize, chunk, chunks) > 0
    # a single item's decode workspace grows with its chunks, not with the batch
    sizes = [2 * 1000] * 300
    items = items_of(sizes)
    one = L.trc_planes_batch_range_work_bytes(trc.RCA, items, 300, 2, 256, 150, 1)
    assert 0 < one < L.trc_planes_batch_range_work_bytes(trc.RCA, items, 300, 2, 256, 0, 300)
    assert one == L.trc_planes_batch_range_work_bytes(trc.RCA, items, 300, 2, 256, 7, 1)


def test_table_bytes():
    L = trc.lib()
    assert L.trc_planes_batch_table_bytes(1, 1) == 512
    assert L.trc_planes_batch_table_bytes(0, 1) == 0 and L.trc_planes_batch_table_bytes(trc.PLANES_BATCH_MAX + 1, 1 << 21) == 0
    assert L.trc_planes_batch_table_bytes(3, 2) == 0                   # every item has a chunk
    assert L.trc_planes_batch_table_bytes(1, 0x80000000) == 0
    assert L.trc_planes_batch_table_bytes(trc.PLANES_BATCH_MAX, 0x7fffffff) >= 32 * trc.PLANES_BATCH_MAX + 4 * 0x7fffffff


REJECTED = [  # (sizes, esize, chunk, count or None): what the plan, and with it every call, rejects
    ([4096], 2, 256, 0),                                       # count == 0
    ([4096, 1], 2, 256, None),                                 # n[i] < esize
    ([4096, 0, 4096], 4, 256, None),
    ([4096, 4098], 4, 256, None),                              # n[i] % esize != 0
    ([4097], 2, 256, None),
    ([4096], 3, 256, None), ([4096], 1, 256, None), ([4096], 16, 256, None), ([4096], 0, 256, None),      # esize
    ([4096], 2, 0, None), ([4096], 2, 100, None), ([4096], 2, 192, None), ([4096], 2, 65600, None), ([4096], 2, 288, None),   # chunk
    ([2 * 256 * 0x40000000, 2 * 256 * 0x40000000], 2, 256, None),      # NC = 2^31
]


@pytest.mark.parametrize("sizes,esize,chunk,count", REJECTED)
def test_rejected_arguments(sizes, esize, chunk, count):
    L = trc.lib()
    items, cnt = items_of(sizes), len(sizes) if count is None else count
    assert plan_rc(sizes, esize, chunk, count) == E_ARG and err()
    for codec in (trc.ANS4S, trc.RCA):
        assert L.trc_planes_batch_work_bytes(codec, items, cnt, esize, chunk) == 0
        assert L.trc_planes_batch_range_work_bytes(codec, items, cnt, esize, chunk, 0, 1) == 0


def test_rejected_count_and_chunks_at_the_limits():
    L = trc.lib()
    big = trc.PLANES_BATCH_MAX + 1
    arr = (trc.PlanesItem * big)()
    for i in range(0, big):
        arr[i].d_ptr, arr[i].n = BASE, 2
    p = trc.PlanesBatchPlan()
    assert L.trc_planes_batch_plan_host(arr, big, 2, 256, C.byref(p), None) == E_ARG and "items" in err()
    assert L.trc_planes_batch_work_bytes(trc.RCA, arr, big, 2, 256) == 0
    assert L.trc_planes_batch_range_work_bytes(trc.RCA, arr, big, 2, 256, 0, 1) == 0
    assert L.trc_planes_batch_plan_host(arr, big - 1, 2, 256, C.byref(p), None) == 0 and p.chunks == big - 1 and p.m_total == 256 * (big - 2) + 1
    assert L.trc_planes_batch_work_bytes(trc.RCA, arr, big - 1, 2, 256) > 0
    # NC = 2^31 - 1 is the last that plans
    assert plan_rc([2 * 256 * 0x40000000, 2 * 256 * 0x3fffffff], 2, 256) == 0
    assert L.trc_planes_batch_plan_host(None, 1, 2, 256, C.byref(p), None) == E_ARG             # a NULL item array
    assert L.trc_planes_batch_plan_host(arr, 1, 2, 256, None, None) == E_ARG                    # ... or plan


def test_rejected_pointers_flags_and_coders():
    L = trc.lib()
    sizes = [2 * 300, 2 * 1000, 2 * 7, 2 * 256]
    good = items_of(sizes)
    assert L.trc_planes_batch_work_bytes(trc.RCA, good, 4, 2, 256) > 0
    for bad_ptr in (None, BASE + 8, BASE + 1):
        ptrs = [BASE, BASE + 0x10000, bad_ptr, BASE + 0x30000]
        items = items_of(sizes, ptrs)
        assert L.trc_planes_batch_work_bytes(trc.RCA, items, 4, 2, 256) == 0
        assert L.trc_planes_batch_range_work_bytes(trc.RCA, items, 4, 2, 256, 2, 1) == 0       # an item the call touches
        assert L.trc_planes_batch_range_work_bytes(trc.RCA, items, 4, 2, 256, 1, 3) == 0
        assert L.trc_planes_batch_range_work_bytes(trc.RCA, items, 4, 2, 256, 0, 2) > 0        # ... and one it does not
        assert L.trc_planes_batch_range_work_bytes(trc.RCA, items, 4, 2, 256, 3, 1) > 0
    for fi, ic in ((0, 5), (4, 1), (5, 0), (2, 3), (0, 0), (4, 0)):                            # outside the batch, or nothing to decode
        assert L.trc_planes_batch_range_work_bytes(trc.RCA, good, 4, 2, 256, fi, ic) == 0
    for codec in (trc.RCA | trc.TABLES_READY, trc.RCA | trc.DIR_READY, trc.ANS4S | trc.TABLES_READY, 0, 42, 255):
        assert L.trc_planes_batch_work_bytes(codec, good, 4, 2, 256) == 0
        assert L.trc_planes_batch_range_work_bytes(codec, good, 4, 2, 256, 0, 1) == 0
    assert L.trc_planes_batch_work_bytes(trc.ANSB, good, 4, 2, 16384) == 0                     # a chunk above the coder's own limit
    assert L.trc_planes_batch_work_bytes(trc.ANSB, good, 4, 2, 8192) > 0


def test_low_nibble_coders_have_no_batch_workspace():
    L = trc.lib()
    assert len(LOW4) == 7
    for esize in PL.ESIZES:
        sizes = [esize * 300, esize * 1000, esize]
        items = items_of(sizes)
        for codec in ASSIGNED:
            w = L.trc_planes_batch_work_bytes(codec, items, 3, esize, 256)
            r = L.trc_planes_batch_range_work_bytes(codec, items, 3, esize, 256, 1, 1)
            if codec in LOW4:
                assert w == 0 and r == 0, (trc.CODEC_NAMES[codec], esize)
            else:
                assert w and r, (trc.CODEC_NAMES[codec], esize)


def test_numpy_virtual_buffer():
    for esize in PL.ESIZES:
        rng = np.random.default_rng(esize)
        items = [rng.integers(1, 256, m * esize, dtype=np.uint8) for m in (1, 256, 257, 5)]
        v = BL.virtual(items, esize, 256)
        pl, first = BL.plan([d.size for d in items], esize, 256)
        assert v.size == pl["n_virtual"] and first == [0, 1, 2, 4, 5] and pl["pad_elems"] == 255 + 0 + 255
        for d, f in zip(items, first):
            assert np.array_equal(v[f * 256 * esize:f * 256 * esize + d.size], d)
        assert int((v == 0).sum()) == pl["pad_elems"] * esize
        assert np.array_equal(BL.virtual(items[:1], esize, 256), items[0])             # one item: the item itself
