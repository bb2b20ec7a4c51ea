"""The TRCE container of a batch coded against a base per item, and the batched base fingerprint, the parts that need no GPU:
declarations and exports, the header struct through a C compiler, trc_planes_bbatch_bound, trc_planes_bbatch_check on containers
assembled by hand -- one defect per check, in the documented order, with neighbouring pairs for the order --,
trc_planes_bbatch_info, and what the device calls refuse before they look for a device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bbatch_container_lib as EL
import planes_container_lib as CL
import trc
from test_planes_container_cpu import ELEMS, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
E_ARG, E_WORK = -1, -3
SYMBOLS = ("trc_base_fingerprint_batch_table_bytes", "trc_base_fingerprint_batch_dev", "trc_base_verify_batch_dev", "trc_planes_bbatch_bound",
           "trc_planes_bbatch_check", "trc_planes_bbatch_info", "trc_planes_bbatch_pack_dev", "trc_decode_bplanes_batch_packed_dev")


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_BBATCH_MAGIC\s+0x45435254u", txt)
    assert struct.pack("<I", trc.BBATCH_MAGIC) == b"TRCE" and trc.BBATCH_MAGIC == EL.MAGIC
    for name in ("planes_bbatch_check", "planes_bbatch_info", "parse_planes_bbatch", "planes_bbatch_bound", "base_fingerprint_batch"):
        assert hasattr(trc, name), name
    assert issubclass(trc.BasePlanesBatchCoder, trc.PlanesBatchCoder)
    assert all(hasattr(trc.BasePlanesBatchCoder, m) for m in ("pack", "decode_packed", "verify"))


def test_header_struct(tmp_path):
    """sizeof(trc_planes_bbatch_hdr) == 16 with the fields where the format puts them, by a C compiler"""
    src = tmp_path / "sz.c"
    fields = ("magic", "version", "zero", "zero2", "count")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(trc_planes_bbatch_hdr), ' + ", ".join("offsetof(trc_planes_bbatch_hdr, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [16, 0, 4, 5, 6, 8]
    assert EL.HDR == 16 and [EL.prefix_bytes(c) for c in (1, 2, 3, 4)] == [32, 32, 48, 48] == [trc.planes_bbatch_prefix(c) for c in (1, 2, 3, 4)]


@pytest.mark.parametrize("esize", (2, 4, 8))
def test_bound_is_the_batch_bound_plus_the_prefix(esize):
    for count in (1, 2, 5, 9):
        sizes = [m * esize for m in ELEMS[:count]]
        for codec, cdfnum in ((trc.RCA, 0), (trc.ANS4S, 256), (trc.RCSS, trc.ss_prm((5, 6)))):
            for chunk in (256, 320, 4096, 0):
                b = trc.planes_batch_bound(codec, sizes, esize, chunk, cdfnum)
                assert b > 0 and trc.planes_bbatch_bound(codec, sizes, esize, chunk, cdfnum) == b + EL.prefix_bytes(count), (codec, count, chunk)
    for codec, sizes, es, chunk in ((trc.RCA, [600, 511], 2, 256), (trc.RCA, [], 2, 256), (trc.RCA4, [600], 2, 256), (trc.RCA, [600], 3, 256), (trc.RCA, [600], 2, 100)):
        assert trc.planes_bbatch_bound(codec, sizes, es, chunk, 0) == 0, (codec, sizes, es, chunk)


# ---- trc_planes_bbatch_check on hand-made containers --------------------------------------------------------------------------
FILTERS5 = [1, 0, 2, 0, 1]
FPS5 = [0x1111111111111111, 0, 0xFFFFFFFFFFFFFFFF, 0, 3]


def build(count=5, filters=None, fps=None, trcb_kw=None, hdr_count=None, **prefix_kw):
    """a TRCE container by hand: the prefix of bbatch_container_lib in front of test_planes_container_cpu's hand-made TRCB container"""
    filters = (FILTERS5 * 2)[:count] if filters is None else filters
    fps = [f if fl else 0 for f, fl in zip((FPS5 * 2), filters)][:count] if fps is None else fps
    return np.concatenate([EL.prefix(fps, count=hdr_count, **prefix_kw), make(count=count, filters=filters, **(trcb_kw or {}))])


def check(buf, buflen=None, count=ANY):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    return trc.lib().trc_planes_bbatch_check(buf.ctypes.data, buf.size if buflen is None else buflen, count)


def refused(text, buf, **kw):
    assert check(buf, **kw) == E_ARG, text
    assert err().startswith("based batch container:") and text in err(), "%r is not in %r" % (text, err())


def test_check_accepts_the_definition():
    for count in (1, 2, 5, 8, 9):
        b = build(count=count)
        assert check(b) == 0 and check(b, count=count) == 0, err()
        assert check(np.concatenate([b, np.zeros(100, np.uint8)])) == 0, "bytes behind the container are the caller's"
        trc.planes_batch_check(b[EL.prefix_bytes(count):], count)          # the TRCB part alone, as it stands
    trc.planes_bbatch_check(build(), 5)


def test_check_one_defect_per_check_in_order():
    refused("shorter than the header", build(), buflen=15)
    refused("bad magic", build(magic=CL.MAGIC))
    refused("version 2", build(version=2))
    refused("reserved fields", build(zero=1))
    refused("reserved fields", build(zero2=0x100))
    refused("0 items", build(hdr_count=0))
    refused("%d items" % ((1 << 20) + 1), build(hdr_count=(1 << 20) + 1))
    refused("caller expects 4", build(), count=4)
    refused("shorter than the fingerprints", build(), buflen=EL.prefix_bytes(5) - 1)
    refused("padding must be zero", build(pad=1))
    refused("batch container: bad magic", build(trcb_kw=dict(magic=EL.MAGIC)))
    refused("batch container:", build(), buflen=build().size - 1)
    refused("fingerprints in front of a batch container of 4 items", np.concatenate([EL.prefix([1, 0, 2, 0, 0]), make(count=4, filters=[1, 0, 2, 0])]))
    refused("item 3: base fingerprint 0x0000000000000007 on an item without a filter", build(fps=[1, 0, 2, 7, 3]))
    refused("no item has a filter", build(filters=[0] * 5))
    refused("TRCB", build(filters=[0] * 5))
    refused("no item has a filter", build(count=1, filters=[0]))


def test_check_order_of_neighbouring_checks():
    """two defects at once: the earlier check of the documented order speaks"""
    refused("bad magic", build(magic=0x54435254, version=2))                                   # magic before version
    refused("version 0", build(version=0, zero=9))                                             # version before the zero fields
    refused("reserved fields", build(zero=9, hdr_count=0))                                         # the zero fields before the count
    refused("0 items", build(hdr_count=0), buflen=20)                                              # the count before the prefix's length
    refused("caller expects 3", build(), buflen=20, count=3)
    refused("shorter than the fingerprints", build(pad=5), buflen=EL.prefix_bytes(5) - 8)      # the length before the padding
    refused("padding must be zero", build(pad=5, trcb_kw=dict(version=7)))                     # the padding before the TRCB part
    refused("batch container: version 7", build(count=5, trcb_kw=dict(version=7), fps=[1, 5, 2, 0, 3]))      # the TRCB part before the fingerprints
    refused("fingerprints in front of a batch container of 4", np.concatenate([EL.prefix([1, 5, 2, 0, 0]), make(count=4, filters=[1, 0, 2, 0])]))      # equal counts before base_fp == 0
    refused("item 0: base fingerprint", build(filters=[0] * 5, fps=[9, 0, 0, 0, 0]))          # base_fp == 0 before "a filter set"


def test_info():
    b = build(count=9)
    filters = (FILTERS5 * 2)[:9]
    want_fp = [f if fl else 0 for f, fl in zip(FPS5 * 2, filters)]
    h, n, f, fp = trc.planes_bbatch_info(b)
    assert h["count"] == 9 and h["magic"] == CL.MAGIC and h["size"] == b.size - EL.prefix_bytes(9)
    assert n == [m * 2 for m in ELEMS[:9]] and f == filters and fp == want_fp
    h3, n3, f3, fp3 = trc.planes_bbatch_info(b, cap=3)
    assert (h3, n3, f3, fp3) == (h, n[:3], f[:3], fp[:3])
    # nothing behind min(cap, count) entries
    L = trc.lib()
    hh = trc.PlanesBatchHdr()
    nn, ff, pp = (C.c_uint64 * 12)(*[7] * 12), (C.c_uint8 * 12)(*[7] * 12), (C.c_uint64 * 12)(*[7] * 12)
    assert L.trc_planes_bbatch_info(b.ctypes.data, b.size, C.byref(hh), nn, ff, pp, 12) == 0
    assert list(nn[9:]) == [7] * 3 and list(ff[9:]) == [7] * 3 and list(pp[9:]) == [7] * 3 and list(pp[:9]) == want_fp
    assert L.trc_planes_bbatch_info(b.ctypes.data, b.size, C.byref(hh), None, None, None, 0) == 0
    assert L.trc_planes_bbatch_info(b.ctypes.data, b.size, None, None, None, None, 0) == E_ARG
    assert L.trc_planes_bbatch_info(b.ctypes.data, b.size - 1, C.byref(hh), None, None, None, 0) == E_ARG and err().startswith("based batch container:")
    info = trc.parse_planes_bbatch(build(count=5))
    assert info["prefix"] == 64 and info["base_fp"] == [FPS5[0], 0, FPS5[2], 0, FPS5[4]] and info["filters"] == FILTERS5


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
FAKE = 1 << 20                                                 # an aligned address nobody dereferences: the calls refuse first


def test_fingerprint_batch_refusals():
    L = trc.lib()
    assert [L.trc_base_fingerprint_batch_table_bytes(c) for c in (0, 1, 8, 9, 1 << 20, (1 << 20) + 1)] == [0, 512, 512, 768, 40 << 20, 0]
    items = trc.planes_items([(None, 600), (None, 7), (None, 4096)])
    bases = trc.planes_bases([FAKE, None, FAKE + 4096], 3)
    tb = L.trc_base_fingerprint_batch_table_bytes(3)

    def call(items=items, bases=bases, filters=[1, 0, 2], count=3, fi=0, ic=3, d_fp=FAKE, d_table=FAKE, table_bytes=tb):
        return L.trc_base_fingerprint_batch_dev(items, bases, trc.planes_filters(filters, 3), count, fi, ic,
                                                d_fp, d_table, table_bytes, None)
    assert call(count=0) == E_ARG and "0 items" in err()
    assert call(items=trc.planes_items([(None, 600), (None, 0), (None, 8)])) == E_ARG and "item 1 has no bytes" in err()
    assert call(filters=[1, 3, 2]) == E_ARG and "item 1: filter 3" in err()
    assert call(fi=2, ic=2) == E_ARG and "items [2, 2 + 2) of 3" in err()
    assert call(bases=trc.planes_bases([FAKE, None, None], 3)) == E_ARG and "item 2" in err()
    assert call(bases=trc.planes_bases([FAKE + 8, None, FAKE], 3)) == E_ARG and "item 0" in err()
    assert call(bases=None) == E_ARG and "item 0" in err()
    assert call(d_fp=FAKE + 4) == E_ARG and "d_fp" in err()
    assert call(d_fp=None) == E_ARG and "d_fp" in err()
    assert call(d_table=FAKE + 16) == E_ARG and "256-byte" in err()
    assert call(table_bytes=tb - 1) == E_WORK
    assert call(filters=[1, 3, 2], fi=2, ic=2) == E_ARG and "filter 3" in err()               # the filters before the range
    assert call(fi=2, ic=2, bases=None) == E_ARG and "items [2" in err()                       # the range before the pointers
    assert call(bases=None, d_fp=None) == E_ARG and "item 0" in err()                          # the bases before d_fp
    assert call(d_fp=FAKE + 4, table_bytes=0) == E_ARG                                         # the pointers before the table
    assert call(ic=0, d_fp=None, d_table=None, table_bytes=0) == 0                             # no item: TRC_OK, nothing enqueued
    assert call(fi=1, ic=1, bases=None, d_fp=None) == E_ARG and "d_fp" in err()                # an unfiltered item needs no base


def test_verify_and_container_calls_refuse_before_any_device():
    L = trc.lib()
    items = trc.planes_items([(FAKE, 600), (FAKE + 4096, 512)])
    bases = trc.planes_bases([FAKE, FAKE + 4096], 2)
    f = trc.planes_filters([1, 2], 2)
    tb = L.trc_base_fingerprint_batch_table_bytes(2)
    assert L.trc_base_verify_batch_dev(FAKE + 4, items, bases, f, 2, 0, 2, FAKE, FAKE, tb, None) == E_ARG and "d_cont" in err()
    assert L.trc_base_verify_batch_dev(FAKE, items, bases, f, 2, 0, 2, FAKE + 4, FAKE, tb, None) == E_ARG and "d_bad" in err()
    assert L.trc_base_verify_batch_dev(FAKE, items, bases, f, 0, 0, 0, FAKE, FAKE, tb, None) == E_ARG and "0 items" in err()
    assert L.trc_base_verify_batch_dev(FAKE, items, bases, trc.planes_filters([1, 9], 2), 2, 0, 2, FAKE, FAKE, tb, None) == E_ARG and "item 1: filter 9" in err()
    assert L.trc_base_verify_batch_dev(FAKE, items, bases, f, 2, 0, 2, FAKE, FAKE, tb - 1, None) == E_WORK

    def pack(codec=trc.RCA, filters=f, count=2, bases=bases, out_bytes=1 << 20, table_bytes=tb, chunk=256):
        return L.trc_planes_bbatch_pack_dev(codec, items, bases, filters, count, 2, chunk, None, 0, None, FAKE, FAKE, FAKE, FAKE, out_bytes, FAKE,
                                            FAKE, table_bytes, None)
    assert pack(count=0) == E_ARG and "0 items" in err()
    assert pack(chunk=100) == E_ARG and "chunk" in err()
    assert pack(filters=trc.planes_filters([1, 3], 2)) == E_ARG and "item 1: filter 3" in err()
    assert pack(filters=trc.planes_filters([0, 0], 2)) == E_ARG and "TRCB" in err() and "trc_planes_batch_pack_dev" in err()
    assert pack(filters=None) == E_ARG and "trc_planes_batch_pack_dev" in err()
    assert pack(bases=None) == E_ARG and "item 0" in err()
    assert pack(out_bytes=8) == E_WORK and "trc_planes_bbatch_bound" in err()
    assert pack(table_bytes=tb - 1) == E_WORK
    assert pack(codec=trc.RCA4) == E_ARG and "low four bits" in err()
    assert pack(out_bytes=trc.planes_bbatch_bound(trc.RCA, [600, 512], 2, 256, 0) - 1) == E_WORK

    tot = (C.c_uint64 * 8)()

    def decode(codec=trc.RCA, filters=f, count=2, bases=bases):
        return L.trc_decode_bplanes_batch_packed_dev(codec, FAKE, 1 << 20, items, bases, filters, count, 0, 2, 2, 256, 0, tot, FAKE, 1 << 30, None)
    assert decode(count=0) == E_ARG and "0 items" in err()
    assert decode(filters=trc.planes_filters([4, 1], 2)) == E_ARG and "item 0: filter 4" in err()
    assert decode(codec=trc.RCA4) == E_ARG and "low four bits" in err()


def test_coder_class_requires_bases():
    with pytest.raises(ValueError, match="bases"):
        trc.BasePlanesBatchCoder(trc.RCA, [], bases=None)


def test_trcfile_lists_a_based_batch_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "harness", "trcfile")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    path = tmp_path / "hand.trce"
    b = build(count=5)
    b.tofile(str(path))
    r = subprocess.run([exe, "l", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "5 items, esize 2, chunk 256, codec 4, %d -> %d bytes, against bases" % (sum(m * 2 for m in ELEMS[:5]), b.size), lines[0]
    assert lines[1:] == ["item 0: 600 bytes, filter z, base 1111111111111111", "item 1: 512 bytes, filter n", "item 2: 88 bytes, filter x, base ffffffffffffffff",
                         "item 3: 2 bytes, filter n", "item 4: 510 bytes, filter z, base 0000000000000003"]
    bad = b.copy()
    bad[5] = 1                                                  # a reserved field
    bad.tofile(str(path))
    r = subprocess.run([exe, "l", str(path)], capture_output=True, text=True)
    assert r.returncode == 2 and "based batch container: reserved fields" in r.stderr
