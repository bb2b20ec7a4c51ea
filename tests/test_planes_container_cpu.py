"""The TRCB container of a coded batch, the parts that need no GPU: declarations and exports, the header struct through a C
compiler, bound / auto chunk / layout against the numpy definition (planes_container_lib), trc_planes_batch_check on containers
assembled by hand, trc_planes_batch_info, what the host encoder refuses before it looks for a device, and `trcfile l`."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import planes_batch_lib as BL
import planes_container_lib as CL
import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
E_ARG = -1
SYMBOLS = ("trc_planes_batch_auto_chunk", "trc_planes_batch_bound", "trc_planes_batch_layout_host", "trc_planes_batch_check",
           "trc_planes_batch_info", "trc_planes_batch_pack_dev", "trc_decode_planes_batch_packed_dev", "trc_encode_planes_batch_host",
           "trc_encode_aplanes_batch_host", "trc_decode_planes_batch_host")
COUNTS = (1, 5, 8, 9)                                          # filter padding of 7, 3, 0 and 7 bytes
ELEMS = [300, 256, 44, 1, 255, 257, 512, 299, 77]              # elements per item, the first `count` of them


def err():
    return trc.lib().trc_last_error().decode()


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)


def test_symbols_declared_and_exported():
    txt = header_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_BATCH_MAGIC\s+0x42435254u", txt)
    assert re.search(r"enum\s*\{\s*TRC_ITEMS_HOST\s*=\s*0\s*,\s*TRC_ITEMS_DEV\s*=\s*1\s*\}", txt)
    assert struct.pack("<I", trc.PLANES_BATCH_MAGIC) == b"TRCB" and trc.PLANES_BATCH_MAGIC == CL.MAGIC
    for name in ("planes_batch_check", "parse_planes_batch", "planes_batch_bound", "host_encode_planes_batch", "host_decode_planes_batch"):
        assert hasattr(trc, name), name
    assert hasattr(trc.PlanesBatchCoder, "pack") and hasattr(trc.PlanesBatchCoder, "decode_packed")


def test_header_struct(tmp_path):
    """sizeof(trc_planes_batch_hdr) == 48 with the fields where the format puts them: by a C compiler and through ctypes"""
    src = tmp_path / "sz.c"
    fields = ("magic", "version", "esize", "zero", "chunk", "zero2", "count", "inner", "size", "bytes")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu %zu'
                   + " %zu" * len(fields) + '\\n", sizeof(trc_planes_batch_hdr), sizeof(trc_planes_batch_layout), '
                   + ", ".join("offsetof(trc_planes_batch_hdr, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = [48, 80, 0, 4, 5, 6, 8, 12, 16, 24, 32, 40]
    assert [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == want
    assert C.sizeof(trc.PlanesBatchHdr) == 48 == trc.PLANES_BATCH_HDR == CL.HDR
    assert [getattr(trc.PlanesBatchHdr, f).offset for f in fields] == want[2:]
    assert C.sizeof(trc.PlanesBatchLayout) == 80


# ---- bound, auto chunk, layout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", (2, 4, 8))
@pytest.mark.parametrize("count", COUNTS)
def test_bound_and_layout_match_the_definition(esize, count):
    L = trc.lib()
    sizes = [m * esize for m in ELEMS[:count]]
    assert CL.inner_offset(count) == 48 + 8 * count + ((count + 7) & ~7)
    for codec, cdfnum in ((trc.RCA, 0), (trc.ANS4S, 256), (trc.RCS1, 17), (trc.RCSS, trc.ss_prm((5, 6)))):
        for chunk in (256, 320, 4096):
            p, _ = BL.plan(sizes, esize, chunk)
            want = CL.bound(sizes, esize, chunk, L.trc_planes_bound(p["n_virtual"], esize, chunk, cdfnum))
            assert trc.planes_batch_bound(codec, sizes, esize, chunk, cdfnum) == want, (codec, chunk)
            rng = np.random.default_rng(count * 100 + esize)
            for totals in ([0] * esize, [p["m_total"]] * esize, [int(x) for x in rng.integers(0, p["m_total"] + 1, esize)]):
                inner, off, size = CL.layout(sizes, esize, chunk, codec, cdfnum, totals)
                got = trc.planes_batch_layout(codec, sizes, esize, chunk, cdfnum, totals)
                assert (got["inner"], got["off"], got["size"]) == (inner, off, size), (codec, chunk, totals)
                assert all(o % 8 == 0 for o in off) and size % 8 == 0 and size + trc.PAD <= want, "the bound holds every layout and TRC_PAD"
            with pytest.raises(trc.TrcError, match="payload bytes"):
                trc.planes_batch_layout(codec, sizes, esize, chunk, cdfnum, [0] * (esize - 1) + [p["m_total"] + 1])
        # chunk 0: the chunk of trc_encode_planes_host for n = sum n[i]
        auto = trc.planes_batch_auto_chunk(codec, sizes, esize)
        assert auto == L.trc_auto_chunk_codec(codec, sum(sizes) // esize)
        assert trc.planes_batch_bound(codec, sizes, esize, 0, cdfnum) == trc.planes_batch_bound(codec, sizes, esize, auto, cdfnum) > 0
    assert trc.planes_batch_auto_chunk(trc.RCC1, sizes, esize) == 16384          # a coder's floor


def test_bound_is_zero_for_what_the_calls_reject():
    good = [600, 512]
    assert trc.planes_batch_bound(trc.RCA, good, 2, 256, 0) > 0
    for codec, sizes, esize, chunk, cdfnum in ((trc.RCA, good, 3, 256, 0), (trc.RCA, good, 2, 100, 0), (trc.RCA, [600, 511], 2, 256, 0),
                                               (trc.RCA, [600, 0], 2, 256, 0), (trc.RCA, [], 2, 256, 0), (42, good, 2, 256, 0),
                                               (trc.RCA4, good, 2, 256, 0), (trc.RC4SS, good, 2, 256, trc.ss_prm((5, 6))),
                                               (trc.ANS4S, good, 2, 256, 0), (trc.ANS4S, good, 2, 256, 257), (trc.RCSS, good, 2, 256, 0)):
        assert trc.planes_batch_bound(codec, sizes, esize, chunk, cdfnum) == 0, (codec, sizes, esize, chunk, cdfnum)
    # (it looks at no pointer: the items above carry NULL)
    for codec, sizes, esize in ((trc.RCA, good, 3), (trc.RCA, [600, 511], 2), (trc.RCA, [], 2), (42, good, 2), (trc.RCA4, good, 2)):
        assert trc.planes_batch_auto_chunk(codec, sizes, esize) == 0, (codec, sizes, esize)


# ---- trc_planes_batch_check on hand-made containers ---------------------------------------------------------------------------
def section(codec, m, chunk, clens, cdfnum=0):
    """a TRC1 container with a stub payload, as test_planes_cpu.py builds its sections"""
    lens = [min(chunk, m - i * chunk) for i in range(len(clens))]
    pay = sum(min(l, ln) for l, ln in zip(clens, lens))
    hdr = struct.pack("<IBBHIIQQ", 0x31435254, codec, 1, cdfnum, chunk, len(clens), m, pay)
    return hdr + struct.pack("<%dI" % len(clens), *clens) + bytes(range(256)) * (pay // 256) + bytes(range(pay % 256))


def inner_container(esize, codec, m, chunk, clens, hdr_chunk=None, tail=0, cdfnum=0):
    secs = [section(codec, m, chunk, clens, cdfnum)] * esize
    pos, off, body = 32 + 8 * esize, [], b""
    for s in secs:
        off.append(pos)
        s = s + b"\0" * (-len(s) % 8)
        body += s
        pos += len(s)
    hdr = struct.pack("<IBBBBIIQQ", trc.PLANES_MAGIC, codec, 1, esize, tail, chunk if hdr_chunk is None else hdr_chunk, cdfnum, m * esize, pos)
    return hdr + struct.pack("<%dQ" % esize, *off) + body


def make(esize=2, count=5, chunk=256, codec=trc.RCA, filters=None, sizes=None, inner_kw=None, size_delta=0, hdr_count=None, **front_kw):
    """a TRCB container of `count` items by hand: the front of planes_container_lib, sections with stub payloads"""
    sizes = [m * esize for m in ELEMS[:count]] if sizes is None else sizes
    elems = [-(-n // esize) for n in sizes]
    nc = [-(-m // chunk) for m in elems]
    M = (sum(nc) - nc[-1]) * chunk + elems[-1]
    clens = [chunk if i % 3 == 0 else 40 + i for i in range(sum(nc))]
    clens[-1] = min(clens[-1], M - (sum(nc) - 1) * chunk)
    inner = inner_container(esize, codec, M, chunk, clens, **(inner_kw or {}))
    size = CL.inner_offset(count) + len(inner) + size_delta
    f = CL.front(sizes, filters, esize, chunk, size, count=hdr_count, **front_kw)
    return np.concatenate([f, np.frombuffer(inner, dtype=np.uint8)])


def check(buf, buflen=None, count=ANY):
    return trc.lib().trc_planes_batch_check(buf.ctypes.data, buf.size if buflen is None else buflen, count)


@pytest.mark.parametrize("esize", (2, 4, 8))
@pytest.mark.parametrize("count", COUNTS)
def test_check_accepts(esize, count):
    filters = [i % 3 for i in range(count)]
    buf = make(esize, count, filters=filters)
    assert check(buf) == 0, err()
    assert check(buf, count=count) == 0
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
    assert check(make(esize, count)) == 0                                      # a batch without filters: zero bytes
    trc.planes_batch_check(buf, count)
    p = trc.parse_planes_batch(buf)
    assert (p["count"], p["esize"], p["chunk"], p["size"], p["inner"]) == (count, esize, 256, buf.size, CL.inner_offset(count))
    assert p["n"] == [m * esize for m in ELEMS[:count]] and p["filters"] == filters and p["bytes"] == sum(p["n"])
    assert p["codec"] == trc.RCA and len(p["total"]) == esize
    # the inner part is a planes container as it stands
    assert trc.lib().trc_planes_check(buf[p["inner"]:].ctypes.data, buf.size - p["inner"], ANY) == 0


def test_check_rejects_each_defect():
    good = make(4, 5)
    assert check(good) == 0
    for buf, why in ((make(4, 5, magic=trc.PLANES_MAGIC), "magic"),
                     (make(4, 5, version=2), "version"),
                     (make(4, 5, zero=1), "reserved"),
                     (make(4, 5, zero2=1), "reserved"),
                     (make(4, 5, hdr_count=0), "0 items"),
                     (make(4, 5, inner=CL.inner_offset(5) + 8), "inner offset"),
                     (make(4, 5, size_delta=8), "the buffer holds"),
                     (make(4, 5, filters=[0, 1, 2, 3, 0]), "item 3: filter 3"),
                     (make(4, 5, pad=1), "filter padding"),
                     (make(4, 5, nbytes=4 * sum(ELEMS[:5]) + 4), "add up"),
                     (make(4, 5, inner_kw={"hdr_chunk": 320}), "chunk"),
                     (make(4, 5, inner_kw={"tail": 1}), "tail"),
                     (make(4, 5, codec=trc.RCA4), "low four bits")):
        assert check(buf) == E_ARG, why
        assert err().startswith("batch container:") and why in err(), (why, err())
    bad = good.copy(); bad[5] = 3                                              # esize 3
    assert check(bad) == E_ARG and "esize 3" in err()
    bad = good.copy(); bad[8:12] = np.frombuffer(struct.pack("<I", 100), np.uint8)
    assert check(bad) == E_ARG and "chunk 100" in err()
    bad = good.copy(); bad[48 + 8 * 2:48 + 8 * 3] = np.frombuffer(struct.pack("<Q", 4 * ELEMS[2] + 1), np.uint8)
    assert check(bad) == E_ARG and "item 2 has" in err() and err().startswith("batch container:")
    assert check(good, buflen=good.size - 1) == E_ARG and "the buffer holds" in err()        # truncated
    assert check(good, buflen=40) == E_ARG and "shorter than the header" in err()
    assert check(good, count=4) == E_ARG and "caller expects 4" in err()
    with pytest.raises(trc.TrcError, match="batch container"):
        trc.planes_batch_check(bad)


def test_info_with_a_short_table():
    buf = make(2, 9, filters=[i % 3 for i in range(9)])
    h, n, f = trc.planes_batch_info(buf, cap=4)
    assert h["count"] == 9 and n == [2 * m for m in ELEMS[:4]] and f == [0, 1, 2, 0]
    h, n, f = trc.planes_batch_info(buf, cap=100)
    assert len(n) == 9 and len(f) == 9
    # nothing behind `cap` entries is written
    L = trc.lib()
    hdr = trc.PlanesBatchHdr()
    nn, ff = (C.c_uint64 * 6)(*[7] * 6), (C.c_uint8 * 6)(*[7] * 6)
    assert L.trc_planes_batch_info(buf.ctypes.data, buf.size, C.byref(hdr), nn, ff, 4) == 0
    assert list(nn[4:]) == [7, 7] and list(ff[4:]) == [7, 7] and hdr.size == buf.size
    bad = buf.copy(); bad[0] = 0
    assert L.trc_planes_batch_info(bad.ctypes.data, bad.size, C.byref(hdr), nn, ff, 4) == E_ARG and "magic" in err()


# ---- the host encoder's refusals that need no device ---------------------------------------------------------------------------
def test_host_encode_refuses_before_a_device_is_needed():
    L = trc.lib()
    data = [np.arange(600, dtype=np.uint8), np.arange(512, dtype=np.uint8)]
    items = trc.planes_items([(d.ctypes.data, d.size) for d in data])
    out = np.full(8192, 0xA5, dtype=np.uint8)
    for codec in (trc.RCA4, trc.RC4SS):
        assert L.trc_encode_planes_batch_host(codec, items, None, 2, 2, 256, 0, trc.ITEMS_HOST, out.ctypes.data, out.size) == 0
        assert "low four bits" in err()
        assert L.trc_encode_aplanes_batch_host(codec, items, 2, 2, 256, 0, trc.ITEMS_HOST, out.ctypes.data, out.size, None) == 0
        assert "low four bits" in err()
    bad = (C.c_uint8 * 2)(0, 3)
    assert L.trc_encode_planes_batch_host(trc.RCA, items, bad, 2, 2, 256, 0, trc.ITEMS_HOST, out.ctypes.data, out.size) == 0
    assert "item 1: filter 3" in err()
    with pytest.raises(trc.TrcError, match="item 1: filter 3"):
        trc.host_encode_planes_batch(trc.RCA, data, 2, 256, filters=[0, 3])
    assert (out == 0xA5).all()
    # a container that does not check is refused by the decoder before a device is needed, and so is a size that differs
    buf = make(2, 5)
    sizes = [2 * m for m in ELEMS[:5]]
    dst = np.zeros(max(sizes), dtype=np.uint8)
    it = trc.planes_items([(dst.ctypes.data, n) for n in sizes])
    bad = buf.copy(); bad[4] = 2
    assert L.trc_decode_planes_batch_host(bad.ctypes.data, bad.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "version" in err()
    it[3].n += 2
    assert L.trc_decode_planes_batch_host(buf.ctypes.data, buf.size, it, 5, 0, 1, trc.ITEMS_HOST) == 0 and "item 3" in err()


# ---- the harness ----------------------------------------------------------------------------------------------------------------
def test_trcfile_lists_a_container_without_a_gpu(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2
    for mode in ("trcfile b <id> <esize> <chunk|0> <n|z|x|a> <out> <in>...", "trcfile B <in> <first> <count> <out>", "trcfile l <in>",
                 "trcfile f <id> <esize> <z|x> <in> <out>", "trcfile a <id> <esize> <in> <out>"):
        assert mode in u.stderr, mode
    path = tmp_path / "batch.trcb"
    buf = make(4, 5, filters=[0, 1, 2, 0, 1])
    buf.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 0, l.stderr
    lines = l.stdout.splitlines()
    assert lines[0].startswith("5 items, esize 4, chunk 256, codec %d" % trc.RCA)
    assert lines[1:] == ["item %d: %d bytes, filter %s" % (i, 4 * ELEMS[i], "nzx"[f]) for i, f in enumerate([0, 1, 2, 0, 1])]
    bad = buf.copy(); bad[0] = 0
    bad.tofile(str(path))
    l = subprocess.run([str(exe), "l", str(path)], capture_output=True, text=True)
    assert l.returncode == 2 and "batch container" in l.stderr
