"""Strided filtered byte planes, the parts that need no GPU: the declarations and exports, the header struct through a C compiler, the
numpy model F_S (splanes_lib) against the per-element restatement of the definition, against fplanes_lib at stride 1 and against
its pinned fixture tests/golden/splanes_vectors.npz, that restarts restart, the stride's argument errors from every new call,
trc_splanes_check on containers assembled by hand, and what the strides are for: the order-0 estimates of interleaved data and
the advisor's choice on them."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fplanes_lib as FL
import splanes_lib as SL
import trc
from test_fplanes_cpu import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
SYMBOLS = ("trc_planes_split_sfilter_dev", "trc_planes_join_sfilter_dev", "trc_encode_splanes_dev", "trc_decode_splanes_dev",
           "trc_decode_splanes_range_dev", "trc_planes_hist_stride_dev", "trc_splanes_bound", "trc_encode_splanes_host",
           "trc_decode_splanes_host", "trc_decode_splanes_range_host", "trc_splanes_check")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = header_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("planes_split_sfilter", "planes_join_sfilter", "StridedPlanesCoder", "planes_hist_stride", "splanes_bound",
                 "host_encode_splanes", "host_decode_splanes", "host_decode_splanes_range", "splanes_check", "SPLANES_MAGIC", "STRIDE_MAX"):
        assert hasattr(trc, name), name
    assert issubclass(trc.StridedPlanesCoder, trc.PlanesCoder)
    # the filter enum is not touched: the stride is an argument, not a filter
    assert re.search(r"enum\s*\{\s*TRC_FILTER_NONE\s*=\s*0\s*,\s*TRC_FILTER_ZDELTA\s*=\s*1\s*,\s*TRC_FILTER_XOR\s*=\s*2\s*\}", txt)


def test_header_struct(tmp_path):
    """sizeof(trc_splanes_hdr) == 16 with the fields where the TRCF prefix has them and the stride in its reserved field: read from
    the header by a C compiler, and through ctypes from a struct laid out as the header declares it"""
    txt = header_text()
    assert re.search(r"#define\s+TRC_SPLANES_MAGIC\s+0x53435254u", txt) and re.search(r"#define\s+TRC_STRIDE_MAX\s+8\b", txt)
    assert (trc.SPLANES_MAGIC, trc.STRIDE_MAX, trc.SPLANES_HDR) == (0x53435254, 8, 16) and SL.STRIDE_MAX == 8
    assert struct.pack("<I", trc.SPLANES_MAGIC) == b"TRCS"
    body = re.search(r"typedef struct trc_splanes_hdr \{(.*?)\} trc_splanes_hdr;", txt, flags=re.S).group(1)
    fields = re.findall(r"(uint\d+_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "magic"), ("uint8_t", "filter"), ("uint8_t", "version"), ("uint16_t", "stride"), ("uint64_t", "size")]
    ct = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}

    class Hdr(C.Structure):
        _fields_ = [(n, ct[t]) for t, n in fields]
    assert C.sizeof(Hdr) == 16
    assert [getattr(Hdr, n).offset for _, n in fields] == [0, 4, 5, 6, 8]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(trc_splanes_hdr), offsetof(trc_splanes_hdr, filter), offsetof(trc_splanes_hdr, stride), offsetof(trc_splanes_hdr, size), '
                   'sizeof(trc_fplanes_hdr), TRC_STRIDE_MAX); return 0; }\n')
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["16", "4", "6", "8", "16", "8"]


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", SL.ESIZES)
@pytest.mark.parametrize("filt", SL.FILTERS)
def test_model_is_the_definition_and_round_trips(esize, filt):
    for stride in (1,) + SL.STRIDES:
        for i, (seg, m, t) in enumerate(((256, 1, 0), (256, stride, 0), (256, stride + 1, esize - 1), (256, 700, esize - 1), (320, 961, 1))):
            kind = SL.KINDS[(i + stride) % 5]
            d = SL.gen(kind, esize, m, t, 11 * m + esize, stride)
            f = SL.forward(d, esize, filt, seg, stride)
            assert f.dtype == np.uint8 and f.size == d.size
            assert np.array_equal(f, SL.scalar_forward(d, esize, filt, seg, stride)), (kind, stride, seg, m, t)
            assert np.array_equal(f[m * esize:], d[m * esize:]), "the tail bytes are not filtered"
            assert np.array_equal(SL.inverse(f, esize, filt, seg, stride), d), (kind, stride, seg, m, t)


@pytest.mark.parametrize("esize", SL.ESIZES)
@pytest.mark.parametrize("filt", SL.FILTERS)
def test_model_is_the_definition_at_the_restart_lengths_of_the_gpu_matrix(esize, filt):
    """the points test_gpu_planes_restart.py adds: strides 4, 6 and 7 at every length of FL.RESTARTS, over two restarts and a ragged
    end -- the model is a sound yardstick there too"""
    for stride in (4, 6, 7):
        for i, seg in enumerate(FL.RESTARTS):
            m, t = 2 * seg + 3 * stride + 2, (0, esize - 1)[i & 1]
            d = SL.gen(SL.KINDS[(i + stride) % 5], esize, m, t, 13 * m + esize, stride)
            f = SL.forward(d, esize, filt, seg, stride)
            assert np.array_equal(f, SL.scalar_forward(d, esize, filt, seg, stride)), (stride, seg)
            assert np.array_equal(SL.inverse(f, esize, filt, seg, stride), d), (stride, seg)


@pytest.mark.parametrize("esize", SL.ESIZES)
@pytest.mark.parametrize("filt", SL.FILTERS)
def test_stride_one_is_the_filter_of_fplanes(esize, filt):
    for kind in FL.KINDS:
        for seg, m, t in ((256, 1, 0), (256, 700, esize - 1), (320, 961, 1), (4096, 4097, 0)):
            d = FL.gen(kind, esize, m, t, 7 * m + esize)
            f = FL.forward(d, esize, filt, seg)
            assert np.array_equal(SL.forward(d, esize, filt, seg, 1), f), (kind, seg, m, t)
            assert np.array_equal(SL.inverse(f, esize, filt, seg, 1), d), (kind, seg, m, t)


def test_model_equals_the_golden():
    golden = SL.load_golden()
    assert [g[0] for g in golden] == SL.golden_cases() and len(golden) >= 84
    assert {(g[0][0], g[0][1], g[0][2]) for g in golden} >= {(e, f, s) for e in SL.ESIZES for f in SL.FILTERS for s in SL.STRIDES}
    stored = 0
    for case, in_sha, out_sha, out in golden:
        esize, filt, stride, seg, m, t, kind = case
        d = SL.golden_input(case)
        assert SL.sha(d) == in_sha, ("the input generator changed", case)
        f = SL.forward(d, esize, filt, seg, stride)
        assert SL.sha(f) == out_sha, case
        if out is not None:
            stored += 1
            assert np.array_equal(f, out), case
        else:
            assert f.size > SL.GOLDEN_STORE_MAX
        assert np.array_equal(SL.inverse(f, esize, filt, seg, stride), d), case
    assert stored >= 30
    assert os.path.getsize(SL.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("stride", SL.STRIDES)
@pytest.mark.parametrize("filt", SL.FILTERS)
def test_restarts_really_restart(filt, stride):
    """changing element i changes F_S at i and i + S only, and never across a segment"""
    for esize in SL.ESIZES:
        seg, m = 256, 4 * 256 + 17
        d = SL.gen("interleaved", esize, m, esize - 1, 5, stride)
        f = SL.forward(d, esize, filt, seg, stride).copy()
        for i in (0, stride - 1, stride, 255, 256 - stride, 256, 300, 767, 1024, m - 1 - stride, m - 1):
            e = d.copy()
            e[i * esize] ^= 0x41
            g = SL.forward(e, esize, filt, seg, stride)
            changed = set(int(c) for c in np.flatnonzero((g != f)[:m * esize]) // esize)
            expect = {i} | ({i + stride} if i + stride < m and (i + stride) // seg == i // seg else set())
            assert changed == expect, (esize, i, sorted(changed))
            assert np.array_equal(g[m * esize:], f[m * esize:])
        # and a segment decodes from its own values alone
        x = SL.inverse(f[2 * seg * esize:3 * seg * esize], esize, filt, seg, stride)
        assert np.array_equal(x, d[2 * seg * esize:3 * seg * esize])


# ---- the stride's argument errors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", (0, 9, -1))
def test_a_bad_stride_is_the_first_error_of_every_new_call(stride):
    """TRC_E_ARG naming the stride, with NULL pointers and sizes of zero behind it, and without a device"""
    L = trc.lib()
    text = "stride %d" % stride
    for filt in (FL.NONE, FL.ZDELTA, FL.XOR):
        assert L.trc_planes_split_sfilter_dev(filt, stride, None, 0, 4, 256, None, 0, None, None) == -1 and text in err()
        assert L.trc_planes_join_sfilter_dev(filt, stride, None, 0, None, 0, 4, 256, None, None) == -1 and text in err()
        assert L.trc_encode_splanes_dev(trc.RCA, filt, stride, None, 0, 4, 256, None, 0, None, None, None, None, None, None, 0, None) == -1 and text in err()
        assert L.trc_decode_splanes_dev(trc.RCA, filt, stride, None, None, None, 0, 4, 256, None, 0, None, None, 0, None) == -1 and text in err()
        assert L.trc_decode_splanes_range_dev(trc.RCA, filt, stride, None, None, 0, 4, 256, 0, 1, None, 0, None, None, 0, None) == -1 and text in err()
        assert L.trc_encode_splanes_host(trc.RCA, filt, stride, None, 0, 4, 256, None, 0, 0) == 0 and text in err()
    for filters in (1, 2, 7):
        assert L.trc_planes_hist_stride_dev(filters, stride, None, 0, 4, 256, None, None) == -1 and text in err()


def test_good_strides_reach_the_next_check():
    """stride 1 .. 8 pass the stride's check: the next complaint is about something else, still without a device"""
    L = trc.lib()
    for stride in range(1, 9):
        assert L.trc_planes_split_sfilter_dev(3, stride, None, 0, 4, 256, None, 0, None, None) == -1 and "filter 3" in err()
        assert L.trc_planes_join_sfilter_dev(1, stride, None, 0, None, 0, 4, 100, None, None) == -1 and "restart length 100" in err()
        assert L.trc_planes_split_sfilter_dev(1, stride, None, 4096, 4, 256, None, 1024, None, None) == -1 and "aligned" in err()
        assert L.trc_encode_splanes_dev(trc.RCA, 3, stride, None, 0, 4, 256, None, 0, None, None, None, None, None, None, 0, None) == -1 and "filter 3" in err()
        assert L.trc_planes_hist_stride_dev(8, stride, None, 0, 4, 256, None, None) == -1 and "filters 0x8" in err()
        assert L.trc_planes_hist_stride_dev(7, stride, None, 4096, 3, 256, None, None) == -1 and "esize 3" in err()


def test_host_encode_takes_filter_1_or_2_and_stride_2_to_8():
    L = trc.lib()
    d = FL.gen("monotone", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    assert L.trc_encode_splanes_host(trc.RCA, FL.ZDELTA, 1, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
    assert "trc_encode_fplanes_host" in err()
    for filt in (FL.NONE, 3, -1):
        assert L.trc_encode_splanes_host(trc.RCA, filt, 2, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert "filter %d" % filt in err()
    with pytest.raises(trc.TrcError, match="trc_encode_fplanes_host"):
        trc.host_encode_splanes(trc.RCA, FL.XOR, 1, d, 4, 256)
    with pytest.raises(trc.TrcError, match="stride 9"):
        trc.host_encode_splanes(trc.RCA, FL.XOR, 9, d, 4, 256)
    assert (out == 0xA5).all()
    # the seven low-nibble coders are refused as everywhere in the planes family, before a device is looked for
    assert L.trc_encode_splanes_host(trc.RC4, FL.ZDELTA, 2, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
    assert "low four bits" in err()


def test_bound():
    L = trc.lib()
    for esize in SL.ESIZES:
        for n in (esize, 1000 * esize + esize - 1, 10**6 + 1):
            for chunk in (0, 256, 4096):
                for cdfnum in (0, 256):
                    assert L.trc_splanes_bound(n, esize, chunk, cdfnum) == L.trc_planes_bound(n, esize, chunk, cdfnum) + 16 > 16
        assert L.trc_splanes_bound(esize - 1, esize, 256, 0) == 0
        assert L.trc_splanes_bound(4096, esize, 100, 0) == 0
    assert L.trc_splanes_bound(4096, 3, 256, 0) == 0
    assert trc.splanes_bound(4096, 4, 256) == trc.planes_bound(4096, 4, 256) + 16


# ---- trc_splanes_check on hand-made containers ------------------------------------------------------------------------------
def wrap(inner, magic=trc.SPLANES_MAGIC, filt=FL.ZDELTA, version=1, stride=3, size=None):
    b = struct.pack("<IBBHQ", magic, filt, version, stride, 16 + len(inner) if size is None else size) + inner
    return np.frombuffer(b, dtype=np.uint8).copy()


def check(buf, buflen=None, outlen=ANY):
    return trc.lib().trc_splanes_check(buf.ctypes.data, buf.size if buflen is None else buflen, outlen)


@pytest.mark.parametrize("esize,t", [(2, 1), (4, 0), (8, 7)])
@pytest.mark.parametrize("filt", SL.FILTERS)
def test_check_accepts(esize, t, filt):
    inner, n = make(esize, t)
    for stride in SL.STRIDES:
        buf = wrap(inner, filt=filt, stride=stride)
        assert check(buf) == 0 and check(buf, outlen=n) == 0, err()
        trc.splanes_check(buf, n)
        assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
        assert trc.lib().trc_planes_check(buf[16:].ctypes.data, buf.size - 16, n) == 0        # the inner part is a TRCP container as it stands


def test_check_rejects_each_defect():
    inner, n = make(4, 1)
    good = wrap(inner)
    assert check(good) == 0
    assert check(wrap(inner, magic=trc.FPLANES_MAGIC)) != 0 and "magic" in err()         # TRCF
    assert check(wrap(inner, magic=trc.PLANES_MAGIC)) != 0 and "magic" in err()          # TRCP
    assert check(np.frombuffer(inner, dtype=np.uint8).copy()) != 0 and "magic" in err()  # a bare TRCP container
    assert check(np.random.default_rng(1).integers(0, 256, 400, dtype=np.uint8)) != 0 and "magic" in err()      # garbage
    assert check(wrap(inner, version=2)) != 0 and "version" in err()
    assert check(wrap(inner, filt=0)) != 0 and "filter 0" in err()
    assert check(wrap(inner, filt=3)) != 0 and "filter 3" in err()
    for stride in (0, 1, 9, 256, 65535):
        assert check(wrap(inner, stride=stride)) != 0 and "stride %d" % stride in err()
    assert check(wrap(inner, size=16 + len(inner) + 8)) != 0 and "buffer holds" in err()      # size > buflen
    assert check(good, buflen=good.size - 1) != 0 and "buffer holds" in err()
    assert check(wrap(inner, size=15)) != 0 and "size 15" in err()                       # size < 16
    assert check(wrap(inner, size=16)) != 0 and "size 16" in err()                       # no room for an inner container
    assert check(good, buflen=15) != 0 and "shorter than the header" in err()
    assert check(good, buflen=0) != 0 and "shorter than the header" in err()
    assert check(wrap(inner[:-9])) != 0 and "planes container" in err()                  # a truncated inner container
    assert check(wrap(inner, size=16 + len(inner) - 9)) != 0 and "planes container" in err()
    assert check(wrap(make(4, 1, version=2)[0])) != 0 and "planes container" in err()    # the TRCP version 2 stays rejected
    assert check(good, outlen=n - 1) != 0 and "caller expects" in err()                  # another length than the caller expects
    with pytest.raises(trc.TrcError, match="stride 9"):
        trc.splanes_check(wrap(inner, stride=9))
    # the decoders check first, before a device is looked for, and write nothing
    L = trc.lib()
    out = np.full(n + 64, 0xA5, dtype=np.uint8)
    bad = wrap(inner, stride=9)
    for name in ("trc_decode_splanes_host", "trc_decode_xplanes_host"):
        assert getattr(L, name)(bad.ctypes.data, bad.size, out.ctypes.data, n) == 0 and "stride 9" in err(), name
    assert L.trc_decode_splanes_range_host(bad.ctypes.data, bad.size, 0, 8, out.ctypes.data) == 0 and "stride 9" in err()
    assert L.trc_decode_splanes_host(good.ctypes.data, good.size, out.ctypes.data, n - 1) == 0 and "caller expects" in err()
    assert (out == 0xA5).all()


# ---- what the strides are for -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return SL.table_inputs()


def test_matching_stride_beats_stride_one_and_no_filter(table):
    """a property of the model: on interleaved series the order-0 estimate under zigzag delta with the matching stride is below both
    the stride-1 estimate and the unfiltered one, and trc_planes_advise, fed the histograms of F_S, chooses zigzag delta where on
    the stride-1 histograms it chooses no filter"""
    seg = 4096
    for name, esize, stride, d in table:
        m = d.size // esize
        h1, hs = SL.hist3(d, esize, seg, 1), SL.hist3(d, esize, seg, stride)
        rows = lambda h, f: h.reshape(3, esize, 256)[f]
        none, z1, zs = (SL.bits_per_byte(r, m, esize) for r in (rows(h1, 0), rows(h1, 1), rows(hs, 1)))
        print("%s: %d elements of %d bytes, bits per byte: no filter %.2f, zdelta stride 1 %.2f, zdelta stride %d %.2f" % (name, m, esize, none, z1, stride, zs))
        assert zs < none and zs < z1, name
        assert np.array_equal(rows(h1, 0), rows(hs, 0)), "the unfiltered row does not depend on the stride"
        a1, as_ = trc.planes_advise(h1, 7, esize, m), trc.planes_advise(hs, 7, esize, m)
        assert a1["filter"] == trc.FILTER_NONE, name
        assert as_["filter"] == trc.FILTER_ZDELTA, name
        assert as_["total_bits"][1] < a1["total_bits"][1] and as_["total_bits"][1] < a1["total_bits"][0]
        assert abs(as_["total_bits"][1] / (8.0 * m * esize) - zs / 8.0) < 1e-9


# ---- the harness --------------------------------------------------------------------------------------------------------------
def test_trcfile_compiles_against_headers_and_knows_the_mode(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "harness", "trcfile.c")).read()
    assert "trc_encode_splanes_host" in src and "trc_splanes_check" in src and "trc_decode_splanes_range_host" in src
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2 and "trcfile s <id> <esize> <z|x> <stride> <in> <out>" in u.stderr
    d = tmp_path / "in.bin"
    SL.table_rows(100).tofile(str(d))
    for stride in ("1", "9", "0"):                              # refused before the library is asked
        r = subprocess.run([str(exe), "s", "46", "4", "z", stride, str(d), str(tmp_path / "o")], capture_output=True, text=True)
        assert r.returncode == 2 and "stride" in r.stderr
