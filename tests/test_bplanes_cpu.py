"""Byte planes against a base buffer, the parts that need no GPU: the declarations and exports, the header struct through a C
compiler and ctypes, the numpy model (bplanes_lib) against a scalar restatement of the definition, trc_base_fingerprint_host against
the model, trc_bplanes_check on containers assembled by hand, the bound, what the host calls do without a device, the advisor on
model histograms, the order-0 gain the README quotes, and harness/trcfile.c against the headers."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import advise_lib as AL
import bplanes_lib as BP
import planes_lib as PL
import trc
from planes_matrix_lib import LOW4, LOW4_TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
SYMBOLS = ("trc_planes_split_base_dev", "trc_planes_join_base_dev", "trc_encode_bplanes_dev", "trc_decode_bplanes_dev",
           "trc_decode_bplanes_range_dev", "trc_planes_hist_base_dev", "trc_base_fingerprint_dev", "trc_base_fingerprint_host",
           "trc_bplanes_bound", "trc_encode_bplanes_host", "trc_decode_bplanes_host", "trc_decode_bplanes_range_host", "trc_bplanes_check")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = header_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("planes_split_base", "planes_join_base", "BasePlanesCoder", "planes_hist_base", "base_fingerprint", "base_fingerprint_host",
                 "bplanes_bound", "host_encode_bplanes", "host_decode_bplanes", "host_decode_bplanes_range", "bplanes_check"):
        assert hasattr(trc, name), name


def test_header_struct(tmp_path):
    """sizeof(trc_bplanes_hdr) == 32 with the fields where the format puts them: read from the header by a C compiler, and through
    ctypes from a struct laid out as the header declares it"""
    txt = header_text()
    assert re.search(r"#define\s+TRC_BPLANES_MAGIC\s+0x44435254u", txt)
    assert struct.pack("<I", trc.BPLANES_MAGIC) == b"TRCD"
    body = re.search(r"typedef struct trc_bplanes_hdr \{(.*?)\} trc_bplanes_hdr;", txt, flags=re.S).group(1)
    fields = re.findall(r"(uint\d+_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "magic"), ("uint8_t", "filter"), ("uint8_t", "version"), ("uint16_t", "zero"), ("uint64_t", "size"),
                      ("uint64_t", "base_bytes"), ("uint64_t", "base_fp")]
    ct = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}

    class Hdr(C.Structure):
        _fields_ = [(n, ct[t]) for t, n in fields]
    assert C.sizeof(Hdr) == 32 == trc.BPLANES_HDR
    assert [getattr(Hdr, n).offset for _, n in fields] == [0, 4, 5, 6, 8, 16, 24]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(trc_bplanes_hdr), '
                   'offsetof(trc_bplanes_hdr, size), offsetof(trc_bplanes_hdr, base_bytes), offsetof(trc_bplanes_hdr, base_fp)); return 0; }\n')
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["32", "8", "16", "24"]


# ---- the model ------------------------------------------------------------------------------------------------------------
def scalar_forward(data, base, esize, filt):
    """the definition, one element at a time in Python integers"""
    w, mask = 8 * esize, (1 << (8 * esize)) - 1
    m = len(data) // esize
    out = bytearray()
    for i in range(m):
        x = int.from_bytes(bytes(data[i * esize:(i + 1) * esize]), "little")
        b = int.from_bytes(bytes(base[i * esize:(i + 1) * esize]), "little")
        if filt == BP.XOR:
            y = x ^ b
        else:
            d = (x - b) & mask
            y = ((d << 1) ^ (0 - (d >> (w - 1)))) & mask
        out += y.to_bytes(esize, "little")
    return np.frombuffer(bytes(out) + bytes(data[m * esize:]), dtype=np.uint8)


@pytest.mark.parametrize("esize", BP.ESIZES)
@pytest.mark.parametrize("filt", BP.FILTERS)
def test_model_is_the_definition_and_round_trips(esize, filt):
    for kind in BP.KINDS:
        for m, t in ((1, 0), (700, esize - 1), (961, 1)):
            d, b = BP.gen_pair(kind, esize, m, t, 11 * m + esize)
            assert d.size == m * esize + t and b.size == m * esize
            f = BP.forward(d, b, esize, filt)
            assert f.dtype == np.uint8 and f.size == d.size
            assert np.array_equal(f, scalar_forward(d, b, esize, filt)), (kind, m, t)
            assert np.array_equal(f[m * esize:], d[m * esize:]), "the tail bytes are not filtered"
            assert np.array_equal(BP.inverse(f, b, esize, filt), d), (kind, m, t)
            if kind == "same":
                assert not f[:m * esize].any(), "data == base: every plane is zero"
            # a longer base is read up to m * esize bytes only
            assert np.array_equal(BP.forward(d, np.concatenate([b, b[:5] ^ 0xFF]), esize, filt), f)


def test_wrap_pairs_reach_every_corner():
    for esize in BP.ESIZES:
        w = 8 * esize
        d, b = BP.gen_pair("wrap", esize, 64, 0, 3)
        y = set(int(v) for v in BP.forward(d, b, esize, BP.ZDELTA).view(BP.DT[esize]))
        assert {0, 1, 2, (1 << w) - 1, (1 << w) - 2} <= y, (esize, sorted(y))


def test_pair_starts_from_the_weights():
    for esize in BP.ESIZES:
        base, data = BP.pair(4096, esize, 7, 1e-4)
        assert np.array_equal(base, PL.weights(4096, esize, 7))
        assert data.size == base.size and not np.array_equal(data, base)


# ---- the fingerprint ------------------------------------------------------------------------------------------------------
def fp_host(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return int(trc.lib().trc_base_fingerprint_host(a.ctypes.data, a.size))


def test_fingerprint_host_is_the_model():
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 8, 9, 4097):
        a = rng.integers(0, 256, n, dtype=np.uint8)
        exp = (sum((2 * j + 1) * int.from_bytes(bytes(a[8 * j:8 * j + 8]), "little") for j in range(-(-n // 8))) + n * 0x9E3779B97F4A7C15) % 2**64
        assert BP.fingerprint(a) == exp, n
        assert fp_host(a) == exp == trc.base_fingerprint_host(a), n
        for i in range(n):                                         # any single-byte change
            c = a.copy()
            c[i] ^= 1 << (i % 8)
            assert fp_host(c) != exp, (n, i)
    big = rng.integers(0, 256, 100003, dtype=np.uint8)             # the model's array path against its word-by-word path
    assert BP.fingerprint(big) == fp_host(big)
    assert BP.fingerprint(big[:4096]) == fp_host(big[:4096])
    # two unequal words swapped; zeros of another length
    a = rng.integers(0, 256, 64, dtype=np.uint8)
    s = a.copy()
    s[8:16], s[40:48] = a[40:48], a[8:16]
    assert fp_host(s) != fp_host(a)
    assert len({fp_host(np.zeros(n, np.uint8)) for n in range(20)}) == 20


# ---- trc_bplanes_check on hand-made containers ------------------------------------------------------------------------------
def section(codec, m, chunk, clens, cdfnum=0):
    lens = [min(chunk, m - i * chunk) for i in range(len(clens))]
    pay = sum(min(l, ln) for l, ln in zip(clens, lens))
    hdr = struct.pack("<IBBHIIQQ", 0x31435254, codec, 1, cdfnum, chunk, len(clens), m, pay)
    return hdr + struct.pack("<%dI" % len(clens), *clens) + bytes(range(256)) * (pay // 256) + bytes(range(pay % 256))


def make(esize=2, t=0, codec=trc.RCA, m=600, chunk=256, clens=(256, 40, 9), version=1, cdfnum=0):
    """a TRCP container of a non-static coder: header, offsets, esize sections (each 8-aligned), t tail bytes"""
    n = m * esize + t
    pos, off, body = 32 + 8 * esize, [], b""
    for _ in range(esize):
        s = section(codec, m, chunk, clens, cdfnum)
        off.append(pos)
        s = s + b"\0" * (-len(s) % 8)
        body += s
        pos += len(s)
    hdr = struct.pack("<IBBBBIIQQ", trc.PLANES_MAGIC, codec, version, esize, t, chunk, cdfnum, n, pos + t)
    return hdr + struct.pack("<%dQ" % esize, *off) + body + bytes([0xEE] * t), n


def wrap(inner, n, esize, magic=trc.BPLANES_MAGIC, filt=BP.ZDELTA, version=1, zero=0, size=None, base_bytes=None, fp=0x1122334455667788):
    bb = n - n % esize if base_bytes is None else base_bytes
    b = struct.pack("<IBBHQQQ", magic, filt, version, zero, 32 + len(inner) if size is None else size, bb, fp) + inner
    return np.frombuffer(b, dtype=np.uint8).copy()


def check(buf, buflen=None, outlen=ANY):
    return trc.lib().trc_bplanes_check(buf.ctypes.data, buf.size if buflen is None else buflen, outlen)


@pytest.mark.parametrize("esize,t", [(2, 1), (4, 0), (8, 7)])
@pytest.mark.parametrize("filt", BP.FILTERS)
def test_check_accepts(esize, t, filt):
    inner, n = make(esize, t)
    buf = wrap(inner, n, esize, filt=filt)
    assert check(buf) == 0 and check(buf, outlen=n) == 0, err()
    trc.bplanes_check(buf, n)
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0
    assert trc.lib().trc_planes_check(buf[32:].ctypes.data, buf.size - 32, n) == 0        # the inner part is a TRCP container as it stands


def test_check_rejects_each_defect():
    inner, n = make(4, 1)
    good = wrap(inner, n, 4)
    assert check(good) == 0
    assert check(wrap(inner, n, 4, magic=trc.FPLANES_MAGIC)) != 0 and "magic" in err()
    assert check(np.frombuffer(inner, dtype=np.uint8).copy()) != 0 and "magic" in err()  # a bare TRCP container
    assert check(wrap(inner, n, 4, version=2)) != 0 and "version" in err()
    assert check(wrap(inner, n, 4, filt=0)) != 0 and "filter 0" in err()
    assert check(wrap(inner, n, 4, filt=3)) != 0 and "filter 3" in err()
    assert check(wrap(inner, n, 4, zero=1)) != 0 and "reserved" in err()
    assert check(wrap(inner, n, 4, size=32 + len(inner) + 8)) != 0 and "buffer holds" in err()     # size > buflen
    assert check(good, buflen=good.size - 1) != 0 and "buffer holds" in err()
    assert check(wrap(inner, n, 4, size=31)) != 0 and "size 31" in err()
    assert check(wrap(inner, n, 4, size=32)) != 0 and "size 32" in err()                  # no room for an inner container
    assert check(good, buflen=31) != 0 and "shorter than the header" in err()
    assert check(wrap(inner, n, 4, base_bytes=n - 1 - 4)) != 0 and "base_bytes" in err()  # one element short
    assert check(wrap(inner, n, 4, base_bytes=n - 1 + 4)) != 0 and "base_bytes" in err()  # one element long
    assert check(wrap(inner, n, 4, base_bytes=n)) != 0 and "base_bytes" in err()          # the tail is not part of the base
    assert check(wrap(inner[:-9], n, 4)) != 0 and "planes container" in err()             # a truncated inner container
    assert check(wrap(make(4, 1, version=2)[0], n, 4)) != 0 and "planes container" in err()
    assert check(good, outlen=n - 1) != 0 and "caller expects" in err()
    low4 = LOW4[0]
    inner4, n4 = make(4, 1, codec=low4, cdfnum=trc.ss_prm((4, 7)) if low4 in trc.SSBIT else 0)
    assert check(wrap(inner4, n4, 4)) != 0 and LOW4_TEXT in err()
    with pytest.raises(trc.TrcError, match="filter 3"):
        trc.bplanes_check(wrap(inner, n, 4, filt=3))
    # the order: a bad prefix is named ahead of a bad inner container, the inner container ahead of base_bytes
    assert check(wrap(inner[:-9], n, 4, zero=1)) != 0 and "reserved" in err()
    assert check(wrap(inner[:-9], n, 4, base_bytes=0)) != 0 and "planes container" in err()


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_low_nibble_coders_are_refused_before_any_device(codec):
    L = trc.lib()
    prm = trc.ss_prm((4, 7)) if codec in trc.SSBIT else 0
    inner, n = make(4, 3, codec=codec, cdfnum=prm)
    buf = wrap(inner, n, 4)
    base = np.zeros(n, np.uint8)
    out = np.full(n + 64, 0xA5, dtype=np.uint8)
    assert check(buf) != 0 and LOW4_TEXT in err() and "codec %d" % codec in err()
    assert L.trc_decode_bplanes_host(buf.ctypes.data, buf.size, base.ctypes.data, base.size, out.ctypes.data, n) == 0 and LOW4_TEXT in err()
    assert L.trc_decode_bplanes_range_host(buf.ctypes.data, buf.size, base.ctypes.data, base.size, 0, 8, out.ctypes.data) == 0 and LOW4_TEXT in err()
    comp = np.full(n + 4096, 0xA5, dtype=np.uint8)
    assert L.trc_encode_bplanes_host(codec, BP.XOR, base.ctypes.data, base.ctypes.data, n, 4, 256, comp.ctypes.data, comp.size, prm) == 0
    assert LOW4_TEXT in err()
    assert (out == 0xA5).all() and (comp == 0xA5).all()


def test_bound():
    L = trc.lib()
    for esize in BP.ESIZES:
        for n in (esize, 1000 * esize + esize - 1, 10**6 + 1):
            for chunk in (0, 256, 4096):
                for cdfnum in (0, 256):
                    assert L.trc_bplanes_bound(n, esize, chunk, cdfnum) == L.trc_planes_bound(n, esize, chunk, cdfnum) + 32 > 32
        assert L.trc_bplanes_bound(esize - 1, esize, 256, 0) == 0
        assert L.trc_bplanes_bound(4096, esize, 100, 0) == 0
    assert L.trc_bplanes_bound(4096, 3, 256, 0) == 0
    assert trc.bplanes_bound(4096, 4, 256) == trc.planes_bound(4096, 4, 256) + 32


# ---- without a device ---------------------------------------------------------------------------------------------------------
def _no_gpu():
    try:
        return trc.lib().trc_device_count() == 0
    except Exception:
        return False


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible: the calls would succeed")
def test_host_calls_without_a_device_return_zero_and_say_why():
    L = trc.lib()
    d, b = BP.gen_pair("drift", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for filt in BP.FILTERS:
        assert L.trc_encode_bplanes_host(trc.RCA, filt, d.ctypes.data, b.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert "no HIP device" in err()
        assert (out == 0xA5).all(), "encode wrote to its output"
        with pytest.raises(trc.TrcError, match="no HIP device"):
            trc.host_encode_bplanes(trc.RCA, filt, d, b, 4, 256)
    inner, n = make(4, 1)
    buf = wrap(inner, n, 4)
    base = np.zeros(n, np.uint8)
    assert L.trc_decode_bplanes_host(buf.ctypes.data, buf.size, base.ctypes.data, base.size, out.ctypes.data, n) == 0 and "no HIP device" in err()
    assert L.trc_decode_bplanes_range_host(buf.ctypes.data, buf.size, base.ctypes.data, base.size, 5, 100, out.ctypes.data) == 0 and "no HIP device" in err()
    assert (out == 0xA5).all(), "a decoder wrote to its output"
    with pytest.raises(trc.TrcError, match="no HIP device"):
        trc.host_decode_bplanes(buf, base, n)


def test_argument_errors_need_no_device():
    """what is wrong with the arguments or the container is said before a device is looked for"""
    L = trc.lib()
    d, b = BP.gen_pair("drift", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for filt in (BP.NONE, 3, -1):
        assert L.trc_encode_bplanes_host(trc.RCA, filt, d.ctypes.data, b.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert "filter %d" % filt in err()
    assert "trc_encode_planes_host" in err()                          # (the last one names where unfiltered data goes, as all do)
    assert L.trc_encode_bplanes_host(trc.RCA, BP.XOR, d.ctypes.data, None, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0 and "base" in err()
    inner, n = make(4, 1)
    base = np.zeros(n, np.uint8)
    bad = wrap(inner, n, 4, filt=3)
    assert L.trc_decode_bplanes_host(bad.ctypes.data, bad.size, base.ctypes.data, base.size, out.ctypes.data, n) == 0 and "filter 3" in err()
    assert L.trc_decode_bplanes_range_host(bad.ctypes.data, bad.size, base.ctypes.data, base.size, 0, 10, out.ctypes.data) == 0 and "filter 3" in err()
    good = wrap(inner, n, 4)
    assert L.trc_decode_bplanes_host(good.ctypes.data, good.size, base.ctypes.data, base.size, out.ctypes.data, n - 1) == 0 and "caller expects" in err()
    assert L.trc_decode_bplanes_host(good.ctypes.data, good.size, base.ctypes.data, n - 1 - 1, out.ctypes.data, n) == 0 and "the base holds" in err()
    assert L.trc_decode_bplanes_range_host(good.ctypes.data, good.size, base.ctypes.data, n - 1 - 1, 0, 10, out.ctypes.data) == 0 and "the base holds" in err()
    # the device calls name a bad filter ahead of everything else, pointers included
    for name, args in (("trc_planes_split_base_dev", (None, None, 64, 4, None, 256, None, None)),
                       ("trc_planes_join_base_dev", (None, 256, None, None, 64, 4, None, None))):
        for filt in (-1, 3):
            assert getattr(L, name)(filt, *args) == -1 and "filter %d" % filt in err(), name
    # trc_decode_xplanes_host has no base to give
    assert L.trc_decode_xplanes_host(good.ctypes.data, good.size, out.ctypes.data, n) == 0 and "trc_decode_bplanes_host" in err()
    assert (out == 0xA5).all()


# ---- the advisor and the gain -----------------------------------------------------------------------------------------------
def test_advisor_picks_the_delta_for_a_fine_tune_and_nothing_for_strangers():
    base, data = BP.pair(1 << 16, 2, 7, 1e-4)
    h = BP.hist(data, base, 2, AL.ALL)
    assert np.array_equal(h[0], AL.hist(data, 2, 256, 1)[0]), "row 0 is the unfiltered row"
    a = trc.planes_advise(h, AL.ALL, 2, 1 << 16)
    assert a["filter"] == BP.ZDELTA == AL.advise(h, AL.ALL, 2, 1 << 16)[0], a["total_bits"]
    d, b = BP.gen_pair("random", 4, 1 << 16, 0, 9)
    h = BP.hist(d, b, 4, AL.ALL)
    a = trc.planes_advise(h, AL.ALL, 4, 1 << 16)
    assert a["filter"] == BP.NONE, a["total_bits"]                  # (the 1/64 rule: the totals differ by noise only)


def test_order0_gain_of_a_bf16_fine_tune():
    """what the README quotes: 2^20 bf16 weights against the same weights plus N(0, (1e-4)^2) noise cost 0.339 of their size under
    the zigzag delta against the base, by the order-0 estimate of the planes"""
    m = 1 << 20
    base, data = BP.pair(m, 2, 7, 1e-4)
    ratio = BP.order0_bytes(BP.forward(data, base, 2, BP.ZDELTA), 2) / data.size
    assert ratio < 0.40, ratio
    assert ratio < BP.order0_bytes(BP.forward(data, base, 2, BP.XOR), 2) / data.size < BP.order0_bytes(data, 2) / data.size


# ---- the harness --------------------------------------------------------------------------------------------------------------
def test_trcfile_compiles_against_headers(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "harness", "trcfile.c")).read()
    assert "trc_encode_bplanes_host" in src and "trc_decode_bplanes_host" in src
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2 and "trcfile r <id> <esize> <z|x> <base> <in> <out>" in u.stderr and "trcfile R <in> <base> <out>" in u.stderr
