"""Byte-plane containers, the parts that need no GPU: the declarations and exports, the size functions, trc_planes_check on
containers assembled by hand, and the numpy definition of the split against the reference's tpenc (tests/golden/planes_vectors.npz,
made by tests/golden/make_planes_golden.py through the compiled reference)."""
import os
import re
import struct

import numpy as np
import pytest

import planes_lib as PL
import trc
from planes_matrix_lib import ASSIGNED, LOW4, LOW4_TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
SYMBOLS = ("trc_planes_pitch", "trc_planes_split_dev", "trc_planes_join_dev", "trc_planes_work_bytes", "trc_encode_planes_dev",
           "trc_decode_planes_dev", "trc_planes_range_work_bytes", "trc_decode_planes_range_dev", "trc_planes_bound",
           "trc_encode_planes_host", "trc_decode_planes_host", "trc_decode_planes_range_host", "trc_planes_check")


def test_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    assert re.search(r"#define\s+TRC_PLANES_CDF_STRIDE\s+264\b", txt)
    for name in ("planes_split", "planes_join", "PlanesCoder", "host_encode_planes", "host_decode_planes", "host_decode_planes_range",
                 "planes_check", "parse_planes"):
        assert hasattr(trc, name), name


def test_pitch():
    L = trc.lib()
    for esize in PL.ESIZES:
        for n in (esize, esize + 1, 255 * esize, 256 * esize, 257 * esize + esize - 1, 10**6 + 3, 5 * 2**30 + 1):
            p = L.trc_planes_pitch(n, esize)
            m = n // esize
            assert p % 256 == 0 and m + trc.PAD <= p < m + trc.PAD + 256, (n, esize, p)
        assert L.trc_planes_pitch(esize - 1, esize) == 0       # no whole element
        assert L.trc_planes_pitch(0, esize) == 0
    for esize in (0, 1, 3, 5, 16):
        assert L.trc_planes_pitch(4096, esize) == 0


def test_work_bytes():
    L = trc.lib()
    for codec in (trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS):
        for esize in PL.ESIZES:
            for n, chunk in ((esize, 256), (1000 * esize + esize - 1, 256), (10**6, 4096)):
                m = n // esize
                w = L.trc_planes_work_bytes(codec, n, esize, chunk)
                one = L.trc_work_bytes(codec, m, chunk)
                assert w % 256 == 0 and w >= esize * (one + L.trc_planes_pitch(n, esize)), (codec, n, esize, chunk)
                nc = trc.nchunks(m, chunk)
                for count in sorted({1, nc}):
                    r = L.trc_planes_range_work_bytes(codec, n, esize, chunk, count)
                    assert r % 256 == 0 and r >= esize * (L.trc_range_work_bytes(codec, m, chunk, count) + count * chunk + trc.PAD)
                assert L.trc_planes_range_work_bytes(codec, n, esize, chunk, 0) == 0
                assert L.trc_planes_range_work_bytes(codec, n, esize, chunk, nc + 1) == 0
    # what the calls reject: a bad esize, no whole element, a bad chunk, an id without a coder, a flag in the id
    for args in ((trc.RCA, 4096, 3, 256), (trc.RCA, 1, 2, 256), (trc.RCA, 4096, 2, 100), (trc.RCA, 4096, 2, 0), (42, 4096, 2, 256),
                 (trc.RCA | trc.TABLES_READY, 4096, 2, 256), (trc.RCA | trc.DIR_READY, 4096, 2, 256), (trc.ANSB, 1 << 20, 2, 16384)):
        assert L.trc_planes_work_bytes(*args) == 0, args
        assert L.trc_planes_range_work_bytes(*args, 1) == 0, args


def test_bound():
    L = trc.lib()
    for esize in PL.ESIZES:
        for n in (esize, 1000 * esize + esize - 1, 10**6 + 1):
            m = n // esize
            for chunk in (256, 4096):
                for cdfnum in (0, 256):
                    b = L.trc_planes_bound(n, esize, chunk, cdfnum)
                    sec = ((2 * (cdfnum + 1) + 7) & ~7 if cdfnum else 0) + 32 + 4 * trc.nchunks(m, chunk) + m   # every chunk stored raw
                    assert b >= 32 + 8 * esize + esize * ((sec + 7) & ~7) + n % esize, (n, esize, chunk, cdfnum)
                    assert b <= n + esize * (4 * trc.nchunks(m, chunk) + 600) + 128
            assert L.trc_planes_bound(n, esize, 0, 0) >= L.trc_planes_bound(n, esize, 256, 0)      # chunk 0: any chunk
        assert L.trc_planes_bound(esize - 1, esize, 256, 0) == 0
        assert L.trc_planes_bound(4096, esize, 100, 0) == 0
    assert L.trc_planes_bound(4096, 3, 256, 0) == 0


# ---- trc_planes_check on hand-made containers -------------------------------------------------------------------------------
def section(codec, m, chunk, clens, cdfnum=0):
    lens = [min(chunk, m - i * chunk) for i in range(len(clens))]
    pay = sum(min(l, ln) for l, ln in zip(clens, lens))
    hdr = struct.pack("<IBBHIIQQ", 0x31435254, codec, 1, cdfnum, chunk, len(clens), m, pay)
    return hdr + struct.pack("<%dI" % len(clens), *clens) + bytes(range(256)) * (pay // 256) + bytes(range(pay % 256))


def make(esize=2, t=0, codec=trc.RCA, m=600, chunk=256, clens=(256, 40, 9), magic=trc.PLANES_MAGIC, version=1, hdr_esize=None,
         hdr_tail=None, size_delta=0, off_delta=None, sections=None, cdfnum=0):
    """a TRCP container of a non-static coder: header, offsets, esize sections (each 8-aligned), t tail bytes; cdfnum: the two
    parameters of an ss coder, in the header and in every section"""
    n = m * esize + t
    secs = sections or [section(codec, m, chunk, clens, cdfnum)] * esize
    pos, off, body = 32 + 8 * esize, [], b""
    for s in secs:
        off.append(pos)
        s = s + b"\0" * (-len(s) % 8)
        body += s
        pos += len(s)
    if off_delta:
        off[off_delta[0]] += off_delta[1]
    size = pos + t + size_delta
    hdr = struct.pack("<IBBBBIIQQ", magic, codec, version, esize if hdr_esize is None else hdr_esize, t if hdr_tail is None else hdr_tail,
                      chunk, cdfnum, n, size)
    return np.frombuffer(hdr + struct.pack("<%dQ" % esize, *off) + body + bytes([0xEE] * t), dtype=np.uint8).copy(), n


def check(buf, buflen=None, outlen=ANY):
    return trc.lib().trc_planes_check(buf.ctypes.data, buf.size if buflen is None else buflen, outlen)


@pytest.mark.parametrize("esize,t", [(2, 0), (2, 1), (4, 0), (4, 1)])
def test_check_accepts(esize, t):
    buf, n = make(esize, t)
    assert n % esize == t
    assert check(buf) == 0 and check(buf, outlen=n) == 0
    trc.planes_check(buf, n)
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
    hdr, sections, tail = trc.parse_planes(buf)
    assert (hdr["esize"], hdr["tail"], hdr["n"], hdr["size"], hdr["chunk"]) == (esize, t, n, buf.size, 256)
    assert len(sections) == esize and all(c is None and bytes(s) == section(trc.RCA, 600, 256, (256, 40, 9)) for c, s in sections)
    assert bytes(tail) == bytes([0xEE] * t)


def err():
    return trc.lib().trc_last_error().decode()


def test_check_rejects_each_defect():
    good, n = make(4, 1)
    assert check(good) == 0
    assert check(make(4, 1, magic=0x31435254)[0]) != 0 and "container" in err()      # the TRC1 magic is not this container's
    assert check(make(4, 1, version=2)[0]) != 0
    assert check(make(4, 1, hdr_esize=3)[0]) != 0 and "esize" in err()
    assert check(make(4, 1, hdr_tail=2)[0]) != 0 and "tail" in err()
    assert check(make(4, 1, size_delta=8)[0]) != 0 and "container" in err()          # size > buflen
    assert check(make(4, 1, off_delta=(2, 4))[0]) != 0 and "multiple of 8" in err()  # an unaligned offset
    big = make(4, 1, off_delta=(2, -400))[0]                                         # a decreasing offset: section 2 before section 1
    assert check(big) != 0 and "offset" in err()
    assert check(make(4, 1, off_delta=(3, 1 << 20))[0]) != 0 and "offset" in err()   # an offset outside the container
    bad_dir = section(trc.RCA, 600, 256, (256, 40, 9))
    bad_dir = bad_dir[:24] + struct.pack("<Q", 304) + bad_dir[32:]                   # header says 304 payload bytes, the directory 305
    assert check(make(4, 1, sections=[section(trc.RCA, 600, 256, (256, 40, 9))] * 3 + [bad_dir])[0]) != 0 and "section 3" in err()
    assert "container" in err()
    assert check(good, buflen=good.size - 1) != 0                                    # a truncated buffer
    assert check(good, buflen=31) != 0
    assert check(good, outlen=n - 1) != 0                                            # another length than the caller expects
    other = section(trc.RCA, 600, 512, (40, 9))                                      # a section at another chunk than the header's
    assert check(make(2, 0, sections=[other, other])[0]) != 0
    assert check(make(2, 0, sections=[section(trc.RCB, 600, 256, (256, 40, 9))] * 2)[0]) != 0       # ... of another coder
    assert check(make(2, 0, sections=[section(trc.RCA, 601, 256, (256, 40, 9))] * 2)[0]) != 0       # ... of another length
    with pytest.raises(trc.TrcError, match="container"):
        trc.planes_check(good[:100])


def test_check_static_and_ss_fields():
    """a static coder's section opens with its CDF (strictly increasing, ending at 32768); an ss coder's cdfnum holds two parameters"""
    m, chunk, clens = 600, 256, (256, 40, 9)

    def static(cdf, cdfnum=4):
        sec = section(trc.ANS4S, m, chunk, clens)
        sec = sec[:6] + struct.pack("<H", cdfnum) + sec[8:]
        table = struct.pack("<%dH" % (cdfnum + 1), *cdf)
        table += b"\0" * (-len(table) % 8)
        body = (table + sec + b"\0" * (-len(sec) % 8)) * 2
        size = 48 + len(body)
        hdr = struct.pack("<IBBBBIIQQ", trc.PLANES_MAGIC, trc.ANS4S, 1, 2, 0, chunk, cdfnum, 2 * m, size)
        return np.frombuffer(hdr + struct.pack("<2Q", 48, 48 + len(body) // 2) + body, dtype=np.uint8).copy()
    assert check(static((0, 100, 200, 300, 32768))) == 0
    assert check(static((0, 100, 100, 300, 32768))) != 0 and "CDF" in err()
    assert check(static((0, 100, 200, 300, 32767))) != 0 and "CDF" in err()
    assert check(static((1, 100, 200, 300, 32768))) != 0

    def ss(prm):
        sec = section(trc.RCSS, m, chunk, clens)
        sec = sec[:6] + struct.pack("<H", prm) + sec[8:]
        sec += b"\0" * (-len(sec) % 8)
        hdr = struct.pack("<IBBBBIIQQ", trc.PLANES_MAGIC, trc.RCSS, 1, 2, 0, chunk, prm, 2 * m, 48 + 2 * len(sec))
        return np.frombuffer(hdr + struct.pack("<2Q", 48, 48 + len(sec)) + sec * 2, dtype=np.uint8).copy()
    assert check(ss(trc.ss_prm((4, 7)))) == 0
    assert check(ss(trc.ss_prm((0, 7)))) != 0
    assert check(ss(trc.ss_prm((4, 16)))) != 0


# ---- the low-nibble coders ------------------------------------------------------------------------------------------------------
def prm_of(codec):
    return trc.ss_prm((4, 7)) if codec in trc.SSBIT else 0


def test_work_bytes_of_every_coder():
    """the seven coders of in[i] & 15 have no planes workspace; every other assigned id has one"""
    L = trc.lib()
    assert len(LOW4) == 7 and set(LOW4) < set(ASSIGNED)
    for esize in PL.ESIZES:
        n = 4096 * esize + esize - 1
        for codec in ASSIGNED:
            w = L.trc_planes_work_bytes(codec, n, esize, 256)
            r = [L.trc_planes_range_work_bytes(codec, n, esize, 256, count) for count in (1, 16)]
            if codec in LOW4:
                assert w == 0 and r == [0, 0], (trc.CODEC_NAMES[codec], esize)
            else:
                assert w and all(r), (trc.CODEC_NAMES[codec], esize)
    for esize in PL.ESIZES:
        n = (1 << 20) * esize
        assert L.trc_planes_work_bytes(trc.ANSB, n, esize, 8192) and L.trc_planes_range_work_bytes(trc.ANSB, n, esize, 8192, 1)
        assert L.trc_planes_work_bytes(trc.ANSB, n, esize, 16384) == 0 and L.trc_planes_range_work_bytes(trc.ANSB, n, esize, 16384, 1) == 0


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_check_rejects_a_low_nibble_coder(codec):
    """a container that is well formed in every other respect: its planes would come back as in[i] & 15"""
    L = trc.lib()
    for esize, t in ((2, 1), (4, 0), (8, 7)):
        buf, n = make(esize, t, codec=codec, cdfnum=prm_of(codec))
        assert check(buf) != 0 and LOW4_TEXT in err(), trc.CODEC_NAMES[codec]
        assert "codec %d" % codec in err()
        with pytest.raises(trc.TrcError, match=LOW4_TEXT):
            trc.planes_check(buf, n)
        # the sections alone are sound TRC1 containers of that coder: nothing but the coder's kind is wrong
        for _, cont in trc.parse_planes(buf)[1]:
            assert L.trc_container_check(cont.ctypes.data, cont.size, codec, n // esize) == 0
        # every host decoder checks first, before a device is looked for
        out = np.full(n + 64, 0xA5, dtype=np.uint8)
        for name in ("trc_decode_planes_host", "trc_decode_xplanes_host"):
            assert getattr(L, name)(buf.ctypes.data, buf.size, out.ctypes.data, n) == 0 and LOW4_TEXT in err(), name
        assert L.trc_decode_planes_range_host(buf.ctypes.data, buf.size, 0, 8, out.ctypes.data) == 0 and LOW4_TEXT in err()
        assert (out == 0xA5).all()


@pytest.mark.parametrize("codec", (trc.RCU3, trc.RCU3SS), ids=lambda c: trc.CODEC_NAMES[c])
def test_check_accepts_the_varint_neighbours(codec):
    """rows of the same table macros as rc4s / rc4ss that code whole bytes"""
    for esize, t in ((2, 1), (4, 0), (8, 7)):
        buf, n = make(esize, t, codec=codec, cdfnum=prm_of(codec))
        assert check(buf) == 0 and check(buf, outlen=n) == 0, err()
        trc.planes_check(buf, n)


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_host_encode_refuses_a_low_nibble_coder_before_any_device(codec):
    """with or without a GPU: 0, the reason, and an untouched output"""
    L = trc.lib()
    d = PL.weights(3000, 2)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for chunk in (0, 256):
        assert L.trc_encode_planes_host(codec, d.ctypes.data, d.size, 2, chunk, out.ctypes.data, out.size, prm_of(codec)) == 0
        assert LOW4_TEXT in err() and "codec %d" % codec in err()
    assert (out == 0xA5).all()
    with pytest.raises(trc.TrcError, match=LOW4_TEXT):
        trc.host_encode_planes(codec, d, 2, 256, prm=(4, 7))


# ---- the definition against the reference ---------------------------------------------------------------------------------
def test_numpy_split_reproduces_the_reference_fixture():
    golden = PL.load_golden()
    assert sorted(golden) == sorted((e, n) for e in PL.ESIZES for n in PL.golden_lengths(e))
    for (esize, n), out in golden.items():
        assert n % (32 * esize) < esize and out.size == n <= 65536
        d = PL.golden_input(esize, n)
        assert np.array_equal(PL.flat(d, esize), out), (esize, n)
        planes, tail = PL.split(d, esize)
        assert planes.shape == (esize, n // esize) and tail.size == n % esize
        assert np.array_equal(PL.join(planes, tail), d)


def test_split_definition_on_odd_lengths():
    for esize in PL.ESIZES:
        for n in (esize, esize + 1, 7 * esize + esize - 1, 1001):
            d = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
            planes, tail = PL.split(d, esize)
            for k in range(esize):
                assert np.array_equal(planes[k], d[k:(n // esize) * esize:esize])
            assert np.array_equal(tail, d[(n // esize) * esize:])
            assert np.array_equal(PL.join(planes, tail), d)

