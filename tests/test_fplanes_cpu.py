"""Filtered byte planes, the parts that need no GPU: the declarations and exports, the header struct and enum through ctypes, the
numpy model of the two filters (fplanes_lib) against a scalar restatement of the definition and against its pinned fixture
tests/golden/fplanes_vectors.npz, trc_fplanes_check on containers assembled by hand, the bound, what the host calls do without a
device, and harness/trcfile.c against the headers."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fplanes_lib as FL
import trc
from planes_matrix_lib import LOW4, LOW4_TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
SYMBOLS = ("trc_planes_split_filter_dev", "trc_planes_join_filter_dev", "trc_encode_fplanes_dev", "trc_decode_fplanes_dev",
           "trc_decode_fplanes_range_dev", "trc_fplanes_bound", "trc_encode_fplanes_host", "trc_decode_fplanes_host",
           "trc_decode_fplanes_range_host", "trc_fplanes_check")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)


def test_symbols_declared_and_exported():
    txt = header_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("FILTER_NONE", "FILTER_ZDELTA", "FILTER_XOR", "planes_split_filter", "planes_join_filter", "FilteredPlanesCoder",
                 "host_encode_fplanes", "host_decode_fplanes", "host_decode_fplanes_range", "fplanes_check"):
        assert hasattr(trc, name), name


def test_header_struct_and_enum(tmp_path):
    """sizeof(trc_fplanes_hdr) == 16 with the fields where the format puts them, and the enum's values: read from the header by a C
    compiler, and through ctypes from a struct laid out as the header declares it"""
    txt = header_text()
    assert re.search(r"enum\s*\{\s*TRC_FILTER_NONE\s*=\s*0\s*,\s*TRC_FILTER_ZDELTA\s*=\s*1\s*,\s*TRC_FILTER_XOR\s*=\s*2\s*\}", txt)
    assert re.search(r"#define\s+TRC_FPLANES_MAGIC\s+0x46435254u", txt)
    assert (trc.FILTER_NONE, trc.FILTER_ZDELTA, trc.FILTER_XOR, trc.FPLANES_MAGIC) == (0, 1, 2, 0x46435254)
    assert struct.pack("<I", trc.FPLANES_MAGIC) == b"TRCF"
    body = re.search(r"typedef struct trc_fplanes_hdr \{(.*?)\} trc_fplanes_hdr;", txt, flags=re.S).group(1)
    fields = re.findall(r"(uint\d+_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "magic"), ("uint8_t", "filter"), ("uint8_t", "version"), ("uint16_t", "zero"), ("uint64_t", "size")]
    ct = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}

    class Hdr(C.Structure):
        _fields_ = [(n, ct[t]) for t, n in fields]
    assert C.sizeof(Hdr) == 16 == trc.FPLANES_HDR
    assert [getattr(Hdr, n).offset for _, n in fields] == [0, 4, 5, 6, 8]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu %zu %d %d %d\\n", sizeof(trc_fplanes_hdr), '
                   'offsetof(trc_fplanes_hdr, size), TRC_FILTER_NONE, TRC_FILTER_ZDELTA, TRC_FILTER_XOR); return 0; }\n')
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["16", "8", "0", "1", "2"]


# ---- the model ------------------------------------------------------------------------------------------------------------
def scalar_forward(data, esize, filt, seg):
    """the definition, one element at a time in Python integers"""
    w, mask = 8 * esize, (1 << (8 * esize)) - 1
    m = len(data) // esize
    out, prev = bytearray(), 0
    for i in range(m):
        x = int.from_bytes(bytes(data[i * esize:(i + 1) * esize]), "little")
        p = 0 if i % seg == 0 else prev
        if filt == FL.XOR:
            y = x ^ p
        else:
            d = (x - p) & mask
            y = ((d << 1) ^ (0 - (d >> (w - 1)))) & mask
        out += y.to_bytes(esize, "little")
        prev = x
    return np.frombuffer(bytes(out) + bytes(data[m * esize:]), dtype=np.uint8)


@pytest.mark.parametrize("esize", FL.ESIZES)
@pytest.mark.parametrize("filt", FL.FILTERS)
def test_model_is_the_definition_and_round_trips(esize, filt):
    for kind in FL.KINDS:
        for seg, m, t in ((256, 1, 0), (256, 700, esize - 1), (320, 961, 1)):
            d = FL.gen(kind, esize, m, t, 11 * m + esize)
            f = FL.forward(d, esize, filt, seg)
            assert f.dtype == np.uint8 and f.size == d.size
            assert np.array_equal(f, scalar_forward(d, esize, filt, seg)), (kind, seg, m, t)
            assert np.array_equal(f[m * esize:], d[m * esize:]), "the tail bytes are not filtered"
            assert np.array_equal(FL.inverse(f, esize, filt, seg), d), (kind, seg, m, t)


def test_wrap_inputs_reach_every_corner():
    """the wrap inputs take x - p through 0, +-1, +-2^(w-1) and the largest magnitudes, so the zigzag gives 0, 1, 2, 2^w - 1, 2^w - 2"""
    for esize in FL.ESIZES:
        w = 8 * esize
        d = FL.gen("wrap", esize, 64, 0, 3)
        y = set(int(v) for v in FL.forward(d, esize, FL.ZDELTA, 256).view(FL.DT[esize]))
        assert {0, 1, 2, (1 << w) - 1, (1 << w) - 2} <= y, (esize, sorted(y))


def test_model_equals_the_golden():
    golden = FL.load_golden()
    assert [g[0] for g in golden] == FL.golden_cases() and len(golden) >= 36
    stored = 0
    for case, in_sha, out_sha, out in golden:
        esize, filt, seg, m, t, kind = case
        d = FL.golden_input(case)
        assert FL.sha(d) == in_sha, ("the input generator changed", case)
        f = FL.forward(d, esize, filt, seg)
        assert FL.sha(f) == out_sha, case
        if out is not None:
            stored += 1
            assert np.array_equal(f, out), case
        else:
            assert f.size > FL.GOLDEN_STORE_MAX
        assert np.array_equal(FL.inverse(f, esize, filt, seg), d), case
    assert stored >= 12
    assert os.path.getsize(FL.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("esize", FL.ESIZES)
@pytest.mark.parametrize("filt", FL.FILTERS)
def test_restarts_really_restart(esize, filt):
    """changing an element of segment k changes F only inside segment k -- and, with the previous element as predictor, only at that
    element and the next"""
    seg, m = 256, 4 * 256 + 17
    d = FL.gen("walk", esize, m, esize - 1, 5)
    f = FL.forward(d, esize, filt, seg).copy()
    for i in (0, 255, 256, 300, 767, 1024, m - 1):
        e = d.copy()
        e[i * esize] ^= 0x41
        g = FL.forward(e, esize, filt, seg)
        changed = np.flatnonzero((g != f)[:m * esize]) // esize
        k = i // seg
        assert changed.size and (changed >= k * seg).all() and (changed < (k + 1) * seg).all(), (i, changed)
        assert set(changed) <= {i, i + 1}
        assert np.array_equal(g[m * esize:], f[m * esize:])
    # and a segment decodes from its own values alone
    x = FL.inverse(f[2 * seg * esize:3 * seg * esize], esize, filt, seg)
    assert np.array_equal(x, d[2 * seg * esize:3 * seg * esize])


# ---- trc_fplanes_check on hand-made containers ------------------------------------------------------------------------------
def section(codec, m, chunk, clens, cdfnum=0):
    lens = [min(chunk, m - i * chunk) for i in range(len(clens))]
    pay = sum(min(l, ln) for l, ln in zip(clens, lens))
    hdr = struct.pack("<IBBHIIQQ", 0x31435254, codec, 1, cdfnum, chunk, len(clens), m, pay)
    return hdr + struct.pack("<%dI" % len(clens), *clens) + bytes(range(256)) * (pay // 256) + bytes(range(pay % 256))


def make(esize=2, t=0, codec=trc.RCA, m=600, chunk=256, clens=(256, 40, 9), magic=trc.PLANES_MAGIC, version=1, cdfnum=0):
    """a TRCP container of a non-static coder: header, offsets, esize sections (each 8-aligned), t tail bytes; cdfnum: the two
    parameters of an ss coder"""
    n = m * esize + t
    secs = [section(codec, m, chunk, clens, cdfnum)] * esize
    pos, off, body = 32 + 8 * esize, [], b""
    for s in secs:
        off.append(pos)
        s = s + b"\0" * (-len(s) % 8)
        body += s
        pos += len(s)
    hdr = struct.pack("<IBBBBIIQQ", magic, codec, version, esize, t, chunk, cdfnum, n, pos + t)
    return hdr + struct.pack("<%dQ" % esize, *off) + body + bytes([0xEE] * t), n


def wrap(inner, magic=trc.FPLANES_MAGIC, filt=FL.ZDELTA, version=1, zero=0, size=None):
    b = struct.pack("<IBBHQ", magic, filt, version, zero, 16 + len(inner) if size is None else size) + inner
    return np.frombuffer(b, dtype=np.uint8).copy()


def check(buf, buflen=None, outlen=ANY):
    return trc.lib().trc_fplanes_check(buf.ctypes.data, buf.size if buflen is None else buflen, outlen)


def err():
    return trc.lib().trc_last_error().decode()


@pytest.mark.parametrize("esize,t", [(2, 1), (4, 0), (8, 7)])
@pytest.mark.parametrize("filt", FL.FILTERS)
def test_check_accepts(esize, t, filt):
    inner, n = make(esize, t)
    buf = wrap(inner, filt=filt)
    assert check(buf) == 0 and check(buf, outlen=n) == 0
    trc.fplanes_check(buf, n)
    assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
    assert trc.lib().trc_planes_check(buf[16:].ctypes.data, buf.size - 16, n) == 0        # the inner part is a TRCP container as it stands


def test_check_rejects_each_defect():
    inner, n = make(4, 1)
    good = wrap(inner)
    assert check(good) == 0
    assert check(wrap(inner, magic=trc.PLANES_MAGIC)) != 0 and "magic" in err()          # TRCP
    assert check(wrap(inner, magic=0x31435254)) != 0 and "magic" in err()                # TRC1
    assert check(np.frombuffer(inner, dtype=np.uint8).copy()) != 0 and "magic" in err()  # a bare TRCP container
    assert check(wrap(inner, version=2)) != 0 and "version" in err()
    assert check(wrap(inner, filt=0)) != 0 and "filter 0" in err()
    assert check(wrap(inner, filt=3)) != 0 and "filter 3" in err()
    assert check(wrap(inner, zero=1)) != 0 and "reserved" in err()
    assert check(wrap(inner, size=16 + len(inner) + 8)) != 0 and "buffer holds" in err()      # size > buflen
    assert check(good, buflen=good.size - 1) != 0 and "buffer holds" in err()
    assert check(wrap(inner, size=15)) != 0 and "size 15" in err()                       # size < 16
    assert check(wrap(inner, size=16)) != 0 and "size 16" in err()                       # no room for an inner container
    assert check(good, buflen=15) != 0 and "shorter than the header" in err()
    assert check(wrap(inner[:-9])) != 0 and "planes container" in err()                  # a truncated inner container
    assert check(wrap(inner, size=16 + len(inner) - 9)) != 0 and "planes container" in err()
    assert check(wrap(make(4, 1, version=2)[0])) != 0 and "planes container" in err()    # the TRCP version 2 stays rejected
    assert check(good, outlen=n - 1) != 0 and "caller expects" in err()                  # another length than the caller expects
    with pytest.raises(trc.TrcError, match="filter 3"):
        trc.fplanes_check(wrap(inner, filt=3))


def prm_of(codec):
    return trc.ss_prm((4, 7)) if codec in trc.SSBIT else 0


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_check_rejects_a_low_nibble_coder(codec):
    """the TRCP container of a coder of in[i] & 15 behind a sound 16-byte prefix: refused by the check and by every decoder that
    reads a TRCF container, before a device is looked for"""
    L = trc.lib()
    for esize, t in ((2, 1), (4, 0), (8, 7)):
        inner, n = make(esize, t, codec=codec, cdfnum=prm_of(codec))
        for filt in FL.FILTERS:
            buf = wrap(inner, filt=filt)
            assert check(buf) != 0 and LOW4_TEXT in err() and "codec %d" % codec in err()
            with pytest.raises(trc.TrcError, match=LOW4_TEXT):
                trc.fplanes_check(buf, n)
            out = np.full(n + 64, 0xA5, dtype=np.uint8)
            for name in ("trc_decode_fplanes_host", "trc_decode_xplanes_host"):
                assert getattr(L, name)(buf.ctypes.data, buf.size, out.ctypes.data, n) == 0 and LOW4_TEXT in err(), name
            assert L.trc_decode_fplanes_range_host(buf.ctypes.data, buf.size, 0, 8, out.ctypes.data) == 0 and LOW4_TEXT in err()
            assert (out == 0xA5).all()
    for codec_ok in (trc.RCU3, trc.RCU3SS):                        # the varint neighbours of the same table macros code whole bytes
        inner, n = make(4, 3, codec=codec_ok, cdfnum=prm_of(codec_ok))
        assert check(wrap(inner)) == 0, err()


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_host_encode_refuses_a_low_nibble_coder_before_any_device(codec):
    L = trc.lib()
    d = FL.gen("monotone", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for filt in FL.FILTERS:
        assert L.trc_encode_fplanes_host(codec, filt, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, prm_of(codec)) == 0
        assert LOW4_TEXT in err() and "codec %d" % codec in err()
        with pytest.raises(trc.TrcError, match=LOW4_TEXT):
            trc.host_encode_fplanes(codec, filt, d, 4, 0, prm=(4, 7))
    assert (out == 0xA5).all()


def test_bound():
    L = trc.lib()
    for esize in FL.ESIZES:
        for n in (esize, 1000 * esize + esize - 1, 10**6 + 1):
            for chunk in (0, 256, 4096):
                for cdfnum in (0, 256):
                    assert L.trc_fplanes_bound(n, esize, chunk, cdfnum) == L.trc_planes_bound(n, esize, chunk, cdfnum) + 16 > 16
        assert L.trc_fplanes_bound(esize - 1, esize, 256, 0) == 0
        assert L.trc_fplanes_bound(4096, esize, 100, 0) == 0
    assert L.trc_fplanes_bound(4096, 3, 256, 0) == 0
    assert trc.fplanes_bound(4096, 4, 256) == trc.planes_bound(4096, 4, 256) + 16


# ---- without a device ---------------------------------------------------------------------------------------------------------
def _no_gpu():
    try:
        return trc.lib().trc_device_count() == 0
    except Exception:
        return False


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible: the calls would succeed")
def test_host_calls_without_a_device_return_zero_and_say_why():
    L = trc.lib()
    d = FL.gen("monotone", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for filt in FL.FILTERS:
        assert L.trc_encode_fplanes_host(trc.RCA, filt, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert "no HIP device" in err()
        assert (out == 0xA5).all(), "encode wrote to its output"
        with pytest.raises(trc.TrcError, match="no HIP device"):
            trc.host_encode_fplanes(trc.RCA, filt, d, 4, 256)
    inner, n = make(4, 1)
    buf = wrap(inner)
    assert L.trc_decode_fplanes_host(buf.ctypes.data, buf.size, out.ctypes.data, n) == 0 and "no HIP device" in err()
    assert L.trc_decode_fplanes_range_host(buf.ctypes.data, buf.size, 5, 100, out.ctypes.data) == 0 and "no HIP device" in err()
    assert (out == 0xA5).all(), "a decoder wrote to its output"
    with pytest.raises(trc.TrcError, match="no HIP device"):
        trc.host_decode_fplanes(buf, n)


def test_host_argument_errors_need_no_device():
    """what is wrong with the arguments or the container is said before a device is looked for"""
    L = trc.lib()
    d = FL.gen("monotone", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for filt in (FL.NONE, 3, -1):
        assert L.trc_encode_fplanes_host(trc.RCA, filt, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert "filter %d" % filt in err()
    inner, n = make(4, 1)
    bad = wrap(inner, filt=3)
    assert L.trc_decode_fplanes_host(bad.ctypes.data, bad.size, out.ctypes.data, n) == 0 and "filter 3" in err()
    assert L.trc_decode_fplanes_range_host(bad.ctypes.data, bad.size, 0, 10, out.ctypes.data) == 0 and "filter 3" in err()
    good = wrap(inner)
    assert L.trc_decode_fplanes_host(good.ctypes.data, good.size, out.ctypes.data, n - 1) == 0 and "caller expects" in err()
    assert (out == 0xA5).all()


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
    assert "trc_encode_fplanes_host" in src and "trc_decode_fplanes_host" in src and "trc_decode_fplanes_range_host" in src
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2 and "trcfile f <id> <esize> <z|x> <in> <out>" in u.stderr
