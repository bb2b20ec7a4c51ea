"""Random-access decode, the parts that need no GPU: the new declarations and wrappers, trc_container_range on hand-built
containers (header + directory + filler payload), the workspace rule of trc_range_work_bytes, and what
trc_decode_range_host answers on a box without a device."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRC_E_ARG = -1
N, CHUNK = 5 * 256 + 7, 256
CLEN = np.array([256, 10, 256, 33, 1, 7], dtype=np.uint32)          # raw, coded, raw, coded, coded, raw (the 7-byte tail)
# one id per decode launcher of csrc/trc_launch.h (the rcs launcher with each of its three geometries)
LAUNCHER_IDS = (trc.ANS4S, trc.RCS1, trc.RCS2, trc.RCSM, trc.RCB, trc.RCA, trc.RCAI, trc.RCA4, trc.RCV8, trc.ANSA, trc.ANSO1, trc.ANSB,
                trc.VLCU16, trc.VLAU16, trc.RCC1, trc.RCG16, trc.RCR32, trc.RCBVZ16, trc.RCW16, trc.RC4, trc.RCU3)
UNASSIGNED = (42, 51, 56, 57, 61)


def container(codec=trc.RCA, n=N, chunk=CHUNK, clen=CLEN, payload=None):
    lens = np.minimum(chunk, n - np.arange(0, n, chunk))
    pay = int(np.minimum(clen, lens).sum()) if payload is None else payload
    hdr = struct.pack("<IBBHIIQQ", 0x31435254, codec, 1, 0, chunk, len(clen), n, pay)
    body = np.arange(int(np.minimum(clen, lens).sum()), dtype=np.uint32).astype(np.uint8)      # filler
    return np.frombuffer(hdr + np.asarray(clen, "<u4").tobytes() + body.tobytes(), dtype=np.uint8).copy()


def plan_rc(buf, buflen, codec, offset, length):
    r = trc.Range()
    rc = trc.lib().trc_container_range(buf.ctypes.data, buflen, codec, offset, length, C.byref(r))
    return rc, r


def test_declarations_and_wrappers():
    txt = open(os.path.join(ROOT, "include", "trc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = trc.lib()
    for name in ("trc_range_work_bytes", "trc_decode_range_dev", "trc_container_range", "trc_decode_range_host"):
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in include/trc_hip.h"
        assert hasattr(lib, name), name + " is not exported"
    assert "typedef struct trc_range" in txt
    for name in ("range_work_bytes", "container_range", "host_decode_range"):
        assert callable(getattr(trc, name))
    assert callable(trc.DeviceCoder.decode_range)


@pytest.mark.parametrize("offset,length", [(0, 1), (255, 2), (256, 256), (300, 1000), (300, N - 300), (N - 1, 1), (0, N)])
def test_container_range_fields(offset, length):
    buf = container()
    if offset + length > N:                                        # (300, 1000) ends 13 bytes behind n = 1287: refused, not clipped;
        assert plan_rc(buf, buf.size, trc.RCA, offset, length)[0] == TRC_E_ARG      # (300, n - 300) covers the same chunks 1 .. 5
        return
    lens = np.minimum(CHUNK, N - np.arange(0, N, CHUNK))
    cum = np.concatenate([[0], np.cumsum(np.minimum(CLEN, lens))])
    first, last = offset // CHUNK, (offset + length - 1) // CHUNK
    want = dict(first_chunk=first, nchunks=last - first + 1, payload_off=int(cum[first]), payload_len=int(cum[last + 1] - cum[first]),
                out_skip=offset - first * CHUNK, out_bytes=min(N, (last + 1) * CHUNK) - first * CHUNK)
    assert trc.container_range(buf, offset, length) == want
    rc, r = plan_rc(buf, buf.size, trc.RCA, offset, length)        # ... and with the codec named
    assert rc == 0 and {f: int(getattr(r, f)) for f in want} == want


def test_container_range_errors():
    lib = trc.lib()
    buf = container()
    assert plan_rc(buf, buf.size, trc.RCA, 0, N)[0] == 0
    for what, args in (("offset + len > n", (buf, buf.size, trc.RCA, 1, N)),
                       ("offset > n", (buf, buf.size, trc.RCA, N + 1, 1)),
                       ("len == 0", (buf, buf.size, trc.RCA, 10, 0)),
                       ("wrong codec", (buf, buf.size, trc.RCB, 0, 1)),
                       ("truncated buffer", (buf, buf.size - 1, trc.RCA, 0, 1)),
                       ("no room for the directory", (buf, 40, trc.RCA, 0, 1))):
        assert plan_rc(*args)[0] == TRC_E_ARG, what
        assert lib.trc_last_error(), what
    bad = container(payload=int(np.minimum(CLEN, 256).sum()) + 1)  # the directory's sum disagrees with the header
    bad = np.concatenate([bad, np.zeros(8, np.uint8)])
    assert plan_rc(bad, bad.size, trc.RCA, 0, 1)[0] == TRC_E_ARG
    with pytest.raises(trc.TrcError):
        trc.container_range(buf, N, 1)


def test_an_entry_above_the_chunk_length_counts_as_raw():
    """the directory entries are clamped as the decoders clamp them: an entry above the chunk's length is that length"""
    clen = CLEN.copy(); clen[2] = 70000
    a, b = container(clen=clen), container()
    assert trc.container_range(a, 600, 500) == trc.container_range(b, 600, 500)


@pytest.mark.parametrize("codec", LAUNCHER_IDS, ids=lambda c: trc.CODEC_NAMES[c])
def test_range_work_bytes_bound(codec):
    """0 < range workspace <= workspace of a `count`-chunk decode + 16 bytes per group of the whole directory + 4096"""
    lib = trc.lib()
    for chunk in (256, 4096, 8192, 16384, 65536):
        if codec == trc.ANSB and chunk > 8192:
            assert trc.range_work_bytes(codec, 10**6, chunk, 1) == 0   # a chunk trc_encode_dev rejects
            continue
        for n in (1, 100000, 10**6 + 7, 1 << 30):
            nch = -(-n // chunk)
            ngroups = -(-nch // 64)
            for count in sorted({1, min(63, nch), min(64, nch), min(65, nch), min(4096, nch), nch}):
                rb = trc.range_work_bytes(codec, n, chunk, count)
                assert 0 < rb <= lib.trc_work_bytes(codec, count * chunk, chunk) + 16 * ngroups + 4096, (chunk, n, count, rb)
            assert trc.range_work_bytes(codec, n, chunk, 0) == 0
            assert trc.range_work_bytes(codec, n, chunk, nch + 1) == 0
    for chunk in (0, 100, 192, 65600):
        assert trc.range_work_bytes(codec, 10**6, chunk, 1) == 0, chunk
    sizes = [trc.range_work_bytes(codec, 1 << 30, 4096, count) for count in (1, 63, 64, 65, 4096)]
    assert sizes == sorted(sizes) and sizes[0] > 0, sizes
    # it grows with the range and the directory, not with n: a gigabyte container, one chunk
    assert sizes[0] < (16 << 20), sizes


def test_range_work_bytes_of_unassigned_ids():
    for codec in UNASSIGNED + (0, -1):
        assert trc.range_work_bytes(codec, 1 << 30, 4096, 64) == 0, codec


def _no_gpu():
    try:
        return trc.lib().trc_device_count() == 0
    except Exception:
        return False


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible: the call would succeed")
def test_decode_range_host_without_a_device():
    """as for every host-pointer call (tests/test_no_device_contract.py): 0, a reason, nothing written"""
    lib = trc.lib()
    buf = container()
    out = np.full(N + 64, 0xA5, dtype=np.uint8)
    assert lib.trc_decode_range_host(trc.RCA, buf.ctypes.data, buf.size, N, 300, 500, out.ctypes.data, None, 0) == 0
    assert b"no HIP device" in lib.trc_last_error()
    assert (out == 0xA5).all()
    with pytest.raises(trc.TrcError):
        trc.host_decode_range(trc.RCA, buf, N, 300, 500)
    # stored raw (inlen == n) needs no device: it is a copy of the range
    raw = np.arange(N, dtype=np.uint32).astype(np.uint8)
    assert np.array_equal(trc.host_decode_range(trc.RCA, raw, N, 300, 500), raw[300:800])
