"""The TRCB container of a coded batch (include/trc_hip.h): the numpy definition of its front and of its layout, on top of the
batch definitions of planes_batch_lib and fplanes_batch_lib, which serve unchanged.

    trc_planes_batch_hdr (48 B) | uint64 n[count] | uint8 filter[count], zero-padded to a multiple of 8 | inner
    inner = the TRCP container of VF(items, filters, esize, chunk):  n = M * esize, tail = 0

Bytes [inner, size) are what trc_encode_planes_host writes for the materialised VF at the same chunk, so the expected container of
a GPU test is front(...) followed by trc.host_encode_planes(codec, VF, esize, chunk, ...), the parent's call."""
import struct

import numpy as np

import fplanes_batch_lib as FB
import planes_batch_lib as BL

MAGIC = 0x42435254                                             # "TRCB"
HDR = 48
PAD = 256
STATIC = (1, 2, 3, 11)                                         # the coders that store a CDF per section


def up8(x):
    return (x + 7) & ~7


def inner_offset(count):
    return HDR + 8 * count + up8(count)


def front(sizes, filters, esize, chunk, size, magic=MAGIC, version=1, zero=0, zero2=0, inner=None, count=None, nbytes=None, pad=0):
    """the container's first `inner` bytes (np.uint8); filters None: a batch without filters stores zeros.  The keyword arguments
    are the defects of the checker's tests; pad: the value of the filter padding"""
    cnt = len(sizes)
    f = [0] * cnt if filters is None else [int(x) for x in filters]
    assert len(f) == cnt
    hdr = struct.pack("<IBBHIIQQQQ", magic, version, esize, zero, chunk, zero2, cnt if count is None else count,
                      inner_offset(cnt) if inner is None else inner, size, sum(sizes) if nbytes is None else nbytes)
    assert len(hdr) == HDR
    out = hdr + struct.pack("<%dQ" % cnt, *sizes) + bytes(f) + bytes([pad] * (up8(cnt) - cnt))
    return np.frombuffer(out, dtype=np.uint8).copy()


def layout(sizes, esize, chunk, codec, cdfnum, totals):
    """(inner, off[esize] from the TRCB start, size) by the rules of the TRCP container: sections at multiples of 8, a static
    coder's CDF in up8(2 (cdfnum + 1)) bytes, the 32-byte TRC1 header, the directory, the payload"""
    p, _ = BL.plan(sizes, esize, chunk)
    cdfb = up8(2 * (cdfnum + 1)) if codec in STATIC else 0
    inner = inner_offset(len(sizes))
    pos, off = 32 + 8 * esize, []
    for k in range(esize):
        assert totals[k] <= p["m_total"]
        off.append(inner + pos)
        pos = up8(pos + cdfb + 32 + 4 * p["chunks"] + totals[k])
    return inner, off, inner + pos


def bound(sizes, esize, chunk, planes_bound):
    """48 + table + trc_planes_bound(M * esize, ...) + TRC_PAD; planes_bound: that figure for n = plan(..)["n_virtual"]"""
    return inner_offset(len(sizes)) + planes_bound + PAD


def virtual_filtered(items, filters, esize, chunk):
    """VF of the batch; filters None: V"""
    return BL.virtual(items, esize, chunk) if filters is None else FB.virtual_filtered(items, filters, esize, chunk)


def expected(items, filters, esize, chunk, inner_container):
    """the whole container, given the TRCP container of VF"""
    sizes = [int(np.asarray(d).size) for d in items]
    f = front(sizes, filters, esize, chunk, inner_offset(len(sizes)) + inner_container.size)
    return np.concatenate([f, np.ascontiguousarray(inner_container, dtype=np.uint8)])
