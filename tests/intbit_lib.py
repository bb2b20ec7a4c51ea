"""Inputs and reference calls for the gamma / Rice integer coders on the bitwise range coder (rcgs*, rcgzs*, rcrs*, rcrzs*:
codecs TRC_RCG8 = 30 .. TRC_RCRZ32 = 41).

gen(kind, es, n, seed): n bytes of little-endian es-byte elements (the last element cut where n is not a multiple of es):
  geo      geometric small values (p = 0.3)
  walk     a slow random walk (steps -3..3, wrapping at the element width): small zigzag deltas
  mixed    geometric values with 1 % uniform ones over the whole width (gamma / Rice escapes, GQMAX32)
  allmax   every element 0xff / 0xffff / 0xffffffff
  const    every element 5
  uniform  uniform bytes (every chunk raw)
"""
import ctypes as C
import os

import numpy as np

import trc_testlib as T

RCG8, RCG16, RCG32, RCGZ8, RCGZ16, RCGZ32 = 30, 31, 32, 33, 34, 35
RCR8, RCR16, RCR32, RCRZ8, RCRZ16, RCRZ32 = 36, 37, 38, 39, 40, 41
CODECS = list(range(30, 42))
ES = {c: 1 << ((c - 30) % 3) for c in CODECS}
FAMILY = {30: "rcgs", 33: "rcgzs", 36: "rcrs", 39: "rcrzs"}
NAMES = {c: FAMILY[30 + 3 * ((c - 30) // 3)] + str(8 * ES[c]) for c in CODECS}
REF_FN = {c: (FAMILY[30 + 3 * ((c - 30) // 3)] + "enc" + str(8 * ES[c]), FAMILY[30 + 3 * ((c - 30) // 3)] + "dec" + str(8 * ES[c]))
          for c in CODECS}
KINDS = ["geo", "walk", "mixed", "allmax", "const", "uniform"]
_INV = {}


def gen(kind, es, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ne = (n + es - 1) // es
    dt = {1: "<u1", 2: "<u2", 4: "<u4"}[es]
    top = (1 << (8 * es)) - 1
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "geo":
        v = np.minimum(rng.geometric(0.3, ne) - 1, top)
    elif kind == "walk":
        v = (np.cumsum(rng.integers(-3, 4, ne)) + (top >> 1)) & top
    elif kind == "mixed":
        v = np.minimum(rng.geometric(0.3, ne) - 1, top)
        big = rng.random(ne) < 0.01
        v = np.where(big, rng.integers(0, top, ne, dtype=np.int64, endpoint=True), v)
    elif kind == "allmax":
        v = np.full(ne, top, dtype=np.int64)
    elif kind == "const":
        v = np.full(ne, 5, dtype=np.int64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v.astype(np.uint64).astype(dt)).view(np.uint8)[:n].copy()


def have_ref():
    return os.path.exists(T.REF_SO)


def _ref_lib():
    lib = C.CDLL(T.REF_SO)
    for codec in REF_FN:
        for name in REF_FN[codec]:
            f = getattr(lib, name)
            f.restype = C.c_size_t
            f.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8)]
    return lib


def ref_enc(codec, data):
    """one call of the reference encoder on `data`, `in` below `out` in one arena (trc_testlib._arena)"""
    lib = _INV.get("lib") or _INV.setdefault("lib", _ref_lib())
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    buf, io, oo = T._arena(n)
    buf[io:io + n] = data
    base = buf.ctypes.data
    l = getattr(lib, REF_FN[codec][0])(C.cast(base + io, C.POINTER(C.c_uint8)), n, C.cast(base + oo, C.POINTER(C.c_uint8)))
    return buf[oo:oo + l].copy()


def chunk_payload(codec, piece):
    """the library's payload of one chunk: the reference's bytes, except that a chunk shorter than one element is stored raw
    (the reference returns its tail bytes plus an empty 4-byte flush there, include/trc_hip.h)"""
    if piece.size < ES[codec]:
        return piece.copy()
    return ref_enc(codec, piece)


def ref_chunked_enc(codec, data, chunk):
    """-> (clen u32 array, payload u8 array): the reference called once per chunk"""
    outs = [chunk_payload(codec, data[i:i + chunk]) for i in range(0, data.size, chunk)]
    clen = np.array([o.size for o in outs], dtype=np.uint32)
    payload = np.concatenate(outs) if outs else np.zeros(0, np.uint8)
    return clen, payload


def ref_dec(codec, comp, n):
    lib = _INV.get("lib") or _INV.setdefault("lib", _ref_lib())
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    if comp.size == n:
        return comp.copy()
    src = np.zeros(comp.size + 1024, dtype=np.uint8); src[:comp.size] = comp
    out = np.zeros(n + 64, dtype=np.uint8)
    getattr(lib, REF_FN[codec][1])(src.ctypes.data_as(C.POINTER(C.c_uint8)), n, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out[:n].copy()
