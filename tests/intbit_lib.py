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


def chunk_payload(codec, piece):
    """the library's payload of one chunk: the reference's bytes, except that a chunk shorter than one element is stored raw
    (the reference returns its tail bytes plus an empty 4-byte flush there, include/trc_hip.h)"""
    if piece.size < ES[codec]:
        return piece.copy()
    return ref_enc(codec, piece)


_REF = T.RefCalls(REF_FN, T.REF_SO, chunk_hook=chunk_payload)
have_ref, ref_enc, ref_chunked_enc, ref_dec = _REF.have, _REF.enc, _REF.chunked_enc, _REF.dec
