"""Inputs and reference calls for the Turbo-VLC coders on the bitwise range coder (rcvs*, rcvzs*, rcvgs*, rcvgzs* at 16 / 32
bits: codecs TRC_RCBV16 = 43 .. TRC_RCBVGZ32 = 50).

gen(kind, es, n, seed): n bytes of little-endian es-byte elements (the last element cut where n is not a multiple of es):
  geo      geometric values, mean ~50 (most above 32: exponent and mantissa)
  walk     a random walk, steps -40..40 (16-bit) or -3000..3000 (32-bit), wrapping at the element width: small zigzag deltas
  mixed    geometric values (mean ~10) with 1 % uniform ones over the whole width
  allmax   every element 0xffff / 0xffffffff
  uniform  uniform bytes (every chunk raw)
  max<v>   v (masked to the width) at every 16th element, 0 elsewhere: the chunk maxima that pin rcvsenc32's vb (VB32)
"""
import numpy as np

import trc_testlib as T

RCBV16, RCBV32, RCBVZ16, RCBVZ32, RCBVG16, RCBVG32, RCBVGZ16, RCBVGZ32 = 43, 44, 45, 46, 47, 48, 49, 50
CODECS = list(range(43, 51))
ES = {c: 2 if c % 2 else 4 for c in CODECS}
FAMILY = {43: "rcvs", 45: "rcvzs", 47: "rcvgs", 49: "rcvgzs"}
NAMES = {c: FAMILY[c - (c - 43) % 2] + str(8 * ES[c]) for c in CODECS}
REF_FN = {c: (FAMILY[c - (c - 43) % 2] + "enc" + str(8 * ES[c]), FAMILY[c - (c - 43) % 2] + "dec" + str(8 * ES[c])) for c in CODECS}
CTX = (RCBV16, RCBVZ16, RCBVZ32)                 # 256 trees per chunk in the workspace
CONSTS = {"max0": 0, "max7": 7, "max8": 8, "max15": 15, "max16": 16, "max1000": 1000, "max2p31": 1 << 31}
# vb byte of rcvsenc32 (payload offset 4) against the chunk's maximum, measured on the reference
VB32 = {0: 255, 7: 255, 8: 247, 15: 240, 16: 239, 1000: 192, 1 << 31: 23}
KINDS = ["geo", "walk", "mixed", "allmax", "uniform"] + list(CONSTS)


def gen(kind, es, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ne = (n + es - 1) // es
    dt = {2: "<u2", 4: "<u4"}[es]
    top = (1 << (8 * es)) - 1
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "geo":
        v = np.minimum(rng.geometric(0.02, ne) - 1, top)
    elif kind == "walk":
        step = 40 if es == 2 else 3000
        v = (np.cumsum(rng.integers(-step, step + 1, ne)) + (top >> 1)) & top
    elif kind == "mixed":
        v = np.minimum(rng.geometric(0.1, ne) - 1, top)
        big = rng.random(ne) < 0.01
        v = np.where(big, rng.integers(0, top, ne, dtype=np.int64, endpoint=True), v)
    elif kind == "allmax":
        v = np.full(ne, top, dtype=np.int64)
    elif kind in CONSTS:
        v = np.where(np.arange(ne) % 16 == 0, CONSTS[kind] & top, 0).astype(np.int64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v.astype(np.uint64).astype(dt)).view(np.uint8)[:n].copy()


# (on short inputs the reference's reversed bit writer stores 8 bytes at out + n - 8: the arena's 2n+64 bytes in front of `out`)
_REF = T.RefCalls(REF_FN, T.REF_SO)
have_ref, ref_enc, ref_chunked_enc = _REF.have, _REF.enc, _REF.chunked_enc
