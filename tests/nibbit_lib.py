"""Inputs and reference calls for the bitwise nibble and varint byte coders (rc4s, rc4cs, rcu3s: codecs TRC_RC4 = 58,
TRC_RC4C = 59, TRC_RCU3 = 60).

gen(kind, n, seed, chunk): n bytes
  nib_uniform    uniform values 0..15
  nib_skew       min(geometric(0.5) - 1, 15)
  zeros          every byte 0
  bytes_uniform  uniform bytes: the rc4 coders code their low nibbles (the decoders return d & 15), rcu3s goes raw in mid-chunk
  bytes_small    min(geometric(0.2) - 1, 255)
  mixed          chunks of bytes_uniform and bytes_small in turn (`chunk` bytes each): raw and coded chunks side by side
"""
import ctypes as C
import os

import numpy as np

import trc_testlib as T

RC4, RC4C, RCU3 = 58, 59, 60
CODECS = [RC4, RC4C, RCU3]
NAMES = {RC4: "rc4s", RC4C: "rc4cs", RCU3: "rcu3s"}
REF_FN = {RC4: ("rc4senc", "rc4sdec"), RC4C: ("rc4csenc", "rc4csdec"), RCU3: ("rcu3senc", "rcu3sdec")}
NIBBLE = (RC4, RC4C)                                           # code d & 15
KINDS = ["nib_uniform", "nib_skew", "zeros", "bytes_uniform", "bytes_small", "mixed"]
_INV = {}


def gen(kind, n, seed, chunk=1024):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "nib_uniform":
        return rng.integers(0, 16, n, dtype=np.uint8)
    if kind == "nib_skew":
        return np.minimum(rng.geometric(0.5, n) - 1, 15).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "bytes_uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "bytes_small":
        return np.minimum(rng.geometric(0.2, n) - 1, 255).astype(np.uint8)
    if kind == "mixed":
        u = rng.integers(0, 256, n, dtype=np.uint8)
        s = np.minimum(rng.geometric(0.2, n) - 1, 255).astype(np.uint8)
        return np.where((np.arange(n) // chunk) % 2 == 0, u, s).astype(np.uint8)
    raise ValueError(kind)


def expected(codec, d, clen, chunk):
    """what a decoder returns for input d coded into the directory clen: the rc4 coders keep the low nibble only, in the
    chunks they coded (a raw chunk holds the input bytes as they were)"""
    if codec not in NIBBLE:
        return d
    lens = np.minimum(chunk, d.size - np.arange(0, d.size, chunk))
    coded = np.repeat(np.asarray(clen) != lens, lens)
    return np.where(coded, d & 15, d).astype(np.uint8)


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


def ref_chunked_enc(codec, data, chunk):
    """-> (clen u32 array, payload u8 array): the reference called once per chunk"""
    outs = [ref_enc(codec, data[i:i + chunk]) for i in range(0, data.size, chunk)]
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
