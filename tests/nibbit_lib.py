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
import numpy as np

import trc_testlib as T

RC4, RC4C, RCU3 = 58, 59, 60
CODECS = [RC4, RC4C, RCU3]
NAMES = {RC4: "rc4s", RC4C: "rc4cs", RCU3: "rcu3s"}
REF_FN = {RC4: ("rc4senc", "rc4sdec"), RC4C: ("rc4csenc", "rc4csdec"), RCU3: ("rcu3senc", "rcu3sdec")}
NIBBLE = (RC4, RC4C)                                           # code d & 15
KINDS = ["nib_uniform", "nib_skew", "zeros", "bytes_uniform", "bytes_small", "mixed"]


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


_REF = T.RefCalls(REF_FN, T.REF_SO)
have_ref, ref_enc, ref_chunked_enc, ref_dec = _REF.have, _REF.enc, _REF.chunked_enc, _REF.dec
