"""Inputs and reference calls for the bitwise order-1 range coders (rccs / rcxs: codecs TRC_RCC1 / TRC_RCX1).

markov_bytes: a seeded order-1 source that order 0 cannot compress.  Every previous byte s selects its own Zipf(1.3)
distribution over a permuted alphabet: x_i = (MK_MUL * x_{i-1} + MK_PERM[r_i]) mod 256 with i.i.d. Zipf ranks r_i, so state s
puts rank r on symbol MK_MUL * s + MK_PERM[r].  The recurrence is affine in x, which makes it vectorisable
(x_i = A^i * (x_0 + sum_{j <= i} A^-j t_j)); harness/trcbench.c --markov generates the same bytes in C.
"""
import numpy as np

import trc_testlib as T

RCC1, RCX1 = 28, 29
NAMES = {RCC1: "rccs", RCX1: "rcxs"}
REF_FN = {RCC1: ("rccsenc", "rccsdec"), RCX1: ("rcxsenc", "rcxsdec")}
ROUND_CHUNK = 16384                                            # TRC_O1BIT_CHUNK_MIN (include/trc_hip.h)
MK_MUL = 77                                                    # odd: a bijection of the state for every rank
MK_PERM = (np.arange(256, dtype=np.int64) * 173 + 29) & 255   # rank -> symbol offset (a permutation)


def markov_bytes(n, seed=21, alpha=1.3):
    r = T.zipf_bytes(n, alpha, 256, seed).astype(np.int64)
    t = MK_PERM[r]
    i = np.arange(1, n + 1, dtype=np.int64)
    # A has order 64 mod 256: A^i and A^-i repeat with period 64
    a_pow = np.ones(64, dtype=np.int64)
    for k in range(1, 64):
        a_pow[k] = (a_pow[k - 1] * MK_MUL) & 255
    a_inv = np.array([a_pow[(64 - k) % 64] for k in range(64)], dtype=np.int64)
    s = np.cumsum((a_inv[i % 64] * t) & 255) & 255             # x_0 = 0
    return ((a_pow[i % 64] * s) & 255).astype(np.uint8)


def gen(kind, n, seed):
    if kind == "text":
        return T.text_bytes(n, seed)
    if kind == "markov":
        return markov_bytes(n, seed)
    if kind == "runs":
        return T.runs_bytes(n, seed)
    if kind == "uniform":
        return T.uniform_bytes(n, seed)
    if kind == "const":
        return np.full(n, 65, dtype=np.uint8)
    if kind == "binary":
        return ((T.uniform_bytes(n, seed) & 1) * 7).astype(np.uint8)
    raise ValueError(kind)


_REF = T.RefCalls(REF_FN, T.REF_SO)
have_ref, ref_enc, ref_chunked_enc, ref_dec = _REF.have, _REF.enc, _REF.chunked_enc, _REF.dec
