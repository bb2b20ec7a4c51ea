"""Inputs and reference calls for the bitwise word coders (rcsenc16 / rcsenc32 / rccsenc32 / rcc2senc32: codecs
TRC_RCW16 = 52 .. TRC_RCC2W32 = 55).

gen(kind, es, n, seed): n bytes of little-endian es-byte words (the last word cut where n is not a multiple of es):
  walk     a random walk, steps -40..40 (16-bit) or -3000..3000 (32-bit), wrapping at the word width
  sine     a sine of ~1/4 the width's amplitude, period ~1000 words, plus noise of +-8 (16-bit) or +-500 (32-bit)
  stamps   increasing timestamps: steps of 900..1100 from a random start (32-bit: ~1.7e9, 16-bit: wrapping)
  geo      geometric small values, mean ~20
  allmax   every word 0xffff / 0xffffffff
  const    one random value repeated
  uniform  uniform bytes (the 32-bit coders store every chunk raw; rcs16 codes it to more than its length: raw)
"""
import os
import re

import numpy as np

import trc_testlib as T

RCW16, RCW32, RCCW32, RCC2W32 = 52, 53, 54, 55
CODECS = [RCW16, RCW32, RCCW32, RCC2W32]
ES = {RCW16: 2, RCW32: 4, RCCW32: 4, RCC2W32: 4}
NAMES = {RCW16: "rcs16", RCW32: "rcs32", RCCW32: "rccs32", RCC2W32: "rcc2s32"}
REF_FN = {RCW16: ("rcsenc16", "rcsdec16"), RCW32: ("rcsenc32", "rcsdec32"), RCCW32: ("rccsenc32", "rccsdec32"),
          RCC2W32: ("rcc2senc32", "rcc2sdec32")}
TREES = {RCW16: 257, RCW32: 2305, RCCW32: 2432, RCC2W32: 4352}
MODEL_BYTES = {c: t * 544 for c, t in TREES.items()}          # 17 blocks of 32 B per tree
KINDS = ["walk", "sine", "stamps", "geo", "allmax", "const", "uniform"]
GUARD = 64


def budget():
    """TRC_WORD_MODEL_BUDGET from include/trc_hip.h"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trc_hip.h")).read()
    return int(re.search(r"#define TRC_WORD_MODEL_BUDGET (\d+)ull", hdr).group(1))


def slots(codec, nchunks):
    """models one call holds: min(chunks, budget / model bytes in whole waves of 64)"""
    return min(nchunks, budget() // MODEL_BYTES[codec] // 64 * 64)


def gen(kind, es, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ne = (n + es - 1) // es
    dt = {2: "<u2", 4: "<u4"}[es]
    top = (1 << (8 * es)) - 1
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "walk":
        step = 40 if es == 2 else 3000
        v = (np.cumsum(rng.integers(-step, step + 1, ne)) + (top >> 1)) & top
    elif kind == "sine":
        noise = 8 if es == 2 else 500
        t = np.arange(ne, dtype=np.float64)
        v = ((top >> 1) + np.round((top >> 2) * np.sin(2 * np.pi * t / 1000.0 + rng.random())).astype(np.int64)
             + rng.integers(-noise, noise + 1, ne)) & top
    elif kind == "stamps":
        start = int(rng.integers(1_600_000_000, 1_800_000_000)) if es == 4 else int(rng.integers(0, 1 << 16))
        v = (start + np.cumsum(rng.integers(900, 1101, ne))) & top
    elif kind == "geo":
        v = np.minimum(rng.geometric(0.05, ne) - 1, top)
    elif kind == "allmax":
        v = np.full(ne, top, dtype=np.int64)
    elif kind == "const":
        v = np.full(ne, int(rng.integers(0, top, endpoint=True)), dtype=np.int64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.asarray(v).astype(np.uint64).astype(dt)).view(np.uint8)[:n].copy()


# `out` sits in a 0xA5-filled arena, and the GUARD bytes in front of it and behind what the encoder returns must be intact;
# ref_chunked_enc gives the chunks as the reference returns them (rcs16 and sub-word chunks may return more bytes than the
# chunk: see expected())
_REF = T.RefCalls(REF_FN, T.REF_SO, guard=GUARD)
have_ref, ref_enc, ref_chunked_enc = _REF.have, _REF.enc, _REF.chunked_enc


def expected(codec, data, chunk, clen, payload):
    """what the library stores for the reference's per-chunk output: a chunk the reference codes to >= its length (a chunk
    shorter than one word; rcsenc16 without an OVERFLOW test) is stored raw -> (clen, payload, number of chunks the reference
    returned more than their length for)"""
    starts = np.concatenate([[0], np.cumsum(clen.astype(np.int64))])
    outc, outp, raised = [], [], 0
    for k, i in enumerate(range(0, data.size, chunk)):
        ln = min(chunk, data.size - i)
        if int(clen[k]) >= ln:                                 # (== ln: the reference's raw chunk, the input itself)
            outc.append(ln)
            outp.append(data[i:i + ln])
            raised += int(clen[k]) > ln
        else:
            outc.append(int(clen[k]))
            outp.append(payload[starts[k]:starts[k + 1]])
    return (np.array(outc, dtype=np.uint32), np.concatenate(outp) if outp else np.zeros(0, np.uint8), raised)
