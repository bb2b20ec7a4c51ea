"""Zigzag-delta and xor filters in front of the byte planes: the numpy model F (and its inverse) that the filtered planar calls are
checked against, the inputs of the tests, and the fixture tests/golden/fplanes_vectors.npz that pins the model.

Definition (include/trc_hip.h): the m = n // esize elements x[i] are little-endian unsigned words of w = 8 * esize bits, the
t = n % esize tail bytes are never filtered; p[i] = 0 where i % seg == 0, else x[i - 1];
    ZDELTA: d = x[i] - p[i] mod 2^w, y[i] = (d << 1) ^ (0 - (d >> (w - 1)))        XOR: y[i] = x[i] ^ p[i]
F(filter, seg, esize, in) = the y's followed by the tail.  No reference implementation exists to compare with (the reference's
scalar zigzag transpose is unfinished), so the definition above is the only source and this model the yardstick.
"""
import hashlib
import json
import os

import numpy as np

ESIZES = (2, 4, 8)
NONE, ZDELTA, XOR = 0, 1, 2
FILTERS = (ZDELTA, XOR)
FILTER_NAMES = {ZDELTA: "z", XOR: "x"}
KINDS = ("random", "monotone", "walk", "wrap")
DT = {2: "<u2", 4: "<u4", 8: "<u8"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fplanes_vectors.npz")
GOLDEN_STORE_MAX = 4096                                        # F(in) of cases up to this many bytes is stored, of larger ones hashed
# restart lengths at which the scanning joins (512 elements per tile) leave a partial tile inside a span: spans of 6 and 7 tiles from
# 8 segments below a tile; one tile + 8 lanes; one tile + 448 elements; 3 tiles + 448; 5 whole tiles, the control
RESTARTS = (384, 448, 576, 960, 1984, 2560)


def _parts(data, esize):
    d = np.ascontiguousarray(data, dtype=np.uint8)
    m = d.size // esize
    return d[:m * esize].view(DT[esize]), d[m * esize:]


def forward(data, esize, filt, seg):
    """F(filt, seg, esize, data) as uint8 array of the same length"""
    x, tail = _parts(data, esize)
    w = 8 * esize
    p = np.concatenate([np.zeros(1, x.dtype), x[:-1]])
    p[::seg] = 0
    if filt == XOR:
        y = x ^ p
    else:
        d = x - p                                              # unsigned: wraps mod 2^w
        ones = np.array((1 << w) - 1, dtype=x.dtype)
        y = (d << np.array(1, x.dtype)) ^ np.where(d >> np.array(w - 1, x.dtype), ones, np.zeros((), x.dtype))
    return np.concatenate([y.astype(DT[esize]).view(np.uint8), tail])


def inverse(data, esize, filt, seg):
    """the inverse of forward: a prefix sum (mod 2^w) or prefix xor that restarts every seg elements"""
    y, tail = _parts(data, esize)
    w, m = 8 * esize, y.size
    if filt == XOR:
        d, acc = y, np.bitwise_xor.accumulate
    else:
        ones = np.array((1 << w) - 1, dtype=y.dtype)
        d = (y >> np.array(1, y.dtype)) ^ np.where(y & np.array(1, y.dtype), ones, np.zeros((), y.dtype))
        acc = np.add.accumulate
    pad = np.zeros(-m % seg, dtype=y.dtype)
    x = acc(np.concatenate([d, pad]).reshape(-1, seg), axis=1, dtype=y.dtype).reshape(-1)[:m]
    return np.concatenate([x.astype(DT[esize]).view(np.uint8), tail])


def gen(kind, esize, m, t, seed):
    """m elements of `kind` and t tail bytes, as bytes:
    random: uniform words; monotone: a sorted series with small random steps; walk: a random walk of +-50 around the middle of
    the range; wrap: 0, 2^w - 1, 2^(w-1), 2^(w-1) - 1 in seeded random order, so that x - p and the zigzag overflow every way"""
    rng = np.random.default_rng(seed)
    w = 8 * esize
    dt = np.dtype(DT[esize])
    if kind == "random":
        x = rng.integers(0, 256, m * esize, dtype=np.uint8).view(dt)
    elif kind == "monotone":
        x = np.cumsum(rng.integers(0, 200, m, dtype=np.uint64), dtype=np.uint64).astype(dt)          # (16-bit: wraps every few hundred)
    elif kind == "walk":
        x = (np.uint64(1 << (w - 1)) + np.cumsum(rng.integers(-50, 51, m), dtype=np.int64).astype(np.uint64)).astype(dt)
    elif kind == "wrap":
        corners = np.array([0, (1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1], dtype=np.uint64).astype(dt)
        x = corners[rng.integers(0, 4, m)]
        x[:min(m, 8)] = np.resize(corners, min(m, 8))                                                # every neighbour pair at least once ...
        if m >= 24:
            x[8:24] = corners[[0, 2, 0, 3, 1, 3, 1, 0, 2, 1, 2, 2, 3, 3, 0, 0]]                      # ... in both orders
    else:
        raise ValueError(kind)
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()


def golden_cases():
    """(esize, filt, seg, m, t, kind): every width and filter, the restart lengths 256 / 320 / 4096, element counts around a
    vector and a restart, with and without tail bytes, every input kind"""
    cases = []
    for esize in ESIZES:
        for filt in FILTERS:
            for i, (seg, m) in enumerate(((256, 1), (256, 9), (256, 257), (320, 3 * 320 + 5), (4096, 4097), (4096, 3 * 4096 + 5))):
                cases.append((esize, filt, seg, m, (0, esize - 1)[i & 1], KINDS[(i + esize + filt) % 4]))
            cases.append((esize, filt, 256, 64, 0, "wrap"))
    return cases


def golden_seed(esize, filt, seg, m, t):
    return ((esize * 7 + filt) * 100003 + seg) * 1009 + 8 * m + t


def golden_input(case):
    esize, filt, seg, m, t, kind = case
    return gen(kind, esize, m, t, golden_seed(esize, filt, seg, m, t))


def load_golden():
    """-> [(case tuple, sha256 of the input, sha256 of F(input), F(input) as uint8 array or None)] of tests/golden/fplanes_vectors.npz"""
    z = np.load(GOLDEN)
    index = json.loads(bytes(z["index"]).decode())
    out = []
    for e in index:
        case = (e["esize"], e["filter"], e["seg"], e["m"], e["t"], e["kind"])
        n = e["m"] * e["esize"] + e["t"]
        out.append((case, e["in_sha256"], e["out_sha256"], z["out"][e["at"]:e["at"] + n] if e["at"] >= 0 else None))
    return out
