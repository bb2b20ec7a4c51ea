"""Strided zigzag-delta / xor filters in front of the byte planes, for interleaved data: the numpy model F_S (and its inverse) that
the strided planar calls are checked against, a per-element restatement of the definition in Python integers, the inputs of the
tests, and the fixture tests/golden/splanes_vectors.npz that pins the model.

Definition (include/trc_hip.h): the m = n // esize elements x[i] are little-endian unsigned words of w = 8 * esize bits, the
t = n % esize tail bytes are never filtered; with a stride S in 1 .. 8:  p[i] = 0 where i % seg < S, else x[i - S];
    ZDELTA: d = x[i] - p[i] mod 2^w, y[i] = (d << 1) ^ (0 - (d >> (w - 1)))        XOR: y[i] = x[i] ^ p[i]
F_S(filter, seg, esize, in) = the y's followed by the tail; F_1 is fplanes_lib's F.  As for F there is no reference implementation
to compare with, so the definition is the only source and this model the yardstick.
"""
import json
import os

import numpy as np

import fplanes_lib as FL

ESIZES, FILTERS, DT = FL.ESIZES, FL.FILTERS, FL.DT
NONE, ZDELTA, XOR = FL.NONE, FL.ZDELTA, FL.XOR
STRIDES = (2, 3, 4, 5, 6, 7, 8)
STRIDE_MAX = 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splanes_vectors.npz")
GOLDEN_STORE_MAX = FL.GOLDEN_STORE_MAX


def forward(data, esize, filt, seg, stride):
    """F_stride(filt, seg, esize, data) as uint8 array of the same length"""
    x, tail = FL._parts(data, esize)
    w, m = 8 * esize, x.size
    p = np.concatenate([np.zeros(stride, x.dtype), x])[:m]
    p[np.arange(m) % seg < stride] = 0
    if filt == XOR:
        y = x ^ p
    else:
        d = x - p                                              # unsigned: wraps mod 2^w
        ones = np.array((1 << w) - 1, dtype=x.dtype)
        y = (d << np.array(1, x.dtype)) ^ np.where(d >> np.array(w - 1, x.dtype), ones, np.zeros((), x.dtype))
    return np.concatenate([y.astype(DT[esize]).view(np.uint8), tail])


def inverse(data, esize, filt, seg, stride):
    """the inverse of forward: `stride` interleaved prefix sums (mod 2^w) or prefix xors that restart every seg elements"""
    y, tail = FL._parts(data, esize)
    w, m = 8 * esize, y.size
    if filt == XOR:
        d, acc = y, np.bitwise_xor.accumulate
    else:
        ones = np.array((1 << w) - 1, dtype=y.dtype)
        d = (y >> np.array(1, y.dtype)) ^ np.where(y & np.array(1, y.dtype), ones, np.zeros((), y.dtype))
        acc = np.add.accumulate
    rows = -(-seg // stride)                                   # a segment as rows of `stride` classes, the last row padded
    nseg = -(-m // seg)
    a = np.zeros((nseg, rows * stride), dtype=y.dtype)
    flat = np.zeros(nseg * seg, dtype=y.dtype)
    flat[:m] = d
    a[:, :seg] = flat.reshape(nseg, seg)
    x = acc(a.reshape(nseg, rows, stride), axis=1, dtype=y.dtype).reshape(nseg, rows * stride)[:, :seg].reshape(-1)[:m]
    return np.concatenate([x.astype(DT[esize]).view(np.uint8), tail])


def scalar_forward(data, esize, filt, seg, stride):
    """the definition, one element at a time in Python integers"""
    w, mask = 8 * esize, (1 << (8 * esize)) - 1
    m = len(data) // esize
    xs = [int.from_bytes(bytes(data[i * esize:(i + 1) * esize]), "little") for i in range(m)]
    out = bytearray()
    for i, x in enumerate(xs):
        p = 0 if i % seg < stride else xs[i - stride]
        if filt == XOR:
            y = x ^ p
        else:
            d = (x - p) & mask
            y = ((d << 1) ^ (0 - (d >> (w - 1)))) & mask
        out += y.to_bytes(esize, "little")
    return np.frombuffer(bytes(out) + bytes(data[m * esize:]), dtype=np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def interleaved(k, esize, m, t, seed, step=50):
    """m elements that weave k series element by element, and t tail bytes: series c is a random walk of +-step (even c) or a
    monotone series with steps below 4 * step (odd c) around an offset of its own, the offsets (c + 1) / (k + 1) of the range
    apart, so that neighbours of different series differ in the high byte planes"""
    rng = np.random.default_rng(seed)
    w = 8 * esize
    rows = -(-m // k)
    cols = []
    for c in range(k):
        base = ((c + 1) << w) // (k + 1)
        if c & 1:
            s = np.cumsum(rng.integers(0, 4 * step, rows), dtype=np.int64)
        else:
            s = np.cumsum(rng.integers(-step, step + 1, rows), dtype=np.int64)
        cols.append(s.astype(np.uint64) + np.uint64(base))                        # (wraps mod 2^64)
    x = np.stack(cols, axis=1).reshape(-1)[:m].astype(DT[esize])                  # (mod 2^w)
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])


KINDS = FL.KINDS + ("interleaved",)


def gen(kind, esize, m, t, seed, stride=1):
    """fplanes_lib.gen's kinds, plus "interleaved": `stride` woven series"""
    if kind == "interleaved":
        return interleaved(stride, esize, m, t, seed)
    return FL.gen(kind, esize, m, t, seed)


# the three inputs of the estimate table (2^20 elements each): (name, esize, matching stride, bytes)
def table_inputs(m=1 << 20):
    rng = np.random.default_rng(2024)
    out = []

    def fold(x, r=1024):                                       # a walk reflected at +-r: it stays with its offset however long it is
        return np.abs((x + r) % (4 * r) - 2 * r) - r
    walks = [off + fold(np.cumsum(rng.integers(-50, 51, m // 3 + 1))) for off in (1000, 20000, 40000)]
    out.append(("3 x int16 walk", 2, 3, np.stack(walks, axis=1).reshape(-1)[:m].astype(np.int64).astype("<u2").view(np.uint8)))
    walks = [off + np.cumsum(rng.integers(-200, 201, m // 2)) for off in (5000, 30000)]
    out.append(("2 x int16 walk", 2, 2, np.stack(walks, axis=1).reshape(-1)[:m].astype(np.int64).astype("<u2").view(np.uint8)))
    out.append(("4 x u32 fields", 4, 4, table_rows(m // 4, rng)))
    return out


def table_rows(rows, rng=None):
    """rows of 4 u32 fields, row-major: a sorted id, two timestamps (one a little behind the other), a counter"""
    rng = rng or np.random.default_rng(2024)
    ident = np.cumsum(rng.integers(1, 40, rows), dtype=np.int64) + 100000
    t0 = 1700000000 + np.cumsum(rng.integers(0, 3, rows), dtype=np.int64)
    t1 = t0 + rng.integers(0, 900, rows)
    cnt = np.cumsum(rng.integers(0, 2, rows), dtype=np.int64)
    return np.ascontiguousarray(np.stack([ident, t0, t1, cnt], axis=1).reshape(-1).astype("<u4")).view(np.uint8)


def plane_hist(data, esize):
    """uint64 [esize, 256]: the byte histogram of every plane of data's whole elements"""
    m = data.size // esize
    b = np.ascontiguousarray(data[:m * esize]).reshape(m, esize)
    return np.stack([np.bincount(b[:, k], minlength=256) for k in range(esize)]).astype(np.uint64)


def hist3(data, esize, seg, stride):
    """what trc_planes_hist_stride_dev(7, stride, ...) leaves: uint64 [3 * esize * 256], rows of none, zigzag delta, xor"""
    return np.concatenate([plane_hist(data, esize).reshape(-1)] +
                          [plane_hist(forward(data, esize, f, seg, stride), esize).reshape(-1) for f in FILTERS])


def bits_per_byte(hist_rows, m, esize):
    """order-0 estimate of the planes `hist_rows` (uint64 [esize, 256]) in bits per input byte"""
    c = hist_rows.astype(np.float64)
    nz = c > 0
    return float((c[nz] * np.log2(m / c[nz])).sum()) / (m * esize)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def golden_cases():
    """(esize, filt, stride, seg, m, t, kind): every width, filter and stride; restart lengths 256 / 320 / 4096, element counts
    around the stride, a vector and a restart, with and without tail bytes, every input kind"""
    cases = []
    for esize in ESIZES:
        for filt in FILTERS:
            for stride in STRIDES:
                shapes = ((256, 1), (256, stride), (256, stride + 1), (256, 9), (256, 257), (320, 3 * 320 + 5), (4096, 4097), (4096, 3 * 4096 + 5))
                for i in ((stride + esize) % 4, 4 + (stride + filt) % 4):          # two shapes per (esize, filt, stride): all eight per stride pair
                    seg, m = shapes[i]
                    cases.append((esize, filt, stride, seg, m, (0, esize - 1)[(i + stride) & 1], KINDS[(i + esize + filt + stride) % 5]))
            cases.append((esize, filt, 3, 256, 64, 0, "wrap"))
    return cases


def golden_seed(esize, filt, stride, seg, m, t):
    return (((esize * 7 + filt) * 11 + stride) * 100003 + seg) * 1009 + 8 * m + t


def golden_input(case):
    esize, filt, stride, seg, m, t, kind = case
    return gen(kind, esize, m, t, golden_seed(esize, filt, stride, seg, m, t), stride)


def load_golden():
    """-> [(case tuple, sha256 of the input, sha256 of F_S(input), F_S(input) as uint8 array or None)] of the fixture"""
    z = np.load(GOLDEN)
    index = json.loads(bytes(z["index"]).decode())
    out = []
    for e in index:
        case = (e["esize"], e["filter"], e["stride"], e["seg"], e["m"], e["t"], e["kind"])
        n = e["m"] * e["esize"] + e["t"]
        out.append((case, e["in_sha256"], e["out_sha256"], z["out"][e["at"]:e["at"] + n] if e["at"] >= 0 else None))
    return out


sha = FL.sha
