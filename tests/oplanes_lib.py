"""Predictors of order 2 and 3 in front of the byte planes, for smooth series: the numpy model O (and its inverse) that the order
calls are checked against, an independent per-element restatement of the closed form in Python integers, the inputs of the tests
and of the estimate table, the model of the order advisor, and the fixture tests/golden/oplanes_vectors.npz that pins the model.

Definition (include/trc_hip.h): the m = n // esize elements x[i] are little-endian unsigned words of w = 8 * esize bits, the
t = n % esize tail bytes are never filtered; with a stride S in 1 .. 8 and an order K in 0 .. 3:
    D_S(a)[i] = a[i] where i % seg < S,  a[i] - a[i - S] mod 2^w elsewhere
    y[i] = zigzag(D_S applied K times to x, at i),  zigzag(d) = (d << 1) ^ (0 - (d >> (w - 1)))
O(K, S, seg, esize, in) = the y's followed by the tail.  The closed form, with x zero in front of its segment:
    D^K[i] = sum_j (-1)^j C(K, j) x[i - j S]
forward() applies D_S K times, scalar_forward() evaluates the closed form: two routes to one result.  There is no reference
implementation of such a filter, so the definition is the only source and this model the yardstick.
"""
import json
import math
import os

import numpy as np

import fplanes_lib as FL
import splanes_lib as SL

ESIZES, DT = FL.ESIZES, FL.DT
ORDERS = (2, 3)
ORDER_MAX = 3
STRIDES = (1, 2, 3, 5, 8)                                      # the fixture's and golden_cases()': pinned
ALL_STRIDES = tuple(range(1, 9))                               # every entry of the kernels' dispatch tables
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oplanes_vectors.npz")
GOLDEN_STORE_MAX = FL.GOLDEN_STORE_MAX


def _d(a, seg, stride):
    m = a.size
    p = np.concatenate([np.zeros(stride, a.dtype), a])[:m]
    p[np.arange(m) % seg < stride] = 0
    return a - p                                               # unsigned: wraps mod 2^w


def _zigzag(d, w):
    ones = np.array((1 << w) - 1, dtype=d.dtype)
    return (d << np.array(1, d.dtype)) ^ np.where(d >> np.array(w - 1, d.dtype), ones, np.zeros((), d.dtype))


def _unzigzag(y, w):
    ones = np.array((1 << w) - 1, dtype=y.dtype)
    return (y >> np.array(1, y.dtype)) ^ np.where(y & np.array(1, y.dtype), ones, np.zeros((), y.dtype))


def forward(data, esize, order, seg, stride):
    """O(order, stride, seg, esize, data) as uint8 array of the same length; order 0: the data"""
    x, tail = FL._parts(data, esize)
    if order == 0:
        return np.concatenate([x.view(np.uint8), tail])
    d = x
    for _ in range(order):
        d = _d(d, seg, stride)
    return np.concatenate([_zigzag(d, 8 * esize).astype(DT[esize]).view(np.uint8), tail])


def _sums(d, seg, stride):
    """`stride` interleaved prefix sums mod 2^w that restart every seg elements"""
    m = d.size
    rows = -(-seg // stride)                                   # a segment as rows of `stride` classes, the last row padded
    nseg = -(-m // seg)
    a = np.zeros((nseg, rows * stride), dtype=d.dtype)
    flat = np.zeros(nseg * seg, dtype=d.dtype)
    flat[:m] = d
    a[:, :seg] = flat.reshape(nseg, seg)
    return np.add.accumulate(a.reshape(nseg, rows, stride), axis=1, dtype=d.dtype).reshape(nseg, rows * stride)[:, :seg].reshape(-1)[:m]


def inverse(data, esize, order, seg, stride):
    """the inverse of forward: undo the zigzag, then `order` class-wise segmented prefix sums from a zero state"""
    y, tail = FL._parts(data, esize)
    if order == 0:
        return np.concatenate([y.view(np.uint8), tail])
    d = _unzigzag(y, 8 * esize)
    for _ in range(order):
        d = _sums(d, seg, stride)
    return np.concatenate([d.astype(DT[esize]).view(np.uint8), tail])


def scalar_forward(data, esize, order, seg, stride):
    """the closed form, one element at a time in Python integers"""
    w, mask = 8 * esize, (1 << (8 * esize)) - 1
    m = len(data) // esize
    xs = [int.from_bytes(bytes(data[i * esize:(i + 1) * esize]), "little") for i in range(m)]
    out = bytearray()
    for i, x in enumerate(xs):
        if order == 0:
            y = x
        else:
            d = 0
            for j in range(order + 1):
                if i % seg >= j * stride:                      # (x is zero in front of its segment)
                    d += (-1) ** j * math.comb(order, j) * xs[i - j * stride]
            d &= mask
            y = ((d << 1) ^ (0 - (d >> (w - 1)))) & mask
        out += y.to_bytes(esize, "little")
    return np.frombuffer(bytes(out) + bytes(data[m * esize:]), dtype=np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
KINDS = ("random", "smooth", "wrap", "ones")


def smooth(k, esize, m, t, seed):
    """m elements that weave k smooth series element by element (three sines and a little noise each, around the middle of the
    range, at amplitudes that use the upper planes), and t tail bytes"""
    rng = np.random.default_rng(seed)
    w = 8 * esize
    rows = -(-m // k)
    i = np.arange(rows, dtype=np.float64)
    amp = float(1 << min(w - 3, 28))
    cols = []
    for c in range(k):
        s = amp * np.sin(0.013 * i + c) + amp / 2 * np.sin(0.071 * i + 2 * c) + amp / 8 * np.sin(0.31 * i) + rng.normal(0, 6, rows)
        cols.append(np.rint(s).astype(np.int64).astype(np.uint64) + np.uint64(1 << (w - 1)))
    x = np.stack(cols, axis=1).reshape(-1)[:m].astype(DT[esize])
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])


def gen(kind, esize, m, t, seed, stride=1):
    """random: uniform words; smooth: `stride` woven smooth series; wrap: fplanes_lib's corners 0, 2^w - 1, 2^(w-1), 2^(w-1) - 1, so
    that every level of the difference and of the sums overflows; ones: every byte 0xff, the tail included"""
    if kind == "smooth":
        return smooth(stride, esize, m, t, seed)
    if kind == "ones":
        return np.full(m * esize + t, 0xFF, dtype=np.uint8)
    return FL.gen(kind, esize, m, t, seed)


def table_inputs(m=1 << 20):
    """the five inputs of the estimate table: (name, esize, stride, bytes) of m elements each"""
    rng = np.random.default_rng(2025)
    i = np.arange(m, dtype=np.float64)

    def pcm(j, phase=0.0):
        return 6000 * np.sin(0.013 * j + phase) + 3000 * np.sin(0.071 * j + 2 * phase) + 800 * np.sin(0.31 * j + 3 * phase) + rng.normal(0, 6, j.size)

    def u(x, dt):
        return np.ascontiguousarray(np.rint(x).astype(np.int64).astype(dt)).view(np.uint8)
    out = [("16-bit PCM-like", 2, 1, u(pcm(i), "<u2"))]
    half = np.arange(m // 2, dtype=np.float64)
    out.append(("the same as interleaved stereo", 2, 2, u(np.stack([pcm(half), pcm(half, 0.4)], axis=1).reshape(-1), "<u2")))
    out.append(("u32 sensor series", 4, 1, u((1 << 20) + 2e5 * np.sin(0.002 * i) + 5e4 * np.sin(0.02 * i) + rng.normal(0, 3, m), "<u4")))
    out.append(("u32 timestamps, step 1000 +- 2", 4, 1, u(1700000000 + np.cumsum(1000 + rng.integers(-2, 3, m)), "<u4")))
    out.append(("sorted u32 ids, gaps 1..29", 4, 1, u(np.cumsum(rng.integers(1, 30, m)), "<u4")))
    return out


# ---- the histograms and the advisor ---------------------------------------------------------------------------------------
def hist4(data, esize, seg, stride, orders=15):
    """what trc_planes_hist_order_dev(orders, stride, ...) leaves: uint64 [4 * esize * 256], rows of orders 0 .. 3, zeros where
    an order is not requested"""
    rows = [SL.plane_hist(forward(data, esize, k, seg, stride), esize) if orders >> k & 1 else np.zeros((esize, 256), np.uint64) for k in range(4)]
    return np.concatenate([r.reshape(-1) for r in rows])


def estimates(hist, esize, m):
    """order-0 model estimate per order in bits: float64 [4], sum over the planes and bins of c * log2(m / c)"""
    c = np.asarray(hist, dtype=np.float64).reshape(4, esize * 256)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, c * np.log2(m / np.where(c > 0, c, 1)), 0.0).sum(axis=1)


def advise(hist, orders, esize, m):
    """the rule of trc_planes_advise_order on such histograms -> the order: the requested order with the smallest total, ties to the
    lower order; order 0 where it was requested and the winner saves less than 1/64 of its total"""
    tot = estimates(hist, esize, m)
    best = None
    for k in range(4):
        if orders >> k & 1 and (best is None or tot[k] < tot[best]):
            best = k
    if orders & 1 and best != 0 and tot[0] - tot[best] < tot[0] / 64:
        best = 0
    return best


# ---- the fixture ----------------------------------------------------------------------------------------------------------
SHAPES = ((256, 5), (256, 9), (256, 2 * 256 + 7), (320, 3 * 320 + 9), (512, 1024 + 1), (256, 2049 + 5))


def golden_cases():
    """(esize, order, stride, seg, m, t, kind): every width, order and stride of the tests; restart lengths 256 / 320 / 512, element
    counts below ORDER * S, around a vector, a restart and a span, with and without tail bytes, every input kind"""
    cases = []
    for esize in ESIZES:
        for order in ORDERS:
            for s, stride in enumerate(STRIDES):
                i = (s + order + esize) % len(SHAPES)
                seg, m = SHAPES[i]
                cases.append((esize, order, stride, seg, m, (0, esize - 1)[(i + s) & 1], KINDS[len(cases) % len(KINDS)]))
            cases.append((esize, order, 3, 256, 64, 0, "wrap"))
    return cases


def golden_seed(esize, order, stride, seg, m, t):
    return (((esize * 7 + order) * 11 + stride) * 100003 + seg) * 1009 + 8 * m + t


def golden_input(case):
    esize, order, stride, seg, m, t, kind = case
    return gen(kind, esize, m, t, golden_seed(esize, order, stride, seg, m, t), stride)


def load_golden():
    """-> [(case tuple, sha256 of the input, sha256 of O(input), O(input) as uint8 array or None)] of the fixture"""
    z = np.load(GOLDEN)
    index = json.loads(bytes(z["index"]).decode())
    out = []
    for e in index:
        case = (e["esize"], e["order"], e["stride"], e["seg"], e["m"], e["t"], e["kind"])
        n = e["m"] * e["esize"] + e["t"]
        out.append((case, e["in_sha256"], e["out_sha256"], z["out"][e["at"]:e["at"] + n] if e["at"] >= 0 else None))
    return out


sha = FL.sha
