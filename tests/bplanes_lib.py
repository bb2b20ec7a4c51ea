"""Zigzag-delta and xor filters against a BASE buffer in front of the byte planes: the numpy model D (and its inverse) that the
base planar calls are checked against, the fingerprint by which a container names its base, and the inputs of the tests.

Definition (include/trc_hip.h): x[i], b[i] = the m = n // esize elements of `data` and of `base`, little-endian unsigned words of
w = 8 * esize bits; the t = n % esize tail bytes of `data` are never filtered, of the base only m * esize bytes are looked at;
    ZDELTA: d = x[i] - b[i] mod 2^w, y[i] = (d << 1) ^ (0 - (d >> (w - 1)))        XOR: y[i] = x[i] ^ b[i]
D(filter, esize, data, base) = the y's followed by the tail.
    fingerprint: fp = sum_j (2j + 1) * w_j + nbytes * 0x9E3779B97F4A7C15 mod 2^64 over the little-endian u64 words of the bytes,
    zero-padded to 8.
"""
import numpy as np

import fplanes_lib as FL
import planes_lib as PL
from fplanes_lib import DT, ESIZES, FILTERS, NONE, XOR, ZDELTA  # noqa: F401 (for the test files)

KINDS = ("wrap", "random", "same", "drift")
FP_LEN_MUL = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def _parts(data, esize):
    d = np.ascontiguousarray(data, dtype=np.uint8)
    m = d.size // esize
    return d[:m * esize].view(DT[esize]), d[m * esize:]


def forward(data, base, esize, filt):
    """D(filt, esize, data, base) as uint8 array of data's length; base: at least m * esize bytes"""
    x, tail = _parts(data, esize)
    b = np.ascontiguousarray(base, dtype=np.uint8)[:x.size * esize].view(DT[esize])
    w = 8 * esize
    if filt == NONE:
        y = x
    elif filt == XOR:
        y = x ^ b
    else:
        d = x - b                                              # unsigned: wraps mod 2^w
        ones = np.array((1 << w) - 1, dtype=x.dtype)
        y = (d << np.array(1, x.dtype)) ^ np.where(d >> np.array(w - 1, x.dtype), ones, np.zeros((), x.dtype))
    return np.concatenate([y.astype(DT[esize]).view(np.uint8), tail])


def inverse(data, base, esize, filt):
    """the inverse of forward: elementwise, no scan"""
    y, tail = _parts(data, esize)
    b = np.ascontiguousarray(base, dtype=np.uint8)[:y.size * esize].view(DT[esize])
    w = 8 * esize
    if filt == NONE:
        x = y
    elif filt == XOR:
        x = y ^ b
    else:
        ones = np.array((1 << w) - 1, dtype=y.dtype)
        x = b + ((y >> np.array(1, y.dtype)) ^ np.where(y & np.array(1, y.dtype), ones, np.zeros((), y.dtype)))
    return np.concatenate([x.astype(DT[esize]).view(np.uint8), tail])


def fingerprint(data):
    """the fingerprint of these bytes, in Python integers word by word for short inputs and in wrapping uint64 arithmetic for long ones"""
    d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    n = d.size
    words = np.concatenate([d, np.zeros(-n % 8, np.uint8)]).view("<u8")
    if n <= 4096:
        return (sum((2 * j + 1) * int(w) for j, w in enumerate(words)) + n * FP_LEN_MUL) & MASK64
    with np.errstate(over="ignore"):
        s = int(np.sum((np.arange(words.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * words, dtype=np.uint64))
    return (s + n * FP_LEN_MUL) & MASK64


def _cut(w, esize):
    """float64 values as the bytes of bf16 / fp32 / fp64, exactly as planes_lib.weights cuts them"""
    if esize == 8:
        return w.astype("<f8").view(np.uint8)
    b = w.astype("<f4").view(np.uint8)
    if esize == 4:
        return b.copy()
    return np.ascontiguousarray(b.reshape(w.size, 4)[:, 2:]).reshape(-1)


def pair(m, esize, seed, step):
    """-> (base, data): planes_lib.weights(m, esize, seed) and the same weights plus N(0, step^2) noise of seed + 1, cut to the
    same dtype: a checkpoint and its successor, a base model and its fine-tune"""
    w = np.random.default_rng(seed).normal(0.0, 0.02, m)
    noise = np.random.default_rng(seed + 1).normal(0.0, step, m)
    return _cut(w, esize), _cut(w + noise, esize)


def gen_pair(kind, esize, m, t, seed):
    """-> (data: m elements and t tail bytes, base: m elements), as bytes:
    wrap: both from fplanes_lib's corner values with different seeds, so that x - b and the zigzag overflow every way;
    random: unrelated uniform words; same: data == base, every plane zero; drift: base a random walk, data = base + a small step"""
    rng = np.random.default_rng(seed + 77)
    if kind == "wrap":
        data, base = FL.gen("wrap", esize, m, t, seed), FL.gen("wrap", esize, m, 0, seed + 1)
    elif kind == "random":
        data, base = FL.gen("random", esize, m, t, seed), FL.gen("random", esize, m, 0, seed + 1)
    elif kind == "same":
        data = FL.gen("random", esize, m, t, seed)
        base = data[:m * esize].copy()
    elif kind == "drift":
        base = FL.gen("walk", esize, m, 0, seed)
        x = base.view(DT[esize]) + rng.integers(-3, 4, m).astype(np.int64).astype(np.uint64).astype(DT[esize])
        data = np.concatenate([x.astype(DT[esize]).view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])
    else:
        raise ValueError(kind)
    return data, base


def hist(data, base, esize, filters):
    """the model of trc_planes_hist_base_dev -> uint64 [3, esize, 256]; rows of filters outside the bit set are zero"""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    d = d[:d.size // esize * esize]
    h = np.zeros((3, esize, 256), dtype=np.uint64)
    for f in (NONE, ZDELTA, XOR):
        if filters >> f & 1:
            planes, _ = PL.split(forward(d, base, esize, f), esize)
            for k in range(esize):
                h[f, k] = np.bincount(planes[k], minlength=256)
    return h


def order0_bytes(data, esize):
    """the order-0 estimate of the byte planes of `data`, in bytes"""
    planes, _ = PL.split(data, esize)
    bits = 0.0
    for k in range(esize):
        c = np.bincount(planes[k], minlength=256).astype(np.float64)
        c = c[c > 0]
        bits += float(np.sum(c * np.log2(planes.shape[1] / c)))
    return bits / 8


# ---- a base per item of a batch ----------------------------------------------------------------------------------------------
def filtered_batch(items, bases, filters, esize):
    """[G(0), .., G(count - 1)]: item i where filters[i] == NONE (bases[i] is not looked at), else D(filters[i], esize, item i, bases[i])"""
    assert len(items) == len(bases) == len(filters)
    return [np.ascontiguousarray(d, dtype=np.uint8) if f == NONE else forward(d, b, esize, f) for d, b, f in zip(items, bases, filters)]


def virtual_batch(items, bases, filters, esize, chunk):
    """the virtual buffer (planes_batch_lib) of the items filtered one by one against their bases; the pad stays zero"""
    import planes_batch_lib as BL
    return BL.virtual(filtered_batch(items, bases, filters, esize), esize, chunk)


def gen_batch(esize, order, seed):
    """-> (items, bases) of `order` elements each, the kinds of gen_pair rotating by item"""
    pairs = [gen_pair(KINDS[i % 4], esize, m, 0, seed + i) for i, m in enumerate(order)]
    return [p[0] for p in pairs], [p[1] for p in pairs]
