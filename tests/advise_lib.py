"""The planes advisor: the numpy model of trc_planes_hist_dev (byte histograms of every plane under every filter) and of
trc_planes_advise (order-0 estimates and the choice), and the input where xor must win.

Definition (include/trc_hip.h): hist[f, k, b] = the number of the m elements whose byte k under filter f equals b;
bits[f][k] = sum over b of c * log2(m / c); the choice is the requested filter with the smallest total, ties to the lower id, but
no filter where that was requested and the winner saves less than 1/64 of its total.
"""
import numpy as np

import fplanes_lib as FL
import planes_lib as PL

ALL = 7                                                        # the bit set of the three filters


def hist(data, esize, seg, filters):
    """-> uint64 [3, esize, 256]; rows of filters outside the bit set `filters` are zero.  The tail bytes are in no plane."""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    d = d[:d.size // esize * esize]
    h = np.zeros((3, esize, 256), dtype=np.uint64)
    for f in (FL.NONE, FL.ZDELTA, FL.XOR):
        if filters >> f & 1:
            planes, _ = PL.split(d if f == FL.NONE else FL.forward(d, esize, f, seg), esize)
            for k in range(esize):
                h[f, k] = np.bincount(planes[k], minlength=256)
    return h


def estimate(h, filters, esize, m):
    """-> bits float64 [3, 8] (zero beyond esize and for filters not requested)"""
    bits = np.zeros((3, 8))
    for f in range(3):
        if filters >> f & 1:
            for k in range(esize):
                c = h[f, k][h[f, k] > 0].astype(np.float64)
                bits[f, k] = float(np.sum(c * np.log2(m / c)))
    return bits


def advise(h, filters, esize, m):
    """-> (choice, bits [3, 8], total_bits [3])"""
    bits = estimate(np.asarray(h).reshape(3, esize, 256), filters, esize, m)
    total = bits.sum(axis=1)
    asked = [f for f in range(3) if filters >> f & 1]
    best = min(asked, key=lambda f: (total[f], f))
    if filters & 1 and best != FL.NONE and total[FL.NONE] - total[best] < total[FL.NONE] / 64:
        best = FL.NONE
    return best, bits, total


def bitflip(esize, m, t, seed):
    """x[i] = x[i - 1] ^ (1 << r_i), r_i seeded uniform in [0, 8 * esize): neighbours differ in one bit, anywhere in the word, so the
    xor of neighbours has one of 8 * esize values while their difference is spread over twice as many; t tail bytes follow"""
    rng = np.random.default_rng(seed)
    flips = np.left_shift(np.uint64(1), rng.integers(0, 8 * esize, m).astype(np.uint64))
    flips[0] = rng.integers(0, 1 << 16)
    x = np.bitwise_xor.accumulate(flips).astype(FL.DT[esize])
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])


def gen(kind, esize, m, t, seed):
    """fplanes_lib.gen plus the kinds `bitflip` and `weights`"""
    if kind == "bitflip":
        return bitflip(esize, m, t, seed)
    if kind == "weights":
        return np.concatenate([PL.weights(m, esize, seed), np.random.default_rng(seed).integers(0, 256, t, dtype=np.uint8)])
    return FL.gen(kind, esize, m, t, seed)
