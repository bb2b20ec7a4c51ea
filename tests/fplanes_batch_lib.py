"""Batched byte planes with a predictor filter per item: the numpy definition of VF(items, filters, esize, chunk) (include/trc_hip.h),
built from the virtual buffer of planes_batch_lib and the filter model of fplanes_lib, and the inputs of its tests.

    G(i) = item i where filters[i] == NONE, else F(filters[i], seg = chunk, esize, item i);   VF = V([G(0), .., G(count - 1)])

Every item is filtered as if it stood alone, then the virtual buffer is built as before: the pad behind an item is zero bytes,
and plan, M, NC, first[] and pitch are those of the unfiltered batch."""
import numpy as np

import fplanes_lib as FL
import planes_batch_lib as BL

KINDS = ("random", "wrap")                                     # every byte carries / x - p and the zigzag overflow every way


def filtered(items, filters, esize, chunk):
    """[G(0), .., G(count - 1)]"""
    assert len(filters) == len(items)
    return [np.ascontiguousarray(d, dtype=np.uint8) if f == FL.NONE else FL.forward(d, esize, f, chunk) for d, f in zip(items, filters)]


def virtual_filtered(items, filters, esize, chunk):
    """VF: the virtual buffer of the items filtered one by one"""
    return BL.virtual(filtered(items, filters, esize, chunk), esize, chunk)


def item_of(vf, i, sizes, filt, esize, chunk):
    """item i back from its own chunk range of VF alone"""
    _, first = BL.plan(sizes, esize, chunk)
    g = vf[first[i] * chunk * esize:first[i] * chunk * esize + sizes[i]]
    return g if filt == FL.NONE else FL.inverse(g, esize, filt, chunk)


def gen_items(esize, order, seed):
    """items of `order` elements each, FL.gen kinds random and wrap alternating by item"""
    return [FL.gen(KINDS[i % 2], esize, m, 0, seed + i) for i, m in enumerate(order)]


def assignments(count, seed):
    """the filter assignments of the tests: all delta, all xor, the cycle (0, 1, 2, ..), one seeded random assignment"""
    rng = np.random.default_rng(seed)
    return {"delta": [FL.ZDELTA] * count, "xor": [FL.XOR] * count, "cycle": [i % 3 for i in range(count)],
            "random": [int(x) for x in rng.integers(0, 3, count)]}
