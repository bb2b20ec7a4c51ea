"""Batched byte planes with a predictor filter and a STRIDE per item: the numpy definition of VS(items, filters, strides, esize,
chunk) (include/trc_hip.h), built from the virtual buffer of planes_batch_lib and the strided filter model of splanes_lib, and the
stride assignments of its tests.

    GS(i) = item i where filters[i] == NONE (strides[i] has no effect), else F_{strides[i]}(filters[i], seg = chunk, esize, item i)
    VS = V([GS(0), .., GS(count - 1)])

Every item is filtered as if it stood alone, then the virtual buffer is built as before: the pad behind an item is zero bytes,
and plan, M, NC, first[] and pitch are those of the unfiltered batch."""
import numpy as np

import planes_batch_lib as BL
import splanes_lib as SL

STRIDE_MAX = SL.STRIDE_MAX


def filtered(items, filters, strides, esize, chunk):
    """[GS(0), .., GS(count - 1)]"""
    assert len(filters) == len(items) == len(strides)
    return [np.ascontiguousarray(d, dtype=np.uint8) if f == SL.NONE else SL.forward(d, esize, f, chunk, s)
            for d, f, s in zip(items, filters, strides)]


def virtual_filtered(items, filters, strides, esize, chunk):
    """VS: the virtual buffer of the items filtered one by one, each at its stride"""
    return BL.virtual(filtered(items, filters, strides, esize, chunk), esize, chunk)


def item_of(vs, i, sizes, filt, stride, esize, chunk):
    """item i back from its own chunk range of VS alone"""
    _, first = BL.plan(sizes, esize, chunk)
    g = vs[first[i] * chunk * esize:first[i] * chunk * esize + sizes[i]]
    return g if filt == SL.NONE else SL.inverse(g, esize, filt, chunk, stride)


def stride_assignments(count, seed):
    """the stride assignments of the tests: uniform 3, uniform 8, the cycle (1, 2, .. 8, 1, ..), one seeded random assignment in 1 .. 8"""
    rng = np.random.default_rng(seed)
    return {"3": [3] * count, "8": [8] * count, "cycle": [1 + i % STRIDE_MAX for i in range(count)],
            "random": [int(x) for x in rng.integers(1, STRIDE_MAX + 1, count)]}


def filter_assignments(count):
    """the filter assignments that go with them: all delta, all xor, the cycle (0, 1, 2, ..)"""
    return {"delta": [SL.ZDELTA] * count, "xor": [SL.XOR] * count, "cycle": [i % 3 for i in range(count)]}


def table_batch(rows=4096, seed=7):
    """the torch helper's batch as int32 / float32 arrays: a [rows, 4] table (sorted id, two timestamps, a counter), a plain sorted-id
    column and a float column -> (arrays, filters, strides)"""
    rng = np.random.default_rng(seed)
    table = np.frombuffer(SL.table_rows(rows, rng).tobytes(), dtype="<i4").reshape(rows, 4).copy()
    ids = (np.cumsum(rng.integers(1, 200, 5000)) + 1000).astype("<i4")
    values = rng.standard_normal(3000).astype("<f4")
    return [table, ids, values], [1, 1, 0], [4, 1, 1]
