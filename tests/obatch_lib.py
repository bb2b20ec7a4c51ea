"""Batched byte planes with a filter, a stride and a predictor ORDER per item: the numpy definition of VO(items, filters, strides,
orders, esize, chunk) (include/trc_hip.h), built from the virtual buffer of planes_batch_lib, the strided filter model of splanes_lib
and the order model of oplanes_lib; the order assignments of its tests; the TRCU container's prefix; and the estimate table of
profiles/planes/obatch_notes.md (python tests/obatch_lib.py prints it).

    GO(i) = item i                                                    where filters[i] == NONE
          = F_{strides[i]}(XOR, seg = chunk, esize, item i)           where filters[i] == XOR     (orders[i] has no effect)
          = O(orders[i], strides[i], seg = chunk, esize, item i)      where filters[i] == ZDELTA
    VO = V([GO(0), .., GO(count - 1)])

Every item is filtered as if it stood alone, then the virtual buffer is built as before: the pad behind an item is zero bytes,
and plan, M, NC, first[] and pitch are those of the unfiltered batch."""
import struct

import numpy as np

import oplanes_lib as OL
import planes_batch_lib as BL
import splanes_lib as SL

ORDER_MAX = OL.ORDER_MAX
MAGIC = 0x55435254                                             # "TRCU"
ORDER_NAMES = ("2", "3", "cycle", "random")


def filtered(items, filters, strides, orders, esize, chunk):
    """[GO(0), .., GO(count - 1)]"""
    assert len(filters) == len(items) == len(strides) == len(orders)
    out = []
    for d, f, s, k in zip(items, filters, strides, orders):
        if f == SL.NONE:
            out.append(np.ascontiguousarray(d, dtype=np.uint8))
        elif f == SL.XOR:
            out.append(SL.forward(d, esize, f, chunk, s))
        else:
            out.append(OL.forward(d, esize, k, chunk, s))
    return out


def virtual_filtered(items, filters, strides, orders, esize, chunk):
    """VO: the virtual buffer of the items filtered one by one, each at its stride and order"""
    return BL.virtual(filtered(items, filters, strides, orders, esize, chunk), esize, chunk)


def item_of(vo, i, sizes, filt, stride, order, esize, chunk):
    """item i back from its own chunk range of VO alone"""
    _, first = BL.plan(sizes, esize, chunk)
    g = vo[first[i] * chunk * esize:first[i] * chunk * esize + sizes[i]]
    if filt == SL.NONE:
        return g
    return SL.inverse(g, esize, filt, chunk, stride) if filt == SL.XOR else OL.inverse(g, esize, order, chunk, stride)


def order_assignments(count, seed):
    """the order assignments of the tests: uniform 2, uniform 3, the cycle (1, 2, 3, 1, ..), one seeded random assignment in 1 .. 3"""
    rng = np.random.default_rng(seed)
    return {"2": [2] * count, "3": [3] * count, "cycle": [1 + i % ORDER_MAX for i in range(count)],
            "random": [int(x) for x in rng.integers(1, ORDER_MAX + 1, count)]}


def stride_assignments(count):
    """the stride assignments that go with them: uniform 1, 3 and 8, the cycle (1, 2, .. 8, 1, ..)"""
    return {"1": [1] * count, "3": [3] * count, "8": [8] * count, "cycle": [1 + i % SL.STRIDE_MAX for i in range(count)]}


def filter_assignments(count):
    """... and the filters: all delta, the cycle (0, 1, 2, ..)"""
    return {"delta": [SL.ZDELTA] * count, "cycle": [i % 3 for i in range(count)]}


def gen_items(esize, sizes, seed, stride_of=lambda i: 1):
    """items of sizes[i] elements, no tail bytes, the input kinds of oplanes_lib in turn (smooth ones woven at the item's stride)"""
    return [OL.gen(OL.KINDS[i % len(OL.KINDS)], esize, m, 0, seed + i, stride_of(i)) for i, m in enumerate(sizes)]


# ---- the TRCU container ---------------------------------------------------------------------------------------------------
def up16(x):
    return (x + 15) & ~15


def prefix_bytes(count):
    return 16 + 2 * up16(count)


def stored(filters, strides, orders):
    """what the prefix holds: stride 1 for an item without a filter, order 1 for an item whose filter is not ZDELTA"""
    return ([1 if f == SL.NONE else s for f, s in zip(filters, strides)], [k if f == SL.ZDELTA else 1 for f, k in zip(filters, orders)])


def prefix(filters, strides, orders, magic=MAGIC, version=1, zero=0, zero2=0, count=None, stride_pad=0, order_pad=0, raw=False):
    """the container's bytes in front of its TRCB part (np.uint8).  The keyword arguments are the defects of the checker's tests;
    raw: strides and orders are stored as given"""
    cnt = len(filters)
    st, od = (list(strides), list(orders)) if raw else stored(filters, strides, orders)
    pad = up16(cnt) - cnt
    out = struct.pack("<IBBHQ", magic, version, zero, zero2, cnt if count is None else count) + bytes(st) + bytes([stride_pad] * pad) + \
        bytes(od) + bytes([order_pad] * pad)
    assert len(out) == prefix_bytes(cnt)
    return np.frombuffer(out, dtype=np.uint8).copy()


# ---- the estimate table ---------------------------------------------------------------------------------------------------
def table_batch(m=1 << 18):
    """the five u32 items of the table: the sensor series, the timestamps and the sorted ids of oplanes_lib.table_inputs, N(0, 0.02^2)
    fp32 weights, four woven sensor series -> [(name, stride, bytes)]"""
    t = {name: d for name, esize, stride, d in OL.table_inputs(m) if esize == 4}
    rng = np.random.default_rng(77)
    weights = np.ascontiguousarray((0.02 * rng.standard_normal(m)).astype("<f4")).view(np.uint8)
    i = np.arange(m // 4, dtype=np.float64)
    woven = np.stack([(1 << 20) + 2e5 * np.sin(0.002 * i + c) + 5e4 * np.sin(0.02 * i + 2 * c) + rng.normal(0, 3, i.size) for c in range(4)], axis=1).reshape(-1)
    woven = np.ascontiguousarray(np.rint(woven).astype(np.int64).astype("<u4")).view(np.uint8)
    return [("u32 sensor series", 1, t["u32 sensor series"]), ("u32 timestamps", 1, t["u32 timestamps, step 1000 +- 2"]),
            ("sorted u32 ids", 1, t["sorted u32 ids, gaps 1..29"]), ("fp32 weights N(0, 0.02^2)", 1, weights), ("four woven sensor series", 4, woven)]


def chunk_estimate(data, esize, chunk):
    """order-0 estimate in bytes of the planes of `data`, a model per chunk and plane (the coded calls' granularity)"""
    m = data.size // esize
    x = data[:m * esize].reshape(m, esize)
    total = 0.0
    for c0 in range(0, m, chunk):
        blk = x[c0:c0 + chunk]
        for p in range(esize):
            cnt = np.bincount(blk[:, p], minlength=256).astype(np.float64)
            nz = cnt[cnt > 0]
            total += float((nz * np.log2(blk.shape[0] / nz)).sum())
    return total / 8


def estimate_table(m=1 << 18, chunk=4096):
    """-> (rows [(name, stride, bytes under no filter, order 1, 2, 3)], the four totals of the table, the picks per item)"""
    rows = []
    for name, stride, d in table_batch(m):
        rows.append((name, stride) + tuple(chunk_estimate(OL.forward(d, 4, k, chunk, stride), 4, chunk) for k in range(4)))
    none = sum(r[2] for r in rows)
    today = sum(min(r[2], r[3]) for r in rows)
    order2 = sum(r[4] for r in rows)
    best = sum(min(r[2:]) for r in rows)
    picks = [int(np.argmin(r[2:])) for r in rows]
    return rows, (none, today, order2, best), picks


if __name__ == "__main__":
    rows, totals, picks = estimate_table()
    print("| Item | Stride | No filter | Order 1 | Order 2 | Order 3 |\n|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %d | %d | %d |" % (r[0], r[1], round(r[2]), round(r[3]), round(r[4]), round(r[5])))
    print("\n| Choice | Bytes |\n|---|---|")
    for name, v in zip(("No filter", "Best the batch can do today (none or zigzag delta per item)", "Order 2 on every item", "An order per item"), totals):
        print("| %s | %d |" % (name, round(v)))
    print("\nper-item picks (0 = none):", picks)
