"""Batched byte planes: the numpy definition of the virtual buffer V(items, esize, chunk) and of its plan (include/trc_hip.h),
and the packer of the GPU tests, which lays the items of a batch into ONE allocation with nothing but 16 to 48 bytes of 0xA5
between them -- no readable slack of their own, and every gap checkable after a join."""
import numpy as np

GAP = 0xA5
GUARD = 512


def up256(x):
    return (x + 255) & ~255


def plan(sizes, esize, chunk):
    """sizes: bytes per item -> (dict of the fields of trc_planes_batch_plan, first_chunk: list of len(sizes) + 1)"""
    m = [n // esize for n in sizes]
    nc = [(x + chunk - 1) // chunk for x in m]
    first = [0]
    for c in nc:
        first.append(first[-1] + c)
    m_total = (first[-1] - nc[-1]) * chunk + m[-1]
    return {"m_total": m_total, "n_virtual": m_total * esize, "chunks": first[-1],
            "pitch": up256(m_total + 256), "pad_elems": m_total - sum(m)}, first


def virtual(items, esize, chunk):
    """items: uint8 arrays of whole elements -> V: every item but the last followed by zero elements up to a whole chunk"""
    parts = []
    for i, d in enumerate(items):
        d = np.ascontiguousarray(d, dtype=np.uint8)
        assert d.size >= esize and d.size % esize == 0
        parts.append(d)
        if i + 1 < len(items):
            parts.append(np.zeros((-(d.size // esize) % chunk) * esize, dtype=np.uint8))
    return np.concatenate(parts)


def offsets(sizes, seed=0):
    """16-byte aligned offsets of the items in one allocation, 16 to 48 bytes between an item's end and the next one's start
    -> (offsets, bytes of the allocation without its guard)"""
    rng = np.random.default_rng(seed)
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos = ((pos + n + 15) & ~15) + 16 * int(rng.integers(1, 3))
    return offs, pos


def image(items, offs, total):
    """the allocation as the host sees it: 0xA5 throughout (gaps, the 512-byte guard), the items (None: left 0xA5) at their offsets"""
    a = np.full(total + GUARD, GAP, dtype=np.uint8)
    for d, o in zip(items, offs):
        if d is not None:
            a[o:o + d.size] = d
    return a


def views(d_buf, offs, sizes, only=None):
    """the items as uint8 views of the device allocation; None outside `only` (a range of item indices)"""
    return [d_buf[o:o + n] if only is None or i in only else None for i, (o, n) in enumerate(zip(offs, sizes))]
