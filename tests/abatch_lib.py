"""The batch advisor: the numpy model of trc_planes_hist_batch_dev and trc_planes_advise_batch.  Both are the planes advisor's
model (advise_lib) item by item: slice i = advise_lib.hist(item i, esize, chunk, filters) -- the item alone, the predictor restarted
every chunk elements, no pad anywhere -- and entry i = advise_lib.advise of that slice with m = the item's elements."""
import numpy as np

import advise_lib as AL

LENGTHS = (1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097, 65539)       # elements per item
CHUNKS = (256, 320)
KINDS = ("random", "wrap")


def gen_items(esize, lengths, seed, kinds=KINDS):
    """items of whole elements (no tail), their kinds taking turns"""
    return [AL.gen(kinds[i % len(kinds)], esize, m, 0, seed + 7 * i) for i, m in enumerate(lengths)]


def hist(items, esize, chunk, filters):
    """-> uint64 [count, 3, esize, 256]"""
    return np.stack([AL.hist(d, esize, chunk, filters) for d in items])


def masked(h, filters):
    """the model of all three filters -> the model of the bit set `filters`: rows not requested are zero"""
    out = h.copy()
    for f in range(3):
        if not filters >> f & 1:
            out[:, f] = 0
    return out


def advise(h, filters, esize, ms):
    """-> [(choice, bits [3, 8], total_bits [3])] per item"""
    return [AL.advise(h[i], filters, esize, m) for i, m in enumerate(ms)]


def assert_advice(got_filters, got_advice, want, filters, esize, ms, tag=""):
    """the library's (filters, advice dicts) against advise(): the choice exact, the estimates to rtol 1e-9 (256 double terms per
    plane, each within an ulp or two of numpy's)"""
    assert got_filters == [w[0] for w in want], tag + ": choices %s, the model has %s" % (got_filters, [w[0] for w in want])
    if got_advice is None:
        return
    for i, (a, (choice, bits, total)) in enumerate(zip(got_advice, want)):
        assert (a["filter"], a["esize"], a["filters"], a["m"]) == (choice, esize, filters, ms[i]), tag + ": item %d" % i
        assert np.allclose(a["bits"], bits, rtol=1e-9, atol=0) and np.allclose(a["total_bits"], total, rtol=1e-9, atol=0), tag + ": item %d" % i
