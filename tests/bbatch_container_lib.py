"""The TRCE container of a batch coded against a base per item (include/trc_hip.h): the numpy definition of its prefix, on top of
planes_container_lib (the TRCB container behind it, unchanged) and bplanes_lib (the filters against a base, the fingerprint).

    trc_planes_bbatch_hdr (16 B: magic "TRCE", version 1, zero, zero2, uint64 count)
    | uint64 base_fp[count], zero-padded so that the prefix is a multiple of 16
    | the TRCB container of (items, filters) whose inner TRCP container is that of V([G(0) .. G(count - 1)])

base_fp[i] = fingerprint(bases[i][:n[i]]) where filters[i] is not NONE, else 0."""
import struct

import numpy as np

import bplanes_lib as BP
import planes_container_lib as CL

MAGIC = 0x45435254                                             # "TRCE"
HDR = 16


def prefix_bytes(count):
    return HDR + ((8 * count + 15) & ~15)


def fingerprints(bases, filters, sizes):
    """base_fp of the batch: the fingerprint of the first n[i] bytes of bases[i], 0 where the item has no filter"""
    return [0 if f == BP.NONE else BP.fingerprint(np.ascontiguousarray(b, dtype=np.uint8)[:n]) for b, f, n in zip(bases, filters, sizes)]


def prefix(fps, magic=MAGIC, version=1, zero=0, zero2=0, count=None, pad=0):
    """the container's prefix (np.uint8) in front of the TRCB part.  The keyword arguments are the defects of the checker's tests;
    pad: the value of the padding bytes"""
    cnt = len(fps)
    out = struct.pack("<IBBHQ", magic, version, zero, zero2, cnt if count is None else count) + struct.pack("<%dQ" % cnt, *fps)
    out += bytes([pad] * (prefix_bytes(cnt) - len(out)))
    return np.frombuffer(out, dtype=np.uint8).copy()


def expected(items, bases, filters, esize, chunk, inner_container):
    """the whole container, given the TRCP container of the virtual buffer of the items filtered against their bases"""
    sizes = [int(np.asarray(d).size) for d in items]
    return np.concatenate([prefix(fingerprints(bases, filters, sizes)), CL.expected(items, filters, esize, chunk, inner_container)])


# ---- the advisor against bases: the batches of the "auto" tests ------------------------------------------------------------------
AUTO_ELEMS = [1000, 256, 3000, 77, 513, 4097]                   # elements per item


def auto_batch(which, esize):
    """-> (items, bases) for the advisor: "pairs": "drift" and "same" pairs in turn, whose deltas are far shorter than the items, with
    item 3 left without a base (None); "random": unrelated uniform words, where no filter wins by the 1/64 rule"""
    kinds = ("drift", "same") if which == "pairs" else ("random",)
    pairs = [BP.gen_pair(kinds[i % len(kinds)], esize, m, 0, 600 + 10 * esize + i) for i, m in enumerate(AUTO_ELEMS)]
    items, bases = [p[0] for p in pairs], [p[1] for p in pairs]
    if which == "pairs":
        bases[3] = None
    return items, bases


def advise(items, bases, esize, filters=7):
    """the model of trc_planes_advise_bbatch: advise_lib.advise on bplanes_lib.hist per item under filters & (7 if it has a base else 1)
    -> (choices, histograms uint64 [count, 3, esize, 256])"""
    import advise_lib as AL
    choice, hists = [], []
    for d, b in zip(items, bases):
        f = filters & (7 if b is not None else 1)
        h = BP.hist(d, b if b is not None else d, esize, f)
        hists.append(h)
        choice.append(AL.advise(h, f, esize, d.size // esize)[0])
    return choice, np.stack(hists)
