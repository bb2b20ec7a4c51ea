"""Writes tests/golden/planes_vectors.npz: the output of the reference's byte transpose tpenc (transpose_.c:110-123) for seeded
random inputs of 2- / 4- / 8-byte elements at the lengths 32 * esize * j + r, j in {1, 8, 64}, r in {0, esize - 1} -- the
lengths with n % (32 * esize) < esize, where tpenc writes the plain layout (plane k = byte k of every element, then the tail)
whatever ISA it was built for.  The reference's transpose is compiled where it lies into a temporary directory (planes_lib.Ref);
nothing compiled is kept.  The inputs are not stored: planes_lib.golden_input(esize, n) regenerates them.  All outputs lie in
one array `out`; the index entry's `at` is the first byte of its case.  The maker asserts that every output equals the numpy
split and that tpdec returns the input.

    python tests/golden/make_planes_golden.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import planes_lib as L  # noqa: E402


def main():
    assert L.have_ref_sources(), "the reference's transpose sources are needed (TRC_REFERENCE)"
    with tempfile.TemporaryDirectory() as tmp:
        ref = L.Ref(tmp)
        index, outs, at = [], [], 0
        for esize in L.ESIZES:
            for n in L.golden_lengths(esize):
                d = L.golden_input(esize, n)
                o = ref.tpenc(d, esize)
                assert o.size == n <= 65536
                assert np.array_equal(o, L.flat(d, esize)), "tpenc differs from the plain layout at esize %d, n %d" % (esize, n)
                assert np.array_equal(ref.tpdec(o, esize), d), "tpdec does not return the input at esize %d, n %d" % (esize, n)
                index.append({"esize": esize, "n": n, "at": at})
                outs.append(o)
                at += n
    np.savez_compressed(L.GOLDEN, out=np.concatenate(outs), index=np.frombuffer(json.dumps(index).encode(), dtype=np.uint8))
    print("%d cases, %d bytes -> %s (%d bytes)" % (len(index), at, L.GOLDEN, os.path.getsize(L.GOLDEN)))


if __name__ == "__main__":
    main()
