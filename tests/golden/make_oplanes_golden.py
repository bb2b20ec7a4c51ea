"""Writes tests/golden/oplanes_vectors.npz: the model of the order-2 / order-3 predictors in front of the byte planes
(tests/oplanes_lib.py), pinned by its per-element restatement.  For every case of oplanes_lib.golden_cases() -- (esize, order,
stride, restart length, elements, tail bytes, input kind) -- the index records the SHA-256 of the input (regenerated from its seed
by oplanes_lib.golden_input, not stored) and of O(input) as scalar_forward, the Python-integer closed form, computes it; O(input)
itself is stored for the cases of at most GOLDEN_STORE_MAX bytes, all in one array `out` (`at` = the first byte of the case,
-1 = hashed only).  The maker asserts that the vectorised model equals the scalar one and that its inverse returns every input.
Data only: nothing here is compiled or run by a test.

    python tests/golden/make_oplanes_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oplanes_lib as L  # noqa: E402


def main():
    index, outs, at = [], [], 0
    for case in L.golden_cases():
        esize, order, stride, seg, m, t, kind = case
        d = L.golden_input(case)
        f = L.scalar_forward(d, esize, order, seg, stride)
        assert f.size == d.size == m * esize + t
        assert np.array_equal(f, L.forward(d, esize, order, seg, stride)), case
        assert np.array_equal(L.inverse(f, esize, order, seg, stride), d), case
        stored = f.size <= L.GOLDEN_STORE_MAX
        index.append({"esize": esize, "order": order, "stride": stride, "seg": seg, "m": m, "t": t, "kind": kind,
                      "in_sha256": L.sha(d), "out_sha256": L.sha(f), "at": at if stored else -1})
        if stored:
            outs.append(f)
            at += f.size
    np.savez_compressed(L.GOLDEN, out=np.concatenate(outs), index=np.frombuffer(json.dumps(index).encode(), dtype=np.uint8))
    print("%d cases, %d bytes stored -> %s (%d bytes)" % (len(index), at, L.GOLDEN, os.path.getsize(L.GOLDEN)))


if __name__ == "__main__":
    main()
