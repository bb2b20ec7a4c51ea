"""Writes tests/golden/bvlc_vectors.npz and bvlc_large.json for the Turbo-VLC coders on the bitwise range coder (rcvs*,
rcvzs*, rcvgs*, rcvgzs* at 16 / 32 bits), THROUGH THE REFERENCE (oracle/_ref/libtrc_ref.so): every chunk is one call of the
reference encoder on that chunk's bytes, with writable guard bytes in front of `out` (bvlc_lib.ref_enc).  The inputs are not
stored: bvlc_lib.gen(kind, es, n, seed) regenerates them from the index, pinned by SHA-256.

    python tests/golden/make_bvlc_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bvlc_lib as L  # noqa: E402

CHUNKS = [256, 1024, 4096, 16384]
LARGE_N, LARGE_CHUNK = 100 * 10**6, 16384


def sizes(chunk, kind):
    """n = 1, 2, 3 (below one element), 63, 64, 65, below the chunk, ragged tails over several chunks; the constant inputs
    and uniform (every chunk raw) at the small chunks only"""
    if kind in L.CONSTS:
        return [1, 2, 3, 63, 64, 65, 515] if chunk == 256 else [3075] if chunk == 1024 else []
    if chunk == 256:
        return [1, 2, 3, 63, 64, 65, 249, 513, 514, 515]
    if chunk == 1024:
        return [1, 3, 1017, 2049, 3075]
    if kind == "uniform":
        return []
    if chunk == 4096:
        return [8195]
    return [16384 + 4321] if kind in ("geo", "walk", "mixed") else [16384 - 777]


def large_kind(codec):
    return "walk" if L.NAMES[codec].startswith(("rcvzs", "rcvgzs")) else "mixed"


def cases():
    k = 0
    for chunk in CHUNKS:
        for kind in L.KINDS:
            for n in sizes(chunk, kind):
                yield k, kind, n, chunk, 2000 + 13 * k
                k += 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    assert L.have_ref(), "needs oracle/_ref/libtrc_ref.so (build() makes it where the reference sources exist)"
    arrays, index = {}, []
    for k, kind, n, chunk, seed in cases():
        ent = dict(case=k, kind=kind, n=n, chunk=chunk, seed=seed, in_sha256={}, raw={})
        for codec in L.CODECS:
            name = L.NAMES[codec]
            d = L.gen(kind, L.ES[codec], n, seed)
            ent["in_sha256"][name] = sha(d)
            clen, payload = L.ref_chunked_enc(codec, d, chunk)
            arrays["clen_%d_%s" % (k, name)] = clen
            arrays["out_%d_%s" % (k, name)] = payload
            lens = [min(chunk, n - i) for i in range(0, n, chunk)]
            ent["raw"][name] = int(sum(int(c) == l for c, l in zip(clen, lens)))
        index.append(ent)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "bvlc_vectors.npz"), **arrays)
    large = []
    for codec in L.CODECS:
        kind, seed = large_kind(codec), 77
        d = L.gen(kind, L.ES[codec], LARGE_N, seed)
        clen, payload = L.ref_chunked_enc(codec, d, LARGE_CHUNK)
        large.append(dict(codec=L.NAMES[codec], kind=kind, n=LARGE_N, seed=seed, chunk=LARGE_CHUNK, in_sha256=sha(d),
                          payload_bytes=int(payload.size), clen_sha256=sha(clen.astype("<u4")), payload_sha256=sha(payload)))
        print(large[-1]["codec"], kind, large[-1]["payload_bytes"])
    with open(os.path.join(HERE, "bvlc_large.json"), "w") as f:
        json.dump(large, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
