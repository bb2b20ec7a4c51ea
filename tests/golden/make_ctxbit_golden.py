"""Writes tests/golden/ctxbit_vectors.npz and ctxbit_large.json for the bitwise order-1 range coders (rccs / rcxs),
THROUGH THE REFERENCE (oracle/_ref/libtrc_ref.so): every chunk is one call of rccsenc / rcxsenc on that chunk's bytes.
The inputs are not stored: ctxbit_lib.gen(kind, n, seed) regenerates them from the index (seeded, vectorised).

    python tests/golden/make_ctxbit_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ctxbit_lib as L  # noqa: E402

KINDS = ["text", "markov", "runs", "uniform", "const", "binary"]
CHUNKS = [256, 1536, 4096, 16384, 65536]
LARGE = [("markov", 100 * 10**6, 21), ("text", 100 * 10**6, 7)]


def sizes(chunk, kind):
    """n = 1, 63, 64, 65, below the chunk, not a multiple of the chunk.  The large chunks keep the file small: one or two sizes
    per kind there (a full chunk of 65536 by runs and const, a ragged two-chunk case by markov at 16384), and uniform input
    (every chunk raw) at the small chunks only."""
    big = {16384: {"markov": [16384 + 4321], "text": [8192 + 333], "runs": [16384 - 777, 16384 + 4321],
                   "binary": [16384 - 777, 16384 + 4321], "const": [16384 - 777, 16384 + 4321], "uniform": []},
           65536: {"markov": [32768 + 333], "text": [16384 + 333], "runs": [65536 + 333], "binary": [65536 - 777],
                   "const": [65536 - 777, 65536 + 4321], "uniform": []}}
    if chunk in big:
        return big[chunk][kind]
    return [1, 63, 64, 65, chunk - 7, (3 if chunk < 4096 else 1) * chunk + 101]


def cases():
    k = 0
    for chunk in CHUNKS:
        for kind in KINDS:
            for n in sizes(chunk, kind):
                yield k, kind, n, chunk, 1000 + 17 * k
                k += 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    assert L.have_ref(), "needs oracle/_ref/libtrc_ref.so (build() makes it where the reference sources exist)"
    arrays, index = {}, []
    for k, kind, n, chunk, seed in cases():
        d = L.gen(kind, n, seed)
        ent = dict(case=k, kind=kind, n=n, chunk=chunk, seed=seed, in_sha256=sha(d), raw={})
        for codec in (L.RCC1, L.RCX1):
            clen, payload = L.ref_chunked_enc(codec, d, chunk)
            arrays["clen_%d_%s" % (k, L.NAMES[codec])] = clen
            arrays["out_%d_%s" % (k, L.NAMES[codec])] = payload
            lens = [min(chunk, n - i) for i in range(0, n, chunk)]
            ent["raw"][L.NAMES[codec]] = int(sum(int(c) == l for c, l in zip(clen, lens)))
        index.append(ent)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "ctxbit_vectors.npz"), **arrays)
    large = []
    for kind, n, seed in LARGE:
        d = L.gen(kind, n, seed)
        for codec in (L.RCC1, L.RCX1):
            clen, payload = L.ref_chunked_enc(codec, d, L.ROUND_CHUNK)
            large.append(dict(codec=L.NAMES[codec], kind=kind, n=n, seed=seed, chunk=L.ROUND_CHUNK, payload_bytes=int(payload.size),
                              clen_sha256=sha(clen.astype("<u4")), payload_sha256=sha(payload)))
            print(large[-1])
    with open(os.path.join(HERE, "ctxbit_large.json"), "w") as f:
        json.dump(large, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
