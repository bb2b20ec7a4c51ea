"""Writes tests/golden/word_vectors.npz and word_large.json for the bitwise word coders (rcsenc16, rcsenc32, rccsenc32,
rcc2senc32), THROUGH THE REFERENCE (oracle/_ref/libtrc_ref.so): every chunk is one call of the reference encoder on that
chunk's bytes, with guard bytes around `out` (word_lib.ref_enc).  The npz holds the reference's own outputs; the inputs are
not stored: word_lib.gen(kind, es, n, seed) regenerates them from the index, pinned by SHA-256.  word_large.json holds the
hashes of what the library stores (word_lib.expected: a chunk the reference codes to more than its length is raw).

    python tests/golden/make_word_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import word_lib as L  # noqa: E402

CHUNKS = [256, 1024, 4096, 16384]
LARGE_N, LARGE_CHUNK = 100 * 10**6, 16384


def sizes(chunk, kind):
    """n = 1, 2, 3, 5 (below and about one word), 63, 64, 65, below the chunk, ragged tails over several chunks"""
    if chunk == 256:
        return [1, 2, 3, 5, 63, 64, 65, 249, 513, 514, 515]
    if chunk == 1024:
        return [1, 3, 1017, 3075] if kind not in ("allmax", "const") else [3075]
    if kind in ("allmax", "const"):
        return []
    if chunk == 4096:
        return [8195]
    return [16384 + 4321] if kind in ("walk", "sine", "stamps") else [16384 - 777] if kind == "geo" else [16384 + 2]


def large_kind(codec):
    return "stamps" if codec == L.RCC2W32 else "walk"


def cases():
    k = 0
    for chunk in CHUNKS:
        for kind in L.KINDS:
            for n in sizes(chunk, kind):
                yield k, kind, n, chunk, 3000 + 17 * k
                k += 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def large_entry(codec, kind, n, chunk, seed):
    d = L.gen(kind, L.ES[codec], n, seed)
    clen, payload = L.ref_chunked_enc(codec, d, chunk)
    clen, payload, raised = L.expected(codec, d, chunk, clen, payload)
    return dict(codec=L.NAMES[codec], kind=kind, n=n, seed=seed, chunk=chunk, nchunks=int(clen.size), in_sha256=sha(d),
                raised=raised, payload_bytes=int(payload.size), clen_sha256=sha(clen.astype("<u4")), payload_sha256=sha(payload))


def main():
    assert L.have_ref(), "needs oracle/_ref/libtrc_ref.so (build() makes it where the reference sources exist)"
    arrays, index = {}, []
    for k, kind, n, chunk, seed in cases():
        ent = dict(case=k, kind=kind, n=n, chunk=chunk, seed=seed, in_sha256={}, raw={}, raised={})
        for codec in L.CODECS:
            name = L.NAMES[codec]
            d = L.gen(kind, L.ES[codec], n, seed)
            ent["in_sha256"][name] = sha(d)
            clen, payload = L.ref_chunked_enc(codec, d, chunk)
            arrays["clen_%d_%s" % (k, name)] = clen
            arrays["out_%d_%s" % (k, name)] = payload
            lens = [min(chunk, n - i) for i in range(0, n, chunk)]
            ent["raw"][name] = int(sum(int(c) == l for c, l in zip(clen, lens)))
            ent["raised"][name] = int(sum(int(c) > l for c, l in zip(clen, lens)))
        index.append(ent)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "word_vectors.npz"), **arrays)
    large = []
    for codec in L.CODECS:
        large.append(large_entry(codec, large_kind(codec), LARGE_N, LARGE_CHUNK, 77))
        print(large[-1]["codec"], large[-1]["kind"], large[-1]["payload_bytes"], large[-1]["raised"])
    # slots + 1 chunks of rcc2s32: the last round holds one chunk
    s = L.slots(L.RCC2W32, 1 << 40)
    large.append(large_entry(L.RCC2W32, "walk", s * LARGE_CHUNK + 5000, LARGE_CHUNK, 78))
    large[-1]["case"] = "slots+1"
    print("slots+1", s, large[-1]["payload_bytes"])
    with open(os.path.join(HERE, "word_large.json"), "w") as f:
        json.dump(large, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
