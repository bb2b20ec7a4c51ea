"""Writes tests/golden/nibbit_vectors.npz and nibbit_large.json for the bitwise nibble and varint byte coders (rc4s, rc4cs,
rcu3s), THROUGH THE REFERENCE (oracle/_ref/libtrc_ref.so): every chunk is one call of the reference encoder on that chunk's
bytes.  The inputs are not stored: nibbit_lib.gen(kind, n, seed, chunk) regenerates them from the index, pinned by SHA-256.

    python tests/golden/make_nibbit_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nibbit_lib as L  # noqa: E402

CHUNKS = [256, 1024, 4096, 65536]
SMALL = [1, 2, 3, 8, 9, 10, 63, 64, 65, 255, 256, 257]       # 9 and below: always raw; around a wave's 64 lanes' worth of bytes; around the smallest chunk
LARGE_N, LARGE_CHUNK, LARGE_KIND, LARGE_SEED = 4 << 20, 1024, "mixed", 77


def sizes(chunk, kind):
    """every small length at every chunk (at the larger chunks, where they are one short chunk, for three kinds); at chunk 256
    chunk + 9, 3 chunks + 10, 64 chunks + 1 (a second directory group of one raw byte) and 65 chunks; at the larger chunks one
    length over whole chunks (at 65536 for the two cheapest kinds only)"""
    s = list(SMALL) if chunk == 256 or kind in ("nib_skew", "bytes_uniform", "bytes_small") else []
    if chunk == 256:
        s += [chunk + 9, 3 * chunk + 10]
        if kind in ("mixed", "nib_skew"):
            s.append(64 * chunk + 1)
        if kind in ("mixed", "zeros"):
            s.append(65 * chunk)
    elif chunk == 1024:
        s.append(2 * chunk + 10)
    elif chunk == 4096:
        s.append(chunk + 10)
    elif kind in ("nib_skew", "zeros"):
        s.append(chunk + 10)
    return s


def cases():
    k = 0
    for chunk in CHUNKS:
        for kind in L.KINDS:
            for n in sizes(chunk, kind):
                yield k, kind, n, chunk, 1000 + 17 * k
                k += 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def chunk_lens(n, chunk):
    return np.minimum(chunk, n - np.arange(0, n, chunk))


def main():
    assert L.have_ref(), "needs oracle/_ref/libtrc_ref.so (build() makes it where the reference sources exist)"
    arrays, index = {}, []
    raw = {c: 0 for c in L.CODECS}
    coded = {c: 0 for c in L.CODECS}
    mid_raw = 0
    for k, kind, n, chunk, seed in cases():
        d = L.gen(kind, n, seed, chunk)
        ent = dict(case=k, kind=kind, n=n, chunk=chunk, seed=seed, in_sha256={}, raw={})
        lens = chunk_lens(n, chunk)
        for codec in L.CODECS:
            name = L.NAMES[codec]
            ent["in_sha256"][name] = sha(d)
            clen, payload = L.ref_chunked_enc(codec, d, chunk)
            arrays["clen_%d_%s" % (k, name)] = clen
            arrays["out_%d_%s" % (k, name)] = payload
            israw = clen == lens
            ent["raw"][name] = int(israw.sum())
            raw[codec] += int(israw.sum())
            coded[codec] += int((~israw).sum())
            # what holds for the reference alone
            assert israw[lens <= 9].all(), (name, kind, n)
            full = (~israw) & np.isin(lens, (256, 1024, 4096))
            if codec == L.RC4C:
                assert (clen[full] == lens[full] // 2 + 4).all(), (kind, n, chunk)
            if kind == "zeros" and chunk in (256, 1024):
                assert (clen[lens == chunk] == {L.RC4: 16, L.RC4C: chunk // 2 + 4, L.RCU3: 4}[codec]).all(), (name, n, chunk)
            if codec == L.RCU3 and kind == "bytes_uniform":
                assert israw.all(), (n, chunk)
                mid_raw += int((lens >= 64).sum())
        index.append(ent)
    for c in L.CODECS:
        assert raw[c] >= 1 and coded[c] >= 40, (L.NAMES[c], raw[c], coded[c])
    assert mid_raw >= 10, mid_raw
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "nibbit_vectors.npz")
    np.savez_compressed(out, **arrays)
    assert os.path.getsize(out) < 512 * 1024, os.path.getsize(out)
    print("%d cases, %d bytes; raw / coded chunks: %s" % (len(index), os.path.getsize(out),
                                                          {L.NAMES[c]: (raw[c], coded[c]) for c in L.CODECS}))
    large = []
    d = L.gen(LARGE_KIND, LARGE_N, LARGE_SEED, LARGE_CHUNK)
    for codec in L.CODECS:
        clen, payload = L.ref_chunked_enc(codec, d, LARGE_CHUNK)
        large.append(dict(codec=L.NAMES[codec], kind=LARGE_KIND, n=LARGE_N, seed=LARGE_SEED, chunk=LARGE_CHUNK, in_sha256=sha(d),
                          payload_bytes=int(payload.size), raw_chunks=int((clen == LARGE_CHUNK).sum()),
                          clen_sha256=sha(clen.astype("<u4")), payload_sha256=sha(payload)))
        print(large[-1]["codec"], LARGE_KIND, large[-1]["payload_bytes"], large[-1]["raw_chunks"])
    with open(os.path.join(HERE, "nibbit_large.json"), "w") as f:
        json.dump(large, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
