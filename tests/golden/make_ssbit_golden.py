"""Writes tests/golden/ssbit_vectors.npz and ssbit_large.json for the byte-level bitwise coders on the dual-rate "ss" predictor
(rcss, rc4ss, rc4css, rcu3ss), THROUGH THE REFERENCE: every chunk is one call of the reference encoder on that chunk's bytes
with the case's two parameters.  The reference's two sources are compiled where they lie into a temporary directory
(ssbit_lib.Ref); nothing compiled is kept.  The inputs are not stored: ssbit_lib.gen(kind, n, seed, chunk) regenerates them
from the index, pinned by SHA-256.  All directories lie in one array `clen` and all payloads in one array `out` (a zip member
per case would cost more than the cases hold): the index entry's `at[coder][prm0_prm1]` = [first directory entry, first payload
byte, payload bytes] (ssbit_lib.fixture reads one back).

    python tests/golden/make_ssbit_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "turbo-range-coder_amd"))
import ssbit_lib as L  # noqa: E402

CHUNKS = [256, 1024, 4096, 65536]
SMALL = [1, 2, 3, 8, 9, 10, 63, 64, 65, 255, 256, 257]       # 9 and below: always raw; around a wave's 64 lanes' worth of bytes; around the smallest chunk
PRM_KINDS = ("mixed", "nib_skew")                              # the chunk-256 cases of these kinds run with every pair of L.PRMS
LARGE_N, LARGE_CHUNK, LARGE_KIND, LARGE_SEED = 4 << 20, 1024, "mixed", 77


def sizes(chunk, kind):
    """chunk 256: every small length, chunk + 9, 3 chunks + 10, and for two kinds each 64 chunks + 1 (a second directory group of
    one raw byte) and 65 chunks; chunks 1024 and 4096: one length over whole chunks; 65536: the same for the two cheapest kinds"""
    if chunk == 256:
        s = SMALL + [chunk + 9, 3 * chunk + 10]
        if kind in ("nib_skew", "bytes_small"):
            s.append(64 * chunk + 1)
        if kind in ("zeros", "bytes_small"):
            s.append(65 * chunk)
        return s
    if chunk == 1024:
        return [2 * chunk + 10]
    if chunk == 4096:
        return [chunk + 10]
    return [chunk + 10] if kind in ("nib_skew", "zeros") else []


def cases():
    k = 0
    for chunk in CHUNKS:
        for kind in L.KINDS:
            for n in sizes(chunk, kind):
                prms = L.PRMS if chunk == 256 and kind in PRM_KINDS else [L.DEFAULT]
                yield k, kind, n, chunk, 2000 + 13 * k, prms
                k += 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def chunk_lens(n, chunk):
    return np.minimum(chunk, n - np.arange(0, n, chunk))


def main():
    assert L.have_ref_sources(), "needs the reference sources (rc_ss.c, rc_s.c and what they include)"
    tmp = tempfile.TemporaryDirectory()
    R = L.Ref(tmp.name)
    clens, outs, index = [], [], []
    nclen = nout = 0
    raw = {c: 0 for c in L.CODECS}
    coded = {c: 0 for c in L.CODECS}
    differs = 0
    for k, kind, n, chunk, seed, prms in cases():
        d = L.gen(kind, n, seed, chunk)
        ent = dict(case=k, kind=kind, n=n, chunk=chunk, seed=seed, in_sha256=sha(d), prms=[list(p) for p in prms],
                   at={L.NAMES[c]: {} for c in L.CODECS})
        lens = chunk_lens(n, chunk)
        for codec in L.CODECS:
            name = L.NAMES[codec]
            default_payload = None
            for prm in prms:
                clen, payload = R.chunked_enc(codec, d, chunk, prm)
                ent["at"][name][L.prm_tag(prm)] = [nclen, nout, int(payload.size)]
                clens.append(clen); outs.append(payload)
                nclen += clen.size; nout += payload.size
                if tuple(prm) == L.DEFAULT:
                    default_payload = payload
                israw = clen == lens
                raw[codec] += int(israw.sum())
                coded[codec] += int((~israw).sum())
                # what holds for the reference alone
                assert israw[lens <= 9].all(), (name, kind, n, prm)
                full = (~israw) & np.isin(lens, (256, 1024, 4096, 65536))
                if codec == L.RC4CSS:
                    assert (clen[full] == lens[full] // 2 + 4).all(), (kind, n, chunk, prm)
                if tuple(prm) == (4, 7):
                    differs += not np.array_equal(payload, default_payload)
                # and the reference decodes every coded chunk back
                want, off = L.expected(codec, d, clen, chunk), 0
                for i, l in enumerate(clen):
                    piece = want[i * chunk:(i + 1) * chunk]
                    if l != piece.size:
                        assert np.array_equal(R.dec(codec, payload[off:off + l], piece.size, prm), piece), (name, kind, n, prm, i)
                    off += int(l)
        index.append(ent)
    for c in L.CODECS:
        assert raw[c] >= 1 and coded[c] >= 40, (L.NAMES[c], raw[c], coded[c])
    assert differs >= 1
    out = os.path.join(HERE, "ssbit_vectors.npz")
    np.savez_compressed(out, clen=np.concatenate(clens).astype(np.uint32), out=np.concatenate(outs),
                        index=np.frombuffer(json.dumps(index).encode(), dtype=np.uint8))
    assert os.path.getsize(out) < 512 * 1024, os.path.getsize(out)
    print("%d cases, %d bytes; raw / coded chunks: %s; (4,7) payloads that differ from (5,6): %d"
          % (len(index), os.path.getsize(out), {L.NAMES[c]: (raw[c], coded[c]) for c in L.CODECS}, differs))
    large = []
    d = L.gen(LARGE_KIND, LARGE_N, LARGE_SEED, LARGE_CHUNK)
    for codec in L.CODECS:
        clen, payload = R.chunked_enc(codec, d, LARGE_CHUNK, L.DEFAULT)
        large.append(dict(codec=L.NAMES[codec], kind=LARGE_KIND, n=LARGE_N, seed=LARGE_SEED, chunk=LARGE_CHUNK, prm=list(L.DEFAULT),
                          in_sha256=sha(d), payload_bytes=int(payload.size), raw_chunks=int((clen == LARGE_CHUNK).sum()),
                          clen_sha256=sha(clen.astype("<u4")), payload_sha256=sha(payload)))
        print(large[-1]["codec"], LARGE_KIND, large[-1]["payload_bytes"], large[-1]["raw_chunks"])
    with open(os.path.join(HERE, "ssbit_large.json"), "w") as f:
        json.dump(large, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
