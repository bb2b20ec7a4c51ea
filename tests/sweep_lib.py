"""Inputs, case lists and reference calls of tests/golden/sweep.json and sweep_sha256.npy: the 26 coders outside trc.AVAILABLE
(CTXBIT 28-29, INTBIT 30-41, BVLC 43-50, WORD 52-55) on many-wave shapes, at the raw / coded threshold and in used workspaces.

Every case is a small dict from which build_input(codec, case) regenerates the bytes (seeded with PCG64 like the family gens):
  sweep  {kind, n, chunk, seed, splice: None | [offset, length, "uniform" | "const"]}
  wave   {pattern, nchunks, last, chunk, seed}: `nchunks - 1` full chunks and a last one of `last` bytes; pattern
           alt      uniform bytes (raw) in the even chunks, HEAD[family] (coded) in the odd ones
           midwave  one whole wave raw: chunks 64..127 where there are more than 128, chunks 0..63 otherwise
           edges    lanes 0 and 63 of every wave raw
           hard0/1  HARD[family][0/1] (allmax, const, ...) over the whole input
  ramp   {chunk, segs: [[count, lo, hi], ...], seed}: per chunk a HEAD head and a uniform tail whose length goes from lo to hi
           bytes over the segment's chunks (a coarse segment over the upper half, a fine one around the crossover)
  late   {chunk, pairs: [[t, nsur], ...], seed}: pairs of chunks; the first is t uniform bytes, then a constant stretch, then
           nsur elements of the costliest kind (SURPRISE), coded to just below the raw limit; the second an ordinary HEAD chunk
"""
import json
import os

import numpy as np

import bvlc_lib as BL
import ctxbit_lib as CL
import intbit_lib as IL
import word_lib as WL

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep.json")
GOLD_SHA = os.path.join(os.path.dirname(GOLD), "sweep_sha256.npy")
LIBS = {"ctxbit": CL, "intbit": IL, "bvlc": BL, "word": WL}
FAMILY = {c: f for f, cs in (("ctxbit", (CL.RCC1, CL.RCX1)), ("intbit", IL.CODECS), ("bvlc", BL.CODECS), ("word", WL.CODECS)) for c in cs}
CODECS = sorted(FAMILY)
NAMES = {c: LIBS[FAMILY[c]].NAMES[c] for c in CODECS}
ES = {c: 1 if FAMILY[c] == "ctxbit" else LIBS[FAMILY[c]].ES[c] for c in CODECS}
KINDS = {"ctxbit": ["text", "markov", "runs", "uniform", "const", "binary"], "intbit": IL.KINDS, "bvlc": BL.KINDS, "word": WL.KINDS}
HEAD = {"ctxbit": "runs", "intbit": "geo", "bvlc": "geo", "word": "geo"}     # coded by every coder of the family at chunk 256
HARD = {"ctxbit": ["binary", "const"], "intbit": ["allmax", "const"], "bvlc": ["allmax", "max7"], "word": ["allmax", "const"]}
ZIGZAG = {c for c in CODECS if NAMES[c].startswith(("rcgzs", "rcrzs", "rcvzs", "rcvgzs"))}
SWEEP_CHUNKS = [256, 320, 512, 1024, 1984, 2560, 4096, 16384, 65536]
WAVE_NCHUNKS = [63, 64, 65, 127, 128, 129, 64 * 7 + 1]
WAVE_PATTERNS = ["alt", "midwave", "edges", "hard0", "hard1"]
RAMP_CHUNKS = [256, 1024, 4096, 16384]
NEAR = 16                                                      # "near the limit": coded to within this many bytes of it
VOLUME_CAP = 2 * 10**9
WORK_CAP = 16 << 30


def gen(codec, kind, n, seed):
    fam = FAMILY[codec]
    return CL.gen(kind, n, seed) if fam == "ctxbit" else LIBS[fam].gen(kind, ES[codec], n, seed)


def uniform(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, n, dtype=np.uint8)


def chunk_lens(n, chunk):
    return np.minimum(chunk, n - np.arange(0, n, chunk)).astype(np.int64)


def case_n(case):
    f = case["fam"]
    if f == "sweep":
        return case["n"]
    if f == "wave":
        return (case["nchunks"] - 1) * case["chunk"] + case["last"]
    if f == "ramp":
        return sum(s[0] for s in case["segs"]) * case["chunk"]
    return 2 * len(case["pairs"]) * case["chunk"] - 37           # late: the last neighbour is ragged


def wave_mask(pattern, nchunks):
    """which chunks are uniform bytes (raw)"""
    c = np.arange(nchunks)
    if pattern == "alt":
        return c % 2 == 0
    if pattern == "midwave":
        return (c // 64 == 1) if nchunks > 128 else (c // 64 == 0)
    if pattern == "edges":
        return (c % 64 == 0) | (c % 64 == 63)
    raise ValueError(pattern)


def ramp_tails(case):
    """uniform tail bytes of every chunk of a ramp"""
    out = []
    for cnt, lo, hi in case["segs"]:
        out += [(lo * (cnt - 1 - i) + hi * i) // max(cnt - 1, 1) for i in range(cnt)]
    return np.array(out, dtype=np.int64)


def surprise(codec, nsur):
    """the costliest elements after a stretch of 5s, as bytes: the all-ones element (a context rcrs32 has not seen), then one
    with another top byte; for the zigzag coders a maximal delta each time"""
    es = ES[codec]
    top, half = (1 << (8 * es)) - 1, 1 << (8 * es - 1)
    vals = [5 + half, 5, 5 + half] if codec in ZIGZAG else [top, top ^ (0x55 << (8 * es - 8)), top >> 1]
    return np.array(vals[:nsur], dtype=np.uint64).astype({1: "<u1", 2: "<u2", 4: "<u4"}[es]).view(np.uint8)


def late_chunk(codec, chunk, t, nsur, seed):
    es = ES[codec]
    sur = surprise(codec, nsur)
    d = np.empty(chunk, dtype=np.uint8)
    d[:t] = uniform(t, seed)
    fill = np.zeros(chunk - t + es, dtype=np.uint8)
    fill[(-t) % es::es] = 5                                     # elements of value 5, aligned to the chunk's element grid
    d[t:] = fill[:chunk - t]
    d[chunk - sur.size:] = sur
    return d


def build_input(codec, case):
    f, seed = case["fam"], case["seed"]
    fam = FAMILY[codec]
    n = case_n(case)
    if f == "sweep":
        d = gen(codec, case["kind"], n, seed)
        if case["splice"]:
            off, ln, what = case["splice"]
            d[off:off + ln] = uniform(ln, seed + 1) if what == "uniform" else 0x41
        return d
    chunk = case["chunk"]
    if f == "wave":
        if case["pattern"].startswith("hard"):
            return gen(codec, HARD[fam][int(case["pattern"][4])], n, seed)
        d = gen(codec, HEAD[fam], n, seed)
        m = np.repeat(wave_mask(case["pattern"], case["nchunks"]), chunk)[:n]
        d[m] = uniform(n, seed + 1)[m]
        return d
    if f == "ramp":
        d = gen(codec, HEAD[fam], n, seed)
        pos = np.arange(n) % chunk
        m = pos >= chunk - np.repeat(ramp_tails(case), chunk)
        d[m] = uniform(n, seed + 1)[m]
        return d
    if f == "late":
        d = gen(codec, HEAD[fam], n + 37, seed)
        for j, (t, nsur) in enumerate(case["pairs"]):
            d[2 * j * chunk:(2 * j + 1) * chunk] = late_chunk(codec, chunk, t, nsur, seed + 1 + j)
        return d[:n]
    raise ValueError(f)


def ref_lengths(codec, d, chunk):
    """-> (reference clen as returned, stored clen, stored payload): one reference call per chunk and the family's own rule for
    what the library stores (intbit: a chunk below one element raw; word: a chunk the reference codes to >= its length raw)"""
    fam = FAMILY[codec]
    L = LIBS[fam]
    if fam == "word":
        rclen, rpay = L.ref_chunked_enc(codec, d, chunk)
        clen, pay, _ = L.expected(codec, d, chunk, rclen, rpay)
        return rclen, clen, pay
    clen, pay = L.ref_chunked_enc(codec, d, chunk)
    return clen, clen, pay


def counts(codec, case, rclen, clen):
    """raw / coded / near_limit / expanded of a case from the reference's lengths.  near_limit counts full chunks coded to
    within NEAR bytes of the largest length the reference codes a full chunk of this case to (rcs16, which has no overflow
    test: of the chunk length itself); expanded counts chunks of at least one element that the reference returns more than
    their length for."""
    chunk = case["chunk"]
    lens = chunk_lens(case_n(case), chunk)
    raw = clen.astype(np.int64) == lens
    full = lens == chunk
    coded_full = clen.astype(np.int64)[~raw & full]
    limit = chunk if codec == WL.RCW16 else int(coded_full.max()) if coded_full.size else 0
    return dict(raw=int(raw.sum()), coded=int((~raw).sum()), near_limit=int((coded_full >= limit - NEAR).sum()), limit=limit,
                expanded=int(((rclen.astype(np.int64) > lens) & (lens >= ES[codec])).sum()))


SWEEP_CONFIGS = 16
WORD_MAX_CHUNKS = 1000                                         # word coders: sweep cases other than the multi-round one
LATE_CHUNK = 4096
HASHES = ["in_sha256", "clen_sha256", "payload_sha256"]
STORED = ["chunk", "n", "nchunks", "payload_bytes", "raw", "coded", "near_limit", "limit", "expanded"]   # one list per coder each


def sweep_cases(codec):
    """configurations 0, 1: more than 640 chunks (word coders: 0 is the multi-round case of slots + 70 chunks of 320 bytes);
    2, 3: more than 64; the rest cycle through the three ranges of n"""
    word = FAMILY[codec] == "word"
    for i in range(SWEEP_CONFIGS):
        rng = np.random.Generator(np.random.PCG64(90000 + 97 * codec + i))
        seed = 50000 + 97 * codec + i
        if i < 2:
            chunk, n = int(rng.choice([256, 320, 512])), int(rng.integers(400000, 1500000))
        elif i < 4:
            chunk, n = int(rng.choice([256, 320, 512, 1024])), int(rng.integers(70000, 1500000))
        else:
            lo, hi = [(1, 300), (300, 70000), (70000, 1500000)][i % 3]
            chunk, n = int(rng.choice(SWEEP_CHUNKS)), int(rng.integers(lo, hi))
        if word and i == 0:
            chunk = 320
            n = (WL.slots(codec, 1 << 30) + 70) * chunk - int(rng.integers(1, chunk))
        elif word and n > WORD_MAX_CHUNKS * chunk:
            n = WORD_MAX_CHUNKS * chunk - int(rng.integers(1, chunk))
        kind = str(rng.choice(KINDS[FAMILY[codec]]))
        splice = None
        if rng.random() < 0.3:
            off = int(rng.integers(0, n))
            splice = [off, int(rng.integers(1, min(n - off, 3 * chunk) + 1)), str(rng.choice(["uniform", "const"]))]
        yield dict(fam="sweep", kind=kind, n=n, chunk=chunk, seed=seed, splice=splice)


def wave_cases(codec):
    es = ES[codec]
    lasts = [1, max(es - 1, 1), es + 1]
    k = 0
    for chunk, counts in ((256, WAVE_NCHUNKS), (320, [65, 129, 64 * 7 + 1])):
        for nchunks in counts:
            for pattern in WAVE_PATTERNS:
                yield dict(fam="wave", pattern=pattern, nchunks=nchunks, last=lasts[k % 3], chunk=chunk, seed=60000 + 97 * codec + k)
                k += 1


def ramp_seed(codec, chunk):
    return 70000 + 97 * codec + chunk // 256


def late_seed(codec):
    return 80000 + 97 * codec


def cases(codec, ramp_segs, late_pairs):
    """the cases of one coder in the fixture's order: sweep, wave, the ramps (their segments found by the maker), the late
    surprises (their pairs found by the maker)"""
    return (list(sweep_cases(codec)) + list(wave_cases(codec))
            + [dict(fam="ramp", chunk=c, segs=ramp_segs[str(c)], seed=ramp_seed(codec, c)) for c in RAMP_CHUNKS]
            + [dict(fam="late", chunk=LATE_CHUNK, pairs=late_pairs, seed=late_seed(codec))])


def load():
    """-> {"volume": .., "codecs": {name: [case + stored counts + the three hex digests, ...]}}"""
    with open(GOLD) as f:
        g = json.load(f)
    sha = np.load(GOLD_SHA)
    assert sha.shape[0] == len(CODECS) and sha.shape[2:] == (3, 32) and sha.dtype == np.uint8
    out = {}
    for i, codec in enumerate(CODECS):
        s = g["codecs"][NAMES[codec]]
        cs = cases(codec, s["ramp_segs"], s["late_pairs"])
        assert all(len(s[f]) == len(cs) for f in STORED) and sha.shape[1] == len(cs), NAMES[codec]
        ents = [dict(c, **{f: s[f][k] for f in STORED}, **{h: sha[i, k, j].tobytes().hex() for j, h in enumerate(HASHES)})
                for k, c in enumerate(cs)]
        for e, r in zip([e for e in ents if e["fam"] == "ramp"], s["ramp_raw_before_coded"]):
            e["raw_before_coded"] = r
        assert all(e["chunk"] == c["chunk"] for e, c in zip(ents, cs)), NAMES[codec]
        out[NAMES[codec]] = ents
    return dict(volume=g["volume"], codecs=out)
