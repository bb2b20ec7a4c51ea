"""CDFs, inputs and the case list of tests/golden/static_cdf.json and static_cdf_sha256.npy: the four static-CDF coders (anscdf4s,
rccdfs, rccdfs2, rccdfsm) under CDFs that a caller made by hand, on data that does not follow them.  Everywhere else the suite derives the CDF from the very
bytes it encodes; here the frequent symbol sits at the bottom, the middle or the top of the CDF, most symbols have f = 1, the
alphabet has 16, 3, 2 or 1 symbols, and the data is anything from the frequent symbol alone to the rare ones alone.

CDFS      name -> frequencies (sum 32768, every f >= 1); cdf(name) -> (uint16[257] with zeros behind cdf[cdfnum], cdfnum)
PATTERNS  what one chunk holds; hot_sym is the argmax of f.  All symbols are < cdfnum.
            hot   hot_sym only                      rare  symbols other than hot_sym, uniform among them
            p01   hot_sym, 1 % other symbols        iid   drawn from the CDF itself
            p38   hot_sym, 3/8 other symbols        unif  uniform over the alphabet
            first symbol 0 only                     last  symbol cdfnum - 1 only
          (`one` has a single symbol: every pattern is `hot` there)
inputs    "mixed": chunk i carries PATTERNS[(i + i // 64) % 8] -- every wave holds all regimes side by side and a lane's regime
          changes from wave to wave; "same:<pattern>": one pattern throughout (hot, p38, rare, last)
case      {cdf, input, chunk, nchunks, n, seed}; "search": 64 top_half / p01 chunks, one per seed the fixture names

The bytes are seeded with PCG64 like the other libs and regenerate from the case alone; the fixture pins them, and each CDF, by
SHA-256."""
import hashlib
import json
import os
import zlib

import numpy as np

import trc_testlib as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "static_cdf.json")
GOLD_SHA = os.path.join(os.path.dirname(GOLD), "static_cdf_sha256.npy")
CODECS = (T.ANS4S, T.RCS1, T.RCS2, T.RCSM)
NAMES = {c: T.CODEC_NAMES[c] for c in CODECS}
PATTERNS = ("hot", "p01", "p38", "rare", "iid", "unif", "first", "last")
SAME = ("hot", "p38", "rare", "last")
INPUTS = ("mixed",) + tuple("same:" + p for p in SAME)
RAGGED_CUT = 101                     # as in test_gpu_ans4s_protocol.py: the last chunk 155 / 411 / 3995 bytes, = 3 mod 4
SHAPES = [(chunk, nch) for chunk in (256, 512) for nch in (17, 64, 65, 200)] + [(4096, 65)]
BIG = [(256, 16448), (256, 8256)]    # 257 groups: 2 waves per workgroup of the rccdfs / rccdfsm decoders; 258 waves of 32 chunks (rccdfs2)
BIG_CDF = "rare_top"
SEARCH_CDF, SEARCH_PATTERN, SEARCH_CHUNK, SEARCH_DRAWS, SEARCH_KEEP = "top_half", "p01", 4096, 2000, 64
SKEWED = ("rare_low", "rare_top", "rare_mid", "three", "two_lo", "two_hi")     # one symbol has nearly all of the range
COUNTS = ("payload_bytes", "raw", "coded", "max_full")
STORED = ("payload_bytes", "raw", "max_full")                     # the columns of the JSON; coded = nchunks - raw


def _stair(k):
    f = np.maximum((np.arange(1, k + 1, dtype=np.int64) * 32768) // (k * (k + 1) // 2), 1)
    f[-1] += 32768 - f.sum()
    return f


def _freqs():
    ones = lambda k: np.ones(k, dtype=np.int64)
    big = np.array([32768 - 255], dtype=np.int64)
    return {
        "rare_low": np.concatenate([big, ones(255)]),
        "rare_top": np.concatenate([ones(255), big]),
        "rare_mid": np.concatenate([ones(127), big, ones(128)]),
        "top_half": np.concatenate([np.full(255, 64, dtype=np.int64), [16448]]),
        "flat": np.full(256, 128, dtype=np.int64),
        "stair": _stair(256),
        "nib": _stair(16),
        "three": np.array([1, 32766, 1], dtype=np.int64),
        "two_lo": np.array([32767, 1], dtype=np.int64),
        "two_hi": np.array([1, 32767], dtype=np.int64),
        "two_eq": np.array([16384, 16384], dtype=np.int64),
        "one": np.array([32768], dtype=np.int64),
    }


CDFS = _freqs()


def cdf(name):
    """-> (uint16[257], cdfnum): cdf[0] = 0, cdf[cdfnum] = 32768, zeros behind it"""
    f = CDFS[name]
    assert f.sum() == 32768 and f.min() >= 1
    out = np.zeros(257, dtype=np.uint16)
    out[1:f.size + 1] = np.cumsum(f).astype(np.uint16)
    return out, int(f.size)


def cdf_sha(name):
    return hashlib.sha256(cdf(name)[0].astype("<u2").tobytes()).hexdigest()


def hot_sym(name):
    return int(np.argmax(CDFS[name]))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pattern_rows(name, pats, chunk, seed):
    """one row of `chunk` bytes per entry of pats (indices into PATTERNS), under the CDF `name`"""
    f = CDFS[name]
    k, hot = f.size, hot_sym(name)
    pats = np.asarray(pats, dtype=np.int64)
    rows = pats.size
    rng = np.random.Generator(np.random.PCG64(seed))
    if k == 1:
        return np.zeros((rows, chunk), dtype=np.uint8)
    out = np.empty((rows, chunk), dtype=np.uint8)
    for p in sorted(set(pats.tolist())):                          # (the draws of a pattern that no row has are not made)
        m = pats == p
        shape = (int(m.sum()), chunk)
        other = None
        if p in (1, 2, 3):
            other = rng.integers(0, k - 1, shape)
            other = other + (other >= hot)                        # uniform among the symbols that are not hot
        if p == 0:
            v = hot
        elif p == 1:
            v = np.where(rng.integers(0, 100, shape) < 1, other, hot)
        elif p == 2:
            v = np.where(rng.integers(0, 8, shape) < 3, other, hot)
        elif p == 3:
            v = other
        elif p == 4:
            v = np.searchsorted(np.cumsum(f), rng.integers(0, 32768, shape), side="right")
        elif p == 5:
            v = rng.integers(0, k, shape)
        else:
            v = 0 if p == 6 else k - 1
        out[m] = v
    return out


def chunk_patterns(inp, nchunks):
    if inp == "mixed":
        i = np.arange(nchunks)
        return (i + i // 64) % 8
    return np.full(nchunks, PATTERNS.index(inp.split(":")[1]))


def case_name(c):
    return "search" if c["input"] == "search" else "%s/%s/%d/%d/%d" % (c["cdf"], c["input"], c["chunk"], c["nchunks"], c["n"])


def names_sha(cases):
    return hashlib.sha256("\n".join(case_name(c) for c in cases).encode()).hexdigest()


def make_case(name, inp, chunk, nchunks, n):
    c = dict(cdf=name, input=inp, chunk=chunk, nchunks=nchunks, n=n)
    c["seed"] = zlib.crc32(case_name(c).encode())
    return c


def small_cases():
    """the cases of at most 200 chunks: every CDF x input x shape, whole and ragged, and per CDF one that ends in a 1-byte chunk
    (`one`: "mixed" and "same:hot" only -- its other inputs would be the same bytes)"""
    out = []
    for name in CDFS:
        for inp in (("mixed", "same:hot") if name == "one" else INPUTS):
            for chunk, nch in SHAPES:
                for n in (nch * chunk, nch * chunk - RAGGED_CUT):
                    out.append(make_case(name, inp, chunk, nch, n))
        out.append(make_case(name, "mixed", 256, 66, 65 * 256 + 1))
    return out


def big_cases():
    return [make_case(BIG_CDF, "mixed", chunk, nch, nch * chunk) for chunk, nch in BIG]


def search_case(seeds):
    return dict(cdf=SEARCH_CDF, input="search", chunk=SEARCH_CHUNK, nchunks=len(seeds), n=len(seeds) * SEARCH_CHUNK, seeds=list(seeds))


def search_chunk(seed):
    return pattern_rows(SEARCH_CDF, [PATTERNS.index(SEARCH_PATTERN)], SEARCH_CHUNK, seed)[0]


def build_input(c):
    if c["input"] == "search":
        return np.concatenate([search_chunk(s) for s in c["seeds"]])
    rows = pattern_rows(c["cdf"], chunk_patterns(c["input"], c["nchunks"]), c["chunk"], c["seed"])
    return np.ascontiguousarray(rows.reshape(-1)[:c["n"]])


def chunk_lens(n, chunk):
    return np.minimum(chunk, n - np.arange(0, n, chunk)).astype(np.int64)


def longest_run(a, value=0xFF):
    """the longest run of `value` in the byte array a"""
    m = np.concatenate([[0], (np.asarray(a) == value).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(m))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def counts(c, clen):
    """payload_bytes / raw / coded of a case from its stored lengths; max_full: the longest stored length among chunks of at
    least 256 bytes"""
    lens = chunk_lens(c["n"], c["chunk"])
    cl = clen.astype(np.int64)
    raw = cl == lens
    return dict(payload_bytes=int(cl.sum()), raw=int(raw.sum()), coded=int((~raw).sum()), max_full=int(cl[lens >= 256].max()))


def load():
    """-> {"cdf_sha256": {name: hex}, "search": {"seeds", "longest_ff_run", ..}, "cases": [case + name + in_sha256 + {coder name: entry}]}
    where entry = {n, chunk, nchunks, payload_bytes, raw, coded, max_full, in_sha256, clen_sha256, payload_sha256}: the shape
    gpu_contracts.encode_checked consumes.  The case list is rebuilt here and pinned by the hash of its names; static_cdf.json holds
    one column per stored count (coded = nchunks - raw), static_cdf_sha256.npy the digests: [case, 0] the input's, [case, 1 + 2 i]
    and [case, 2 + 2 i] those of the lengths and the payload of coder i of CODECS."""
    with open(GOLD) as f:
        g = json.load(f)
    dig = np.load(GOLD_SHA)
    cs = small_cases() + big_cases() + [search_case(g["search"]["seeds"])]
    assert len(cs) == g["ncases"] and names_sha(cs) == g["names_sha256"]
    assert dig.shape == (len(cs), 1 + 2 * len(CODECS), 32) and dig.dtype == np.uint8
    out = []
    for k, c in enumerate(cs):
        e = dict(c, name=case_name(c), in_sha256=dig[k, 0].tobytes().hex())
        for i, codec in enumerate(CODECS):
            col = g["codecs"][NAMES[codec]]
            ent = dict(n=c["n"], chunk=c["chunk"], nchunks=c["nchunks"], in_sha256=e["in_sha256"], **{h: col[h][k] for h in STORED},
                       clen_sha256=dig[k, 1 + 2 * i].tobytes().hex(), payload_sha256=dig[k, 2 + 2 * i].tobytes().hex())
            ent["coded"] = c["nchunks"] - ent["raw"]
            e[NAMES[codec]] = ent
        out.append(e)
    return dict(cdf_sha256=g["cdf_sha256"], search=g["search"], cases=out)
