"""Inputs, case lists and reference calls of tests/golden/bytesweep.json and bytesweep_sha256.npy: the seven byte-level bitwise
coders of nibbit_lib and ssbit_lib (rc4s, rc4cs, rcu3s: 58-60; rcss, rc4ss, rc4css, rcu3ss: 62-65) on many-wave shapes, on
every short last chunk around the raw decision, at the raw / coded threshold and in used workspaces.

NIBBLE coders code d & 15 and never store a full chunk raw; BYTE coders return the input and go raw on uniform bytes.
Every case is a small dict from which build_input(codec, case) regenerates the bytes (seeded with PCG64); an "ss" coder's case
carries its parameter pair `prm`:
  wave   {pattern, nchunks, last, chunk, seed}: `nchunks - 1` full chunks and a last one of `last` bytes; the chunks of
           sweep_lib.wave_mask(pattern) are bytes_uniform (byte coders: raw; nibble coders: a long payload), the others
           bytes_small (coded / short); hard0 / hard1 are bytes_uniform / zeros over the whole input
  tail   {head, last, kind, chunk, seed}: `head` full chunks of bytes_small and a last chunk of `last` bytes of `kind`
  ramp   {chunk, segs: [[count, lo, hi], ...], seed}: per chunk a bytes_small head and a uniform tail whose length goes from
           lo to hi bytes over the segment's chunks (a coarse segment over the upper half, a fine one around the crossover)
  late   {chunk, pairs: [[t, nsur], ...], seed}: pairs of chunks; the first is t uniform bytes, then bytes of value 5, then
           nsur bytes of SURPRISE, coded to just below the raw limit; the second an ordinary bytes_small chunk
"""
import json
import os
import tempfile

import numpy as np

import nibbit_lib as NL
import ssbit_lib as SL
import sweep_lib as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytesweep.json")
GOLD_SHA = os.path.join(os.path.dirname(GOLD), "bytesweep_sha256.npy")
CODECS = NL.CODECS + SL.CODECS
NAMES = {**NL.NAMES, **SL.NAMES}
NIBBLE = (58, 59, 63, 64)
BYTE = (60, 62, 65)
FIXED = (59, 64)                                               # rc4cs, rc4css: no model, every full chunk codes to one length
SS = tuple(SL.CODECS)
DEFAULT = SL.DEFAULT
PRMS = SL.PRMS
NEAR = S.NEAR
WORK_CAP = S.WORK_CAP
VOLUME_CAP = 64 * 10**6
FILE_CAP = 256 * 1024
gen = NL.gen
uniform, chunk_lens, wave_mask, ramp_tails = S.uniform, S.chunk_lens, S.wave_mask, S.ramp_tails

FAMILIES = ["wave", "tail", "ramp", "late"]
WAVE_NCHUNKS = {256: [63, 64, 65, 127, 128, 129, 64 * 7 + 1], 320: [65, 129]}
WAVE_PATTERNS = S.WAVE_PATTERNS
WAVE_LASTS = [1, 9, 17, 25, 255]
TAIL_CHUNK = 256
TAIL_HEADS = [0, 64]
TAIL_LENS = list(range(1, 41)) + [63, 64, 65]
TAIL_KINDS = ["zeros", "nib_uniform"]
RAMP_CHUNKS = [256, 4096]
RAMP_COUNTS = {256: (120, 180), 4096: (60, 90)}               # (coarse, fine) chunks
LATE_CHUNK = 1024
LATE_PAIRS = 9
SURPRISE = [0xFF, 0xAA, 0x7F]
HASHES = ["in_sha256", "clen_sha256", "payload_sha256"]
STORED = ["n", "nchunks", "payload_bytes", "raw", "coded", "near_limit", "limit"]     # one list per coder each


def families(codec):
    return FAMILIES if codec in BYTE else FAMILIES[:2]


def prm_of(case):
    """the case's parameter pair, None for an "s" coder (which has none)"""
    return tuple(case["prm"]) if "prm" in case else None


def expected(codec, d, clen, chunk):
    return (NL if codec in NL.CODECS else SL).expected(codec, d, clen, chunk)


def expected_of(codec, d, ent):
    """what a decoder returns for fixture entry `ent`, from its stored counts: a nibble coder's only raw chunk is the ragged
    last one (the maker asserts it), so `raw` says whether that one holds the input's bytes or their low nibbles"""
    lens = chunk_lens(ent["n"], ent["chunk"])
    clen = np.zeros(lens.size, np.int64)
    if codec in NIBBLE:
        assert ent["raw"] in (0, 1), ent
        if ent["raw"]:
            clen[-1] = lens[-1]
    return expected(codec, d, clen, ent["chunk"])


def case_n(case):
    f = case["fam"]
    if f == "wave":
        return (case["nchunks"] - 1) * case["chunk"] + case["last"]
    if f == "tail":
        return case["head"] * case["chunk"] + case["last"]
    if f == "ramp":
        return sum(s[0] for s in case["segs"]) * case["chunk"]
    return 2 * len(case["pairs"]) * case["chunk"] - 37           # late: the last neighbour is ragged


def late_chunk(chunk, t, nsur, seed):
    d = np.full(chunk, 5, dtype=np.uint8)
    d[:t] = uniform(t, seed)
    d[chunk - nsur:] = SURPRISE[:nsur]
    return d


def build_input(codec, case):
    f, seed, chunk = case["fam"], case["seed"], case["chunk"]
    n = case_n(case)
    if f == "wave":
        if case["pattern"].startswith("hard"):
            return gen(["bytes_uniform", "zeros"][int(case["pattern"][4])], n, seed)
        d = gen("bytes_small", n, seed)
        m = np.repeat(wave_mask(case["pattern"], case["nchunks"]), chunk)[:n]
        d[m] = uniform(n, seed + 1)[m]
        return d
    if f == "tail":
        d = gen("bytes_small", n, seed)
        d[case["head"] * chunk:] = gen(case["kind"], case["last"], seed + 1)
        return d
    if f == "ramp":
        d = gen("bytes_small", n, seed)
        pos = np.arange(n) % chunk
        m = pos >= chunk - np.repeat(ramp_tails(case), chunk)
        d[m] = uniform(n, seed + 1)[m]
        return d
    if f == "late":
        d = gen("bytes_small", n + 37, seed)
        for j, (t, nsur) in enumerate(case["pairs"]):
            d[2 * j * chunk:(2 * j + 1) * chunk] = late_chunk(chunk, t, nsur, seed + 1 + j)
        return d[:n]
    raise ValueError(f)


# ---------------------------------------------------------------------------------- the reference (maker and CPU test only) ---
_REF = {}


def have_ref():
    return NL.have_ref() and SL.have_ref_sources()


def ss_ref():
    """ssbit_lib.Ref, compiled once per process into a temporary directory"""
    if "ss" not in _REF:
        _REF["tmp"] = tempfile.TemporaryDirectory()
        _REF["ss"] = SL.Ref(_REF["tmp"].name)
    return _REF["ss"]


def ref_enc(codec, data, prm=None):
    """one call of the reference encoder on `data`"""
    return NL.ref_enc(codec, data) if codec in NL.CODECS else ss_ref().enc(codec, data, tuple(prm or DEFAULT))


def ref_chunked_enc(codec, d, chunk, prm=None):
    """-> (clen u32 array, payload u8 array): the reference called once per chunk"""
    if codec in NL.CODECS:
        return NL.ref_chunked_enc(codec, d, chunk)
    return ss_ref().chunked_enc(codec, d, chunk, tuple(prm or DEFAULT))


def counts(case, clen):
    """raw / coded / near_limit / limit of a case from the reference's lengths.  limit is the largest length the reference
    codes a full chunk of this case to, near_limit the full chunks coded to within NEAR bytes of it."""
    chunk = case["chunk"]
    lens = chunk_lens(case_n(case), chunk)
    cl = clen.astype(np.int64)
    raw = cl == lens
    coded_full = cl[~raw & (lens == chunk)]
    limit = int(coded_full.max()) if coded_full.size else 0
    return dict(raw=int(raw.sum()), coded=int((~raw).sum()), near_limit=int((coded_full >= limit - NEAR).sum()), limit=limit)


def transitions(flags):
    """raw / coded changes along a series of last-chunk lengths"""
    f = np.asarray(flags, dtype=bool)
    return int((f[1:] != f[:-1]).sum())


# ------------------------------------------------------------------------------------------------------------ case lists ---
def _with_prm(codec, case, prm=DEFAULT):
    return dict(case, prm=list(prm)) if codec in SS else case


def wave_cases(codec):
    k = 0
    again = None
    for chunk in (256, 320):
        for nchunks in WAVE_NCHUNKS[chunk]:
            for pattern in WAVE_PATTERNS:
                case = dict(fam="wave", pattern=pattern, nchunks=nchunks, last=WAVE_LASTS[k % 5], chunk=chunk, seed=160000 + 97 * codec + k)
                if (pattern, nchunks, chunk) == ("alt", 129, 256):
                    again = case
                yield _with_prm(codec, case)
                k += 1
    if codec in SS:                                            # the alt / 129 / 256 input once more for each pair
        for prm in PRMS:
            yield dict(again, prm=list(prm), again=True)


def tail_cases(codec):
    k = 0
    for head in TAIL_HEADS:
        for kind in TAIL_KINDS:
            for last in TAIL_LENS:
                yield _with_prm(codec, dict(fam="tail", head=head, last=last, kind=kind, chunk=TAIL_CHUNK, seed=170000 + 997 * codec + k))
                k += 1


def ramp_seed(codec, chunk):
    return 180000 + 97 * codec + chunk // 256


def late_seed(codec):
    return 190000 + 97 * codec


def cases(codec, ramp_segs=None, late_pairs=None):
    """the cases of one coder in the fixture's order: wave, tail and, for a byte coder, the ramps (their segments found by the
    maker) and the late surprises (their pairs found by the maker)"""
    out = list(wave_cases(codec)) + list(tail_cases(codec))
    if codec in BYTE:
        out += [_with_prm(codec, dict(fam="ramp", chunk=c, segs=ramp_segs[str(c)], seed=ramp_seed(codec, c))) for c in RAMP_CHUNKS]
        out += [_with_prm(codec, dict(fam="late", chunk=LATE_CHUNK, pairs=late_pairs, seed=late_seed(codec)))]
    return out


def load():
    """-> {"volume": .., "codecs": {name: [case + stored counts + the three hex digests, ...]}, "info": {name: the coder's
    searched parameters and per-coder records}}.  Case k of coder i is row (cases of the coders before i) + k of the digests."""
    with open(GOLD) as f:
        g = json.load(f)
    sha = np.load(GOLD_SHA)
    assert sha.ndim == 3 and sha.shape[1:] == (3, 32) and sha.dtype == np.uint8
    out, info, row = {}, {}, 0
    for codec in CODECS:
        s = g["codecs"][NAMES[codec]]
        cs = cases(codec, s.get("ramp_segs"), s.get("late_pairs"))
        assert all(len(s[f]) == len(cs) for f in STORED), NAMES[codec]
        ents = [dict(c, **{f: s[f][k] for f in STORED}, **{h: sha[row + k, j].tobytes().hex() for j, h in enumerate(HASHES)})
                for k, c in enumerate(cs)]
        row += len(cs)
        out[NAMES[codec]] = ents
        info[NAMES[codec]] = {k: v for k, v in s.items() if k not in STORED}
    assert row == sha.shape[0]
    return dict(volume=g["volume"], codecs=out, info=info)
