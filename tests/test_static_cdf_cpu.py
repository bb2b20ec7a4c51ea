"""CPU side of tests/golden/static_cdf.json (static coders under caller-made CDFs, tests/static_cdf_lib.py): inputs and CDFs
regenerate to the pinned hashes, the oracle's per-chunk encode hashes to the fixture and its decode returns the input (no reference
build needed), the reference itself does where oracle/_ref/libtrc_ref.so exists, and the data does what it is here for.
tests/test_gpu_static_cdf.py holds the device against the same fixture."""
import numpy as np
import pytest

import static_cdf_lib as S
import trc_testlib as T

CODEC_IDS = dict(ids=lambda c: S.NAMES[c])


@pytest.fixture(scope="module")
def gold():
    return S.load()


@pytest.fixture(scope="module")
def inputs(gold):
    """every input of the fixture, built once"""
    return [S.build_input(c) for c in gold["cases"]]


def test_cdfs_are_the_pinned_ones(gold):
    assert list(gold["cdf_sha256"]) == list(S.CDFS)
    for name, f in S.CDFS.items():
        cdf, cdfnum = S.cdf(name)
        assert cdf.dtype == np.uint16 and cdf.size == 257 and cdf[0] == 0 and cdf[cdfnum] == 32768 and not cdf[cdfnum + 1:].any(), name
        assert (np.diff(cdf[:cdfnum + 1].astype(np.int64)) == f).all() and f.min() >= 1, name
        assert S.cdf_sha(name) == gold["cdf_sha256"][name], name
    f = S.CDFS
    assert f["rare_low"][0] == f["rare_top"][255] == f["rare_mid"][127] == 32768 - 255 and f["top_half"][255] == 16448
    assert f["stair"][0] == 1 and (np.diff(f["stair"][:-1]) >= 0).all() and [S.cdf(n)[1] for n in ("nib", "three", "two_eq", "one")] == [16, 3, 2, 1]


def test_inputs_regenerate(gold, inputs):
    assert len(gold["cases"]) == len(S.small_cases()) + len(S.BIG) + 1
    for c, d in zip(gold["cases"], inputs):
        assert d.dtype == np.uint8 and d.size == c["n"] and int(d.max()) < S.cdf(c["cdf"])[1], c["name"]
        assert S.sha(d) == c["in_sha256"], c["name"]
        assert c["nchunks"] == (c["n"] + c["chunk"] - 1) // c["chunk"], c["name"]


def test_case_list(gold):
    """the shapes, inputs and CDFs the fixture was asked for"""
    small = [c for c in gold["cases"] if c["nchunks"] <= 200 and c["input"] != "search"]
    for name in S.CDFS:
        mine = [c for c in small if c["cdf"] == name]
        want = ("mixed", "same:hot") if name == "one" else S.INPUTS
        for inp in want:
            got = sorted((c["chunk"], c["nchunks"], c["n"]) for c in mine if c["input"] == inp and c["n"] % c["chunk"] != 1)
            assert got == sorted((ch, k, n) for ch, k in S.SHAPES for n in (ch * k, ch * k - S.RAGGED_CUT)), (name, inp)
        assert sum(c["n"] % c["chunk"] == 1 for c in mine) == 1, name
    big = [c for c in gold["cases"] if c["nchunks"] > 200]
    assert [(c["cdf"], c["input"], c["chunk"], c["nchunks"]) for c in big] == [("rare_top", "mixed", 256, 16448), ("rare_top", "mixed", 256, 8256)]
    s = gold["cases"][-1]
    assert s["input"] == "search" and s["nchunks"] == S.SEARCH_KEEP == len(set(s["seeds"])) and max(s["seeds"]) < S.SEARCH_DRAWS


def test_mixed_puts_every_pattern_into_every_wave():
    p = S.chunk_patterns("mixed", 200)
    assert all(set(p[w:w + 64].tolist()) == set(range(8)) for w in (0, 64, 128)) and (p[:64] != p[64:128]).all()


@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_oracle_matches_fixture(gold, inputs, codec):
    for c, d in zip(gold["cases"], inputs):
        e = c[S.NAMES[codec]]
        cdf, cdfnum = S.cdf(c["cdf"])
        pay, clen, _ = T.orc_chunked_enc(codec, d, c["chunk"], cdf, cdfnum)
        assert clen.size == e["nchunks"] and pay.size == e["payload_bytes"], c["name"]
        assert S.sha(clen.astype("<u4")) == e["clen_sha256"] and S.sha(pay) == e["payload_sha256"], c["name"]
        assert S.counts(c, clen) == {h: e[h] for h in S.COUNTS}, c["name"]
        assert np.array_equal(T.orc_chunked_dec(codec, pay, clen, d.size, c["chunk"], cdf, cdfnum), d), c["name"]


REF_DECODERS = {T.ANS4S: (), T.RCS1: ("l", "b", "vl", "vb"), T.RCS2: ("b",), T.RCSM: ("b", "l")}      # (rccdfs2: rccdfsb2dec)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref/libtrc_ref.so not built")
@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_reference_matches_fixture(gold, inputs, codec):
    """the 256- and 512-byte cases of 17 and 65 chunks: the reference's encode, and every reference decoder of every coded chunk"""
    from golden.make_static_cdf_golden import ref_chunked
    ran = 0
    for c, d in zip(gold["cases"], inputs):
        if c["chunk"] not in (256, 512) or c["nchunks"] not in (17, 65):
            continue
        e = c[S.NAMES[codec]]
        cdf, cdfnum = S.cdf(c["cdf"])
        clen, pay = ref_chunked(codec, d, c["chunk"], cdf, cdfnum)
        assert S.sha(clen.astype("<u4")) == e["clen_sha256"] and S.sha(pay) == e["payload_sha256"], c["name"]
        off = np.concatenate([[0], np.cumsum(clen.astype(np.int64))])
        for k, ln in enumerate(S.chunk_lens(d.size, c["chunk"])):
            if clen[k] == ln:
                continue
            piece = d[k * c["chunk"]:k * c["chunk"] + ln]
            for s in REF_DECODERS[codec]:
                assert np.array_equal(T.ref_dec(codec, pay[off[k]:off[k + 1]], int(ln), cdf, cdfnum, search=s), piece), (c["name"], k, s)
        ran += 1
    assert ran == 11 * 5 * 8 + 2 * 8


@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_the_data_does_what_it_is_here_for(gold, codec):
    """from the stored counts.  Under a CDF that gives one symbol nearly all of the range: a mixed input stores at least one chunk
    in eight raw (the all-rare ones) and codes at least one in four (hot, p01, p38, iid); the frequent symbol alone codes to next
    to nothing; the rare symbols alone are stored raw.  For the other CDFs the counts are recorded, not asserted."""
    seen = set()
    for c in gold["cases"]:
        e = c[S.NAMES[codec]]
        assert e["raw"] + e["coded"] == c["nchunks"], c["name"]
        if c["input"] == "search" or c["cdf"] not in S.SKEWED + ("one",):
            continue
        if c["input"] == "mixed" and c["cdf"] in S.SKEWED:
            assert 8 * e["raw"] >= c["nchunks"] and 4 * e["coded"] >= c["nchunks"], (c["name"], e["raw"], e["coded"])
        if c["input"] == "same:hot":
            assert e["max_full"] <= 16, (c["name"], e["max_full"])
        if c["input"] == "same:rare":
            assert e["coded"] == 0, c["name"]
        seen.add((c["cdf"], c["input"]))
    assert len(seen) == 6 * 5 + 2


def test_search_case(gold, inputs):
    """the kept chunks give the recorded run of 0xFF bytes in rccdfs' output (by the oracle here; the maker used the reference)"""
    s, d = gold["cases"][-1], inputs[-1]
    cdf, cdfnum = S.cdf(S.SEARCH_CDF)
    runs = [S.longest_run(T.orc_enc(T.RCS1, d[o:o + S.SEARCH_CHUNK], cdf, cdfnum)) for o in range(0, d.size, S.SEARCH_CHUNK)]
    assert runs == gold["search"]["runs_kept"] and max(runs) == gold["search"]["longest_ff_run"]
    assert s[S.NAMES[T.RCS1]]["raw"] == 0
