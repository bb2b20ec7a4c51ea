"""tests/golden/bytesweep.json and bytesweep_sha256.npy without a GPU: they parse, hold the seven byte-level bitwise coders
(rc4s, rc4cs, rcu3s, rcss, rc4ss, rc4css, rcu3ss) and all their case families, meet the conditions they were generated for (from
the stored counts), the inputs regenerate, and, where the reference is present, the hashes are the reference's."""
import hashlib
import os
import sys

import numpy as np
import pytest

import bytesweep_lib as B

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
FIELDS = set(B.STORED) | set(B.HASHES) | {"fam", "chunk", "seed"}
by_name = pytest.mark.parametrize("codec", B.CODECS, ids=lambda c: B.NAMES[c])


@pytest.fixture(scope="module")
def gold():
    return B.load()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_every_coder_and_family_is_present(gold):
    import trc
    assert B.CODECS == [58, 59, 60, 62, 63, 64, 65] and sorted(B.NIBBLE + B.BYTE) == B.CODECS
    assert all(trc.CODEC_NAMES[c] == B.NAMES[c] for c in B.CODECS)
    assert sorted(gold["codecs"]) == sorted(B.NAMES.values())
    for codec in B.CODECS:
        ents = gold["codecs"][B.NAMES[codec]]
        assert [f for f in B.FAMILIES if any(e["fam"] == f for e in ents)] == B.families(codec)
        for e in ents:
            assert FIELDS <= set(e), (B.NAMES[codec], e)
            assert ("prm" in e) == (codec in B.SS), (B.NAMES[codec], e)
            assert e["chunk"] % 64 == 0 and 256 <= e["chunk"] <= 4096
    for f in (B.GOLD, B.GOLD_SHA):
        assert os.path.getsize(f) < B.FILE_CAP, f


def test_conditions_hold_on_the_stored_counts(gold):
    from make_bytesweep_golden import check_codec
    volume = 0
    for codec in B.CODECS:
        name = B.NAMES[codec]
        ents, info = gold["codecs"][name], gold["info"][name]
        check_codec(codec, ents, info)                          # the maker's own conditions
        assert sum(e["fam"] == "tail" for e in ents) == 172, name
        wv = [e for e in ents if e["fam"] == "wave" and not e.get("again")]
        assert len(wv) == 45 and max(e["nchunks"] for e in wv) == 449, name
        if codec in B.SS:                                       # every pair on one input, and a series with a raw length
            again = [e for e in ents if e.get("again")]         # behind a coded one
            (base,) = [e for e in wv if (e["pattern"], e["nchunks"], e["chunk"]) == ("alt", 129, 256)]
            assert len(again) == len(B.PRMS) and {e["in_sha256"] for e in again} == {base["in_sha256"]}, name
            assert len({e["payload_sha256"] for e in again}) >= (1 if codec in B.FIXED else 4), name
            assert [e for e in again if tuple(e["prm"]) == B.DEFAULT][0]["payload_sha256"] == base["payload_sha256"], name
            assert max(info["tail_transitions"].values()) > 1, name
        if codec in B.NIBBLE:
            assert "ramp_segs" not in info and info["max_raw_last"] <= 40, name
        else:
            for e in (e for e in ents if e["fam"] == "ramp"):
                coarse, fine = B.RAMP_COUNTS[e["chunk"]]
                assert [s[0] for s in e["segs"]] == [coarse, fine] and e["segs"][0][1:] == [e["chunk"] // 2, e["chunk"]], (name, e)
                assert e["limit"] < e["chunk"] and e["limit"] >= e["chunk"] - 2 * B.NEAR, (name, e)
        volume += sum(e["n"] for e in ents)
    assert volume == gold["volume"] <= B.VOLUME_CAP


def test_inputs_regenerate(gold):
    """every case up to 64 KiB, and every ramp"""
    seen = 0
    for codec in B.CODECS:
        for e in gold["codecs"][B.NAMES[codec]]:
            if e["n"] <= 65536 or e["fam"] == "ramp":
                d = B.build_input(codec, e)
                assert d.size == e["n"] and d.dtype == np.uint8 and sha(d) == e["in_sha256"], (B.NAMES[codec], e)
                seen += 1
    assert seen >= 7 * (172 + 25)


def test_expected_of_follows_the_stored_counts(gold):
    """what the GPU tests compare a nibble coder's decodes with: the low nibbles, except in a raw ragged last chunk"""
    for codec in B.NIBBLE:
        tl = [e for e in gold["codecs"][B.NAMES[codec]] if e["fam"] == "tail" and e["head"] == 64 and e["kind"] == "nib_uniform"]
        raw, coded = [e for e in tl if e["raw"]][0], [e for e in tl if not e["raw"]][0]
        for e in (raw, coded):
            d = B.build_input(codec, e)
            want = B.expected_of(codec, d, e)
            head = 64 * e["chunk"]
            assert np.array_equal(want[:head], d[:head] & 15) and (d[:head] > 15).any()
            assert np.array_equal(want[head:], d[head:])        # (nib_uniform: raw or coded, the bytes are their low nibbles)
    for codec in B.BYTE:
        e = gold["codecs"][B.NAMES[codec]][0]
        d = B.build_input(codec, e)
        assert B.expected_of(codec, d, e) is d


@by_name
def test_fixture_matches_reference(gold, codec):
    """every case recomputed through the reference"""
    if not B.have_ref():
        pytest.skip("oracle/_ref/libtrc_ref.so or the reference sources are not here")
    for e in gold["codecs"][B.NAMES[codec]]:
        d = B.build_input(codec, e)
        assert sha(d) == e["in_sha256"], e
        clen, pay = B.ref_chunked_enc(codec, d, e["chunk"], B.prm_of(e))
        assert (int(pay.size), sha(clen.astype("<u4")), sha(pay)) == (e["payload_bytes"], e["clen_sha256"], e["payload_sha256"]), e
        cnt = B.counts(e, clen)
        assert all(cnt[k] == e[k] for k in cnt), (e, cnt)
