"""tests/golden/sweep.json and sweep_sha256.npy without a GPU: they parse, hold all 26 coders outside trc.AVAILABLE and all four case families, meet
the conditions they were generated for (from the stored counts), the inputs regenerate, and, where the reference build is present,
the hashes are the reference's."""
import hashlib
import os
import sys

import numpy as np
import pytest

import sweep_lib as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
FIELDS = {"n", "chunk", "nchunks", "in_sha256", "payload_bytes", "clen_sha256", "payload_sha256", "raw", "coded", "near_limit", "expanded"}


@pytest.fixture(scope="module")
def gold():
    return S.load()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_every_coder_and_family_is_present(gold):
    import trc
    named = sorted(c for c in trc.CODEC_NAMES if 28 <= c <= 55)
    assert named == S.CODECS and len(named) == 26
    assert not set(named) & set(trc.AVAILABLE)
    assert sorted(gold["codecs"]) == sorted(S.NAMES.values())
    for name, ents in gold["codecs"].items():
        assert {e["fam"] for e in ents} == {"sweep", "wave", "ramp", "late"}, name
        for e in ents:
            assert FIELDS <= set(e), (name, e)
            assert e["n"] == S.case_n(e) and e["nchunks"] == (e["n"] + e["chunk"] - 1) // e["chunk"], (name, e)
            assert e["raw"] + e["coded"] == e["nchunks"], (name, e)
            assert e["chunk"] % 64 == 0 and 256 <= e["chunk"] <= 65536


def test_conditions_hold_on_the_stored_counts(gold):
    from make_sweep_golden import check_codec
    volume = 0
    for name, ents in gold["codecs"].items():
        check_codec(name, ents)                                # the maker's own conditions
        sw = [e for e in ents if e["fam"] == "sweep"]
        assert len(sw) >= 16 and sum(e["nchunks"] > 64 for e in sw) >= 4 and sum(e["nchunks"] > 640 for e in sw) >= 2, name
        assert {e["chunk"] for e in sw} <= set(S.SWEEP_CHUNKS), name
        assert min(e["n"] for e in sw) < 300 and max(e["n"] for e in sw) >= 70000, name
        wv = [e for e in ents if e["fam"] == "wave"]
        for pattern in S.WAVE_PATTERNS:
            assert {e["nchunks"] for e in wv if e["pattern"] == pattern and e["chunk"] == 256} == set(S.WAVE_NCHUNKS), (name, pattern)
            assert any(e["chunk"] == 320 for e in wv if e["pattern"] == pattern), (name, pattern)
        es = S.ES[[c for c in S.CODECS if S.NAMES[c] == name][0]]
        assert {e["last"] for e in wv} == {1, max(es - 1, 1), es + 1}, name
        for e in wv:                                           # the layouts the patterns were built for, from the counts
            if not e["pattern"].startswith("hard"):
                want = int(S.wave_mask(e["pattern"], e["nchunks"])[:-1].sum())
                assert want <= e["raw"] <= want + 1, (name, e)
        rp = [e for e in ents if e["fam"] == "ramp"]
        assert sorted(e["chunk"] for e in rp) == S.RAMP_CHUNKS, name
        for e in rp:
            assert e["nchunks"] >= 100, (name, e)
            if name == "rcs16":
                assert e["expanded"] >= 4 and e["near_limit"] >= 4, (name, e)
            else:
                assert e["near_limit"] >= 4 and e["raw"] >= 4 and e["raw_before_coded"] is True, (name, e)
        for e in (e for e in ents if e["fam"] == "late"):
            assert e["raw"] == 0 and len(e["pairs"]) >= 8 and {p[1] for p in e["pairs"]} == {1, 2, 3}, (name, e)
        if S.FAMILY[[c for c in S.CODECS if S.NAMES[c] == name][0]] == "word":
            import word_lib as WL
            codec = [c for c in S.CODECS if S.NAMES[c] == name][0]
            assert sum(e["nchunks"] > WL.slots(codec, 1 << 30) for e in sw) == 1, name      # the multi-round case
        assert sum(e["raw"] for e in ents) >= 50 and sum(e["coded"] for e in ents) >= 500, name
        volume += sum(e["n"] for e in ents)
    assert volume == gold["volume"] <= S.VOLUME_CAP


def test_inputs_regenerate(gold):
    """every case up to 64 KiB and the first ramp of each coder"""
    seen = 0
    for codec in S.CODECS:
        ents = gold["codecs"][S.NAMES[codec]]
        first_ramp = [e for e in ents if e["fam"] == "ramp"][0]
        for e in ents:
            if e["n"] <= 65536 or e is first_ramp:
                assert sha(S.build_input(codec, e)) == e["in_sha256"], (S.NAMES[codec], e)
                seen += 1
    assert seen > 26 * 40


@pytest.mark.parametrize("codec", S.CODECS, ids=lambda c: S.NAMES[c])
def test_fixture_matches_reference(gold, codec):
    """all wave, ramp and late cases and the sweep cases up to 1 MB, recomputed through the reference"""
    if not S.LIBS["intbit"].have_ref():
        pytest.skip("oracle/_ref/libtrc_ref.so not built")
    for e in gold["codecs"][S.NAMES[codec]]:
        if e["fam"] == "sweep" and e["n"] > 10**6:
            continue
        d = S.build_input(codec, e)
        assert sha(d) == e["in_sha256"], e
        rclen, clen, pay = S.ref_lengths(codec, d, e["chunk"])
        assert (int(pay.size), sha(clen.astype("<u4")), sha(pay)) == (e["payload_bytes"], e["clen_sha256"], e["payload_sha256"]), e
        cnt = S.counts(codec, e, rclen, clen)
        assert all(cnt[k] == e[k] for k in cnt), (e, cnt)
