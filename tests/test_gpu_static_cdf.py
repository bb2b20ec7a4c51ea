"""The four static-CDF coders (anscdf4s, rccdfs, rccdfs2, rccdfsm) on the MI355X under CDFs that a caller made by hand, on data that
does not follow them (tests/static_cdf_lib.py): the frequent symbol at the bottom, the middle or the top of the CDF, runs of f = 1
symbols, alphabets of 16, 3, 2 and 1 symbols, every wave a mix of regimes.  Everywhere else the suite hands these coders the CDF
of the very bytes it encodes (test_gpu_ans4s_protocol.py: one hand-made CDF, anscdf4s only).

Expected lengths and payloads are the hashes of tests/golden/static_cdf.json, made through the reference; decodes return the
input.  Every comparison is byte or hash equality, nothing has a tolerance.  On a mismatch the message names the first differing
chunk and byte by the oracle's encode -- for diagnosis only, the verdict is the fixture's."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gpu_contracts as G
import static_cdf_lib as S
import trc
import trc_testlib as T
from gpu_contracts import to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
CODEC_IDS = dict(ids=lambda c: S.NAMES[c])
GUARD = 512
RANGES = [(0, 1), (63, 2), (64, 64), (137, 63), (199, 1), (0, 200)]
# the workgroup shapes of test_gpu_parity.py::test_round5_workgroup_shapes, each forced in a process of its own
FORMS = (dict(TRC_ENC_WPB="12", TRC_RCS_ENC_WPB="12", TRC_CODEQ_GPW="4", TRC_O1_ROWS="4", TRC_NIB_BIG="1"),
         dict(TRC_ENC_WPB="4", TRC_RCS_ENC_WPB="1", TRC_CODEQ_GPW="1", TRC_O1_ROWS="1", TRC_NIB_BIG="0"))
FORM_CDFS = ("rare_low", "rare_top", "top_half", "two_hi", "one")


@pytest.fixture(scope="module")
def gold():
    return S.load()


class Inputs:
    """the bytes of a case, built at first use"""

    def __init__(self):
        self.made = {}

    def __call__(self, case):
        key = S.case_name(case) + str(case.get("seeds", ""))
        if key not in self.made:
            self.made[key] = S.build_input(case)
        return self.made[key]


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


def diagnose(codec, d, case):
    """-> diagnose(clen, payload) for gpu_contracts: the first chunk and byte that differ from the oracle's encode"""
    def f(clen, payload):
        cdf, cdfnum = S.cdf(case["cdf"])
        ep, ec, _ = T.orc_chunked_enc(codec, d, case["chunk"], cdf, cdfnum)
        if clen.size != ec.size:
            return "directory of %d chunks, the oracle's has %d" % (clen.size, ec.size)
        bad = np.flatnonzero(clen != ec)
        if bad.size:
            return "first differing length: chunk %d, %d bytes (oracle %d)" % (bad[0], clen[bad[0]], ec[bad[0]])
        m = min(ep.size, payload.size)
        bad = np.flatnonzero(payload[:m] != ep[:m])
        if not bad.size:
            return "lengths and payload equal the oracle's"
        k = int(np.searchsorted(np.cumsum(ec.astype(np.int64)), bad[0], side="right"))
        start = int(ec[:k].astype(np.int64).sum())
        return "first differing byte: chunk %d (%s, stored %d bytes), byte %d of it: 0x%02x, oracle 0x%02x" % (
            k, S.PATTERNS[int(S.chunk_patterns(case["input"], case["nchunks"])[k])] if case["input"] != "search" else "p01",
            ec[k], bad[0] - start, payload[bad[0]], ep[bad[0]])
    return f


def checked(which, torch, dc, case, codec, d):
    cdf = S.cdf(case["cdf"])
    getattr(G, which)(torch, dc, d, to_dev(torch, d), case[S.NAMES[codec]], "%s %s" % (S.NAMES[codec], case["name"]),
                      diagnose(codec, d, case), cdf=cdf)


@pytest.mark.parametrize("chunk", (256, 512, 4096))
@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_contracts(torch_cuda, gold, inputs, codec, chunk):
    """every case of up to 200 chunks through gpu_contracts.contracts, all in ONE DeviceCoder sized for the largest, by
    descending and then by ascending n, the CDF another one at every step: no table of the CDF before may survive"""
    torch = torch_cuda
    cases = [c for c in gold["cases"] if c["chunk"] == chunk and c["nchunks"] <= 200 and c["input"] != "search"]
    order = sorted(cases, key=lambda c: (-c["n"], c["input"], list(S.CDFS).index(c["cdf"])))
    assert len(cases) == {256: 11 * 41 + 17, 512: 11 * 40 + 16, 4096: 11 * 10 + 4}[chunk]
    assert sum(a["cdf"] != b["cdf"] for a, b in zip(order, order[1:])) >= len(order) - 12
    dc = trc.DeviceCoder(codec, max(c["n"] for c in cases), chunk, "cuda:0")
    for case in order + order[::-1]:
        checked("contracts", torch, dc, case, codec, inputs(case))


@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_many_groups_and_the_search_case(torch_cuda, gold, inputs, codec):
    """16 448 and 8 256 chunks of 256 bytes (257 groups: two waves per workgroup of the rccdfs / rccdfsm decoders; 258 waves of
    32 chunks of rccdfs2's), and the 64 chunks whose rccdfs output holds the longest runs of 0xFF bytes: encode parity, one round trip"""
    torch = torch_cuda
    cases = [c for c in gold["cases"] if c["nchunks"] > 200 or c["input"] == "search"]
    assert [c["nchunks"] for c in cases] == [16448, 8256, 64]
    for case in cases:
        dc = trc.DeviceCoder(codec, case["n"], case["chunk"], "cuda:0")
        checked("roundtrip", torch, dc, case, codec, inputs(case))


def _encode(torch, dc, d, n):
    """-> (clen, payload on the host, clones of both on the device)"""
    dc.payload.fill_(0x5A)
    dc.encode(to_dev(torch, d), n)
    clen, payload = dc.result(n)
    return clen, payload, dc.clen.clone(), dc.payload.clone()


@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_tables_ready(torch_cuda, codec):
    """one CDF, many buffers: trc_tables_dev once per CDF, then three different inputs of that CDF encoded and decoded with
    TRC_TABLES_READY.  Lengths and payloads equal those of the calls without the flag, byte for byte."""
    torch = torch_cuda
    for chunk in (256, 512, 4096):
        nmax = 65 * chunk
        flagged = trc.DeviceCoder(codec, nmax, chunk, "cuda:0")
        plain = trc.DeviceCoder(codec, nmax, chunk, "cuda:0")
        for name in S.CDFS:
            cdf, cdfnum = S.cdf(name)
            flagged.set_cdf(cdf, cdfnum)                          # trc_tables_dev: every call below carries TRC_TABLES_READY
            assert flagged.tables_ready == trc.TABLES_READY
            plain.set_cdf(cdf, cdfnum)
            plain.tables_ready = 0                                # ... and none of these does
            for n in (nmax, nmax - S.RAGGED_CUT):
                held = []
                for inp in ("mixed", "same:p38", "same:last"):
                    d = S.build_input(S.make_case(name, inp, chunk, 65, n))
                    a = _encode(torch, flagged, d, n)
                    b = _encode(torch, plain, d, n)
                    tag = (S.NAMES[codec], name, inp, chunk, n)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), tag
                    held.append((d, a[2], a[3], tag))
                for d, d_clen, d_pay, tag in held:
                    for dc in (flagged, plain):
                        G.decode_checked(torch, dc, d, n, 0xA5, "%s (tables_ready = %#x)" % (tag, dc.tables_ready), clen=d_clen, payload=d_pay)


@pytest.mark.parametrize("name", ("rare_top", "two_hi", "nib", "one"))
@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_ranges(torch_cuda, gold, inputs, codec, name):
    """trc_decode_range_dev on the mixed 200-chunk ragged cases: slices of the input, 0xA5 behind them, without and with
    TRC_DIR_READY"""
    torch = torch_cuda
    cases = [c for c in gold["cases"] if c["cdf"] == name and c["input"] == "mixed" and c["nchunks"] == 200 and c["n"] % c["chunk"]]
    assert [c["chunk"] for c in cases] == [256, 512]
    for case in cases:
        n, chunk, d = case["n"], case["chunk"], inputs(case)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        G.encode_checked(torch, dc, to_dev(torch, d), n, case[S.NAMES[codec]], case["name"], diagnose(codec, d, case), cdf=S.cdf(name))
        d_out = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda:0")
        for dir_ready, ranges in ((False, RANGES), (True, RANGES[::-1])):
            for first, count in ranges:
                nb = min(n, (first + count) * chunk) - first * chunk
                d_out.fill_(0xA5)
                dc.decode_range(d_out, first, count, n, dir_ready=dir_ready)
                torch.cuda.synchronize()
                out = d_out.cpu().numpy()
                tag = (S.NAMES[codec], case["name"], first, count, dir_ready)
                assert np.array_equal(out[:nb], d[first * chunk:first * chunk + nb]), tag
                assert (out[nb:] == 0xA5).all(), tag + ("guard",)


CHILD = textwrap.dedent("""
    import sys, numpy as np, torch
    sys.path[:0] = [%r, %r]
    import trc, gpu_contracts as G, static_cdf_lib as S
    import test_gpu_static_cdf as me
    gold = S.load()
    done = 0
    for case in gold["cases"]:
        if case["cdf"] in me.FORM_CDFS and case["input"] == "mixed" and case["nchunks"] in (65, 200):
            d = S.build_input(case)
            for codec in S.CODECS:
                dc = trc.DeviceCoder(codec, case["n"], case["chunk"], "cuda:0")
                me.checked("roundtrip", torch, dc, case, codec, d)
                done += 1
    print("ok", done)
""") % (os.path.dirname(os.path.abspath(trc.__file__)), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", FORMS, ids=("twelve_waves", "small"))
def test_workgroup_forms(torch_cuda, form):
    """the twelve-wave encoders and the small forms (the switches are read once per process: a child for each) on the mixed
    65- and 200-chunk cases of five CDFs, all four coders: encode parity and one round trip"""
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300, env=dict(os.environ, **form))
    want = "ok %d" % (len(FORM_CDFS) * 10 * len(S.CODECS))
    assert r.returncode == 0 and want in r.stdout, (form, r.stdout[-2000:] + r.stderr[-3000:])


def _small_alphabet_inputs():
    two = np.zeros(40000, dtype=np.uint8)
    two[23456] = 1
    return [("zeros", np.zeros(5000, dtype=np.uint8), 1), ("one_in_40000", two, 2), ("nibbles", T.nibble_bytes(5000, 21, "geo"), 16)]


@pytest.mark.parametrize("which", (0, 1, 2), ids=("cdfnum1", "cdfnum2", "cdfnum16"))
def test_device_cdfini_small_alphabets(torch_cuda, which):
    """trc_cdfini_dev and the host-pointer cdfini at alphabets of 1, 2 and 16 symbols: status and CDF equal the oracle's; then the
    encode / decode contracts of every coder under that CDF, against the oracle's encode"""
    torch = torch_cuda
    tag, d, cdfnum = _small_alphabet_inputs()[which]
    n, chunk = d.size, 256
    r0, cdf0, _ = T.orc_cdfini(d, cdfnum)
    assert r0 == n and cdf0[cdfnum] == 32768
    r1, cdf1, _ = trc.host_cdfini(d, cdfnum)
    assert r1 == r0 and np.array_equal(cdf1, cdf0), tag
    d_in = to_dev(torch, d)
    for codec in S.CODECS:
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.cdf.fill_(0x5A5A)
        dc.cdfini(d_in, n, cdfnum)
        torch.cuda.synchronize()
        got = dc.cdf[:cdfnum + 1].cpu().numpy().view(np.uint16)
        assert int(dc.status[0].item()) == r0 and np.array_equal(got, cdf0[:cdfnum + 1]), (tag, S.NAMES[codec])
        pay, clen, _ = T.orc_chunked_enc(codec, d, chunk, cdf0, cdfnum)
        ent = dict(nchunks=int(clen.size), payload_bytes=int(pay.size), clen_sha256=G.sha(clen.astype("<u4")), payload_sha256=G.sha(pay))
        G.contracts(torch, dc, d, d_in, ent, "%s %s" % (S.NAMES[codec], tag), cdf=(cdf0, cdfnum))


@pytest.mark.parametrize("name", ("rare_top", "nib", "one"))
@pytest.mark.parametrize("codec", S.CODECS, **CODEC_IDS)
def test_host_pointers(torch_cuda, gold, inputs, codec, name):
    """the reference-named host-pointer calls under a caller-made CDF, alphabets of 16 and of 1 symbol included: the container's
    directory and payload are the fixture's, the round trip and two ranges are exact"""
    case = [c for c in gold["cases"] if c["name"] == "%s/mixed/256/200/%d" % (name, 200 * 256)][0]
    e, d, n = case[S.NAMES[codec]], inputs(case), case["n"]
    cdf, cdfnum = S.cdf(name)
    lib = trc.lib()
    prev = lib.trc_get_chunk()
    assert lib.trc_set_chunk(256) == 0
    try:
        comp = trc.host_encode(codec, d, cdf, cdfnum)
        hdr, clen, payload = trc.parse_container(comp)
        assert hdr["chunk"] == 256 and hdr["n"] == n and hdr["nchunks"] == 200 and hdr["cdfnum"] == cdfnum and hdr["codec"] == codec
        assert payload.size == e["payload_bytes"] and G.sha(clen.astype("<u4")) == e["clen_sha256"] and G.sha(payload) == e["payload_sha256"], \
            diagnose(codec, d, case)(clen, payload)
        assert comp.size == 32 + 4 * clen.size + payload.size
        assert np.array_equal(trc.host_decode(codec, comp, n, cdf, cdfnum), d)
        for off, ln in ((255, 2), (63 * 256 + 17, 70 * 256)):
            assert np.array_equal(trc.host_decode_range(codec, comp, n, off, ln, cdf, cdfnum), d[off:off + ln]), (off, ln)
    finally:
        lib.trc_set_chunk(prev)
