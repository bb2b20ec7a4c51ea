"""Gamma / Rice integer coders on the MI355X (rcgs*, rcgzs*, rcrs*, rcrzs*: TRC_RCG8 .. TRC_RCRZ32): device-resident encode
bit-exact to the fixtures generated through the reference (tests/golden/make_intbit_golden.py), the decoder on the fixtures'
payloads, the 100 MB hashes, the host-pointer layer, malformed arguments and the reference harness."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import trc
import intbit_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    return G.vectors("intbit")


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_fixtures_encode_and_decode(torch_cuda, vectors, codec):
    torch = torch_cuda
    z, index = vectors
    name, es = L.NAMES[codec], L.ES[codec]
    raw_seen = coded_seen = 0
    for ent in index:
        k, n, chunk = ent["case"], ent["n"], ent["chunk"]
        d = L.gen(ent["kind"], es, n, ent["seed"])             # (inputs are regenerated, not stored)
        eclen, epay = z["clen_%d_%s" % (k, name)], z["out_%d_%s" % (k, name)]
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(to_dev(torch, d), n)
        clen, payload = dc.result(n)
        tag = (name, ent["kind"], n, chunk)
        assert np.array_equal(clen, eclen), tag
        assert np.array_equal(payload, epay), tag
        out, guards = G.decode_fixture(torch, codec, n, chunk, eclen, epay)   # the FIXTURE's directory and payload
        assert np.array_equal(out, d) and guards, tag
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        raw = int((eclen == lens).sum())
        raw_seen += raw
        coded_seen += int(eclen.size - raw)
    assert raw_seen > 20 and coded_seen > 80


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, codec):
    with open(os.path.join(GOLD, "intbit_large.json")) as f:
        (e,) = [e for e in json.load(f) if e["codec"] == L.NAMES[codec]]
    d = L.gen(e["kind"], L.ES[codec], e["n"], e["seed"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    G.large_roundtrip(torch_cuda, codec, d, e)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_layer(torch_cuda, codec):
    torch = torch_cuda
    es = L.ES[codec]
    for kind, n in [("geo", 1), ("geo", 3), ("walk", 777), ("mixed", 16385), ("geo", 300001), ("uniform", 40000), ("mixed", 3 * 10**6 + 7)]:
        d = L.gen(kind, es, n, 5 + n)
        comp = trc.host_encode(codec, d)
        assert np.array_equal(trc.host_decode(codec, comp, n), d), (kind, n)
        if comp.size == n:
            continue                                           # raw: the whole input
        hdr, clen, payload = trc.parse_container(comp)
        assert hdr["codec"] == codec and hdr["n"] == n
        dc = trc.DeviceCoder(codec, n, hdr["chunk"], "cuda:0")
        dc.encode(to_dev(torch, d), n)
        dclen, dpay = dc.result(n)
        assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay), (kind, n)
    # a multi-slice call at chunk 1024 (the smallest such n of 2^k * 1000 * 1024 + 1 bytes), its last chunk one byte
    lib = trc.lib()
    fc = (ctypes.c_size_t * 4097)()
    n = 31250 * 1024 + 1
    while lib.trc_host_plan(codec, n, 1024, 0, 0, fc, 4097, None) < 2:
        n = 2 * (n - 1) + 1
        assert n < (1 << 29)
    d = L.gen("mixed", es, n, 9)
    prev = trc.lib().trc_get_chunk()
    trc.lib().trc_set_chunk(1024)
    try:
        comp = trc.host_encode(codec, d)
    finally:
        trc.lib().trc_set_chunk(prev)
    hdr, clen, payload = trc.parse_container(comp)
    assert hdr["chunk"] == 1024 and clen[-1] == 1
    assert np.array_equal(trc.host_decode(codec, comp, n), d)
    dc = trc.DeviceCoder(codec, n, 1024, "cuda:0")
    dc.encode(to_dev(torch, d), n)
    dclen, dpay = dc.result(n)
    assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_malformed_arguments_like_rcs(torch_cuda, codec):
    """every bad call is refused with the code TRC_RCB's is refused with"""
    G.refused_like_rcb(torch_cuda, codec, 4096, L.gen("geo", 1, 50000, 1))


def test_reference_harness_no_mismatch(torch_cuda, tmp_path):
    """the reference's own harness linked against the library: -e26,27,28,29 on an 8-bit file, no mismatch reported"""
    src = tmp_path / "geo8.bin"
    src.write_bytes(L.gen("geo", 1, 3 * 10**6 + 11, 4).tobytes())
    G.reference_harness(["-e26,27,28,29"], src, ("26:rcg-8", "27:rcgz-8", "28:rcr-8", "29:rcrz-8"), 600)
