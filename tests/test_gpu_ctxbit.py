"""Bitwise order-1 range coders on the MI355X (rccs / rcxs: TRC_RCC1 / TRC_RCX1): device-resident encode bit-exact to the
fixtures generated through the reference (tests/golden/make_ctxbit_golden.py), the decoder on the fixtures' payloads, the 100 MB
hashes at the round chunk, the host-pointer layer and malformed arguments."""
import json
import os

import numpy as np
import pytest

import trc
import ctxbit_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
CODECS = [L.RCC1, L.RCX1]


@pytest.fixture(scope="module")
def vectors():
    return G.vectors("ctxbit")


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: L.NAMES[c])
def test_fixtures_encode_and_decode(torch_cuda, vectors, codec):
    torch = torch_cuda
    z, index = vectors
    name = L.NAMES[codec]
    raw_seen = coded_seen = 0
    for ent in index:
        k, n, chunk = ent["case"], ent["n"], ent["chunk"]
        d = L.gen(ent["kind"], n, ent["seed"])                 # (inputs are regenerated, not stored)
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
    assert raw_seen > 20 and coded_seen > 80                  # both kinds of chunk, mixed containers among them


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, codec):
    torch = torch_cuda
    with open(os.path.join(GOLD, "ctxbit_large.json")) as f:
        large = [e for e in json.load(f) if e["codec"] == L.NAMES[codec]]
    assert len(large) == 2
    for e in large:
        n, chunk = e["n"], e["chunk"]
        assert trc.lib().trc_round_chunk(codec, n) == chunk
        G.large_roundtrip(torch, codec, L.gen(e["kind"], n, e["seed"]), e, tag=e["kind"])


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_layer(torch_cuda, codec):
    torch = torch_cuda
    lib = trc.lib()
    for kind, n in [("markov", 1), ("markov", 777), ("text", 16385), ("markov", 300001), ("runs", 1 << 20), ("uniform", 40000), ("markov", 3 * 10**6 + 7)]:
        d = L.gen(kind, n, 5 + n)
        for pinned in (False, True):
            if pinned:
                assert lib.trc_host_pin(d.ctypes.data, d.nbytes) == 0
            try:
                comp = trc.host_encode(codec, d)
            finally:
                if pinned:
                    lib.trc_host_unpin(d.ctypes.data)
            assert np.array_equal(trc.host_decode(codec, comp, n), d), (kind, n, pinned)
            if comp.size == n:
                continue                                       # raw: the whole input
            hdr, clen, payload = trc.parse_container(comp)
            assert hdr["codec"] == codec and hdr["chunk"] >= L.ROUND_CHUNK and hdr["n"] == n
            dc = trc.DeviceCoder(codec, n, hdr["chunk"], "cuda:0")
            dc.encode(to_dev(torch, d), n)
            dclen, dpay = dc.result(n)
            assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay), (kind, n, pinned)
    # two pipelines on one device: byte-identical containers
    d = L.gen("markov", 5 * 10**6 + 3, 3)
    one = trc.host_encode(codec, d)
    trc.set_devices([0, 0])
    try:
        two = trc.host_encode(codec, d)
        back = trc.host_decode(codec, two, d.size)
    finally:
        trc.set_devices([])
    assert np.array_equal(one, two)
    assert np.array_equal(back, d)


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: L.NAMES[c])
def test_malformed_arguments_like_rcs(torch_cuda, codec):
    """every bad call is refused with the code TRC_RCB's is refused with"""
    # (and a container of another coder is refused by the host-pointer decoder)
    G.refused_like_rcb(torch_cuda, codec, 16384, L.gen("text", 50000, 1))
