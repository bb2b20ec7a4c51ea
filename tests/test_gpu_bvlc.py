"""Turbo-VLC coders on the bitwise range coder on the MI355X (rcvs*, rcvzs*, rcvgs*, rcvgzs*: TRC_RCBV16 .. TRC_RCBVGZ32):
device-resident encode bit-exact to the fixtures generated through the reference (tests/golden/make_bvlc_golden.py), the
decoder on the fixtures' payloads, the 100 MB hashes, the host-pointer layer, malformed arguments, corrupt payloads and the
reference harness."""
import hashlib
import json
import os

import numpy as np
import pytest

import trc
import bvlc_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    return G.vectors("bvlc")


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
        out, guards = G.decode_fixture(torch, codec, n, chunk, eclen, epay, front=512)   # the FIXTURE's directory and payload
        assert np.array_equal(out, d) and guards, tag
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        raw = int((eclen == lens).sum())
        raw_seen += raw
        coded_seen += int(eclen.size - raw)
    assert raw_seen > 20 and coded_seen > 80


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, codec):
    with open(os.path.join(GOLD, "bvlc_large.json")) as f:
        (e,) = [e for e in json.load(f) if e["codec"] == L.NAMES[codec]]
    d = L.gen(e["kind"], L.ES[codec], e["n"], e["seed"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    G.large_roundtrip(torch_cuda, codec, d, e)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_layer(torch_cuda, codec):
    torch = torch_cuda
    es = L.ES[codec]
    lib = trc.lib()
    prev = lib.trc_get_chunk()
    try:
        for chunk in (0, 1024, 16384):
            lib.trc_set_chunk(chunk)
            for kind, n in [("geo", 1), ("geo", 3), ("walk", 777), ("mixed", 16385), ("geo", 300001), ("uniform", 40000),
                            ("mixed", 3 * 10**6 + 7)]:
                d = L.gen(kind, es, n, 5 + n)
                comp = trc.host_encode(codec, d)
                assert np.array_equal(trc.host_decode(codec, comp, n), d), (kind, n, chunk)
                if comp.size == n:
                    continue                                   # raw: the whole input
                hdr, clen, payload = trc.parse_container(comp)
                assert hdr["codec"] == codec and hdr["n"] == n
                if codec in L.CTX:                             # the context coders never go below 16384 here
                    assert hdr["chunk"] == max(chunk, 16384) if chunk else hdr["chunk"] >= 16384
                elif chunk:
                    assert hdr["chunk"] == chunk
                dc = trc.DeviceCoder(codec, n, hdr["chunk"], "cuda:0")
                dc.encode(to_dev(torch, d), n)
                dclen, dpay = dc.result(n)
                assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay), (kind, n, chunk)
    finally:
        lib.trc_set_chunk(prev)
    # two pipelines on one device: byte-identical containers
    d = L.gen("walk", es, 5 * 10**6 + 3, 3)
    one = trc.host_encode(codec, d)
    trc.set_devices([0, 0])
    try:
        two = trc.host_encode(codec, d)
        back = trc.host_decode(codec, two, d.size)
    finally:
        trc.set_devices([])
    assert np.array_equal(one, two)
    assert np.array_equal(back, d)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_malformed_arguments_like_rcs(torch_cuda, codec):
    """every bad call is refused with the code TRC_RCB's is refused with"""
    G.refused_like_rcb(torch_cuda, codec, 4096, L.gen("geo", 2, 50000, 1), unknown=(42, 51))


def test_corrupt_payloads_stay_inside_the_output(torch_cuda):
    """forged payloads (flipped bytes, forged header totals and vb, truncated lengths): decoding completes and writes nothing
    outside the output (sentinel bytes around it)"""
    torch = torch_cuda
    rng = np.random.Generator(np.random.PCG64(99))
    for codec in L.CODECS:
        n, chunk = 3 * 16384 + 1001, 16384
        d = L.gen("mixed", L.ES[codec], n, 12)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(to_dev(torch, d), n)
        clen, payload = dc.result(n)
        starts = np.concatenate([[0], np.cumsum(clen)[:-1]]).astype(np.int64)
        variants = []
        p = payload.copy(); p[rng.integers(0, p.size, 64)] ^= 0xFF; variants.append((clen, p))
        p = payload.copy()
        for s in starts:
            p[s:s + 4] = np.frombuffer(np.uint32(rng.integers(0, 1 << 32)).tobytes(), np.uint8)   # forged total
            if codec == L.RCBV32:
                p[s + 4] = 0                                   # vb 0: every symbol >= 16 takes mantissa bits
        variants.append((clen, p))
        p = rng.integers(0, 256, payload.size, dtype=np.uint8); variants.append((clen, p))
        c2 = np.minimum(clen, 9).astype(np.uint32)             # directory entries cut short: tiny chunks of noise
        variants.append((c2, rng.integers(0, 256, int(c2.sum()), dtype=np.uint8)))
        for i, (cl, pay) in enumerate(variants):
            _, guards = G.decode_fixture(torch, codec, n, chunk, cl, pay, front=512)
            assert guards, (L.NAMES[codec], i)


def test_reference_harness_no_mismatch(torch_cuda, tmp_path):
    """the reference's own harness linked against the library: -e30,33,35,36 on a 16-bit file (-Os) and a 32-bit file (-Ou)"""
    for es, rows in ((2, ("30:rcv-16", "33:rcvz-16", "35:rcvg-16", "36:rcvgz-16")),
                     (4, ("30:rcv-32", "33:rcvz-32", "35:rcvg-32", "36:rcvgz-32"))):
        src = tmp_path / ("mixed%d.bin" % (8 * es))
        src.write_bytes(L.gen("mixed", es, 3 * 10**6 + 2 * es, 4).tobytes())
        G.reference_harness(["-e30,33,35,36", "-Os" if es == 2 else "-Ou"], src, rows, 600)
