"""Bitwise word coders on the MI355X (rcsenc16, rcsenc32, rccsenc32, rcc2senc32: TRC_RCW16 .. TRC_RCC2W32): device-resident
encode bit-exact to the fixtures generated through the reference (tests/golden/make_word_golden.py), the decoder on the
fixtures' payloads, the 100 MB and slots + 1 hashes (several rounds of model slots), the host-pointer layer, malformed
arguments, corrupt payloads and the reference harness."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import trc
import word_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    return G.vectors("word")


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_fixtures_encode_and_decode(torch_cuda, vectors, codec):
    torch = torch_cuda
    z, index = vectors
    name, es = L.NAMES[codec], L.ES[codec]
    raw_seen = coded_seen = expanded = 0
    for ent in index:
        k, n, chunk = ent["case"], ent["n"], ent["chunk"]
        d = L.gen(ent["kind"], es, n, ent["seed"])             # (inputs are regenerated, not stored)
        rclen, rpay = z["clen_%d_%s" % (k, name)], z["out_%d_%s" % (k, name)]
        eclen, epay, raised = L.expected(codec, d, chunk, rclen, rpay)
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        # the two raw exceptions, explicitly: a chunk shorter than one word, and rcs16's expanding chunks
        for i in np.nonzero(rclen > lens)[0]:
            assert lens[i] < es or codec == L.RCW16, (name, k, i)
            expanded += int(lens[i] >= es)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(to_dev(torch, d), n)
        clen, payload = dc.result(n)
        tag = (name, ent["kind"], n, chunk)
        assert np.array_equal(clen, eclen), tag
        assert np.array_equal(payload, epay), tag
        out, guards = G.decode_fixture(torch, codec, n, chunk, eclen, epay, front=512)
        assert np.array_equal(out, d) and guards, tag
        raw = int((eclen == lens).sum())
        raw_seen += raw
        coded_seen += int(eclen.size - raw)
    assert raw_seen > 20 and coded_seen > 60
    assert (expanded > 10) == (codec == L.RCW16)


def _large(torch, e, codec):
    d = L.gen(e["kind"], L.ES[codec], e["n"], e["seed"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    G.large_roundtrip(torch, codec, d, e, nchunks=True)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, codec):
    """100 MB at chunk 16384: 1 round (rcs16), 2 (rcs32, rccs32), 4 (rcc2s32) at a 4 GiB budget"""
    with open(os.path.join(GOLD, "word_large.json")) as f:
        (e,) = [e for e in json.load(f) if e["codec"] == L.NAMES[codec] and "case" not in e]
    if codec != L.RCW16:
        assert L.slots(codec, e["nchunks"]) < e["nchunks"]
    _large(torch_cuda, e, codec)


def test_slots_plus_one(torch_cuda):
    """rcc2s32 on slots + 1 chunks: the last round holds one chunk (a short one)"""
    with open(os.path.join(GOLD, "word_large.json")) as f:
        (e,) = [e for e in json.load(f) if e.get("case") == "slots+1"]
    assert e["nchunks"] == L.slots(L.RCC2W32, e["nchunks"]) + 1
    _large(torch_cuda, e, L.RCC2W32)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_layer(torch_cuda, codec):
    torch = torch_cuda
    es = L.ES[codec]
    lib = trc.lib()
    prev = lib.trc_get_chunk()
    try:
        for chunk in (0, 16384, 32768):
            lib.trc_set_chunk(chunk)
            for kind, n in [("geo", 1), ("walk", 3), ("walk", 777), ("sine", 16385), ("stamps", 300001), ("uniform", 40000),
                            ("walk", 3 * 10**6 + 7)]:
                d = L.gen(kind, es, n, 5 + n)
                for pinned in (False, True):
                    src = torch.from_numpy(d).pin_memory().numpy() if pinned else d
                    comp = trc.host_encode(codec, src)
                    assert np.array_equal(trc.host_decode(codec, comp, n), d), (kind, n, chunk, pinned)
                if comp.size == n:
                    continue                                   # raw: the whole input
                hdr, clen, payload = trc.parse_container(comp)
                assert hdr["codec"] == codec and hdr["n"] == n
                assert hdr["chunk"] == max(chunk, 16384) if chunk else hdr["chunk"] >= 16384
                dc = trc.DeviceCoder(codec, n, hdr["chunk"], "cuda:0")
                dc.encode(to_dev(torch, d), n)
                dclen, dpay = dc.result(n)
                assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay), (kind, n, chunk)
    finally:
        lib.trc_set_chunk(prev)
    # a call of several slices (the host plan holds at most ~1 GiB of models per slice), and two pipelines on one device
    fc = (ctypes.c_size_t * 4096)()
    n = 40 * 10**6 + 3                                         # (rcs16: 1 GiB of models is 7680 chunks, one slice here)
    assert lib.trc_host_plan(codec, n, 0, 0, 0, fc, 4096, None) >= (1 if codec == L.RCW16 else 3)
    d = L.gen("walk", es, n, 3)
    one = trc.host_encode(codec, d)
    assert np.array_equal(trc.host_decode(codec, one, n), d)
    hdr, clen, payload = trc.parse_container(one)
    dc = trc.DeviceCoder(codec, n, hdr["chunk"], "cuda:0")
    dc.encode(to_dev(torch, d), n)
    dclen, dpay = dc.result(n)
    assert np.array_equal(clen, dclen) and np.array_equal(payload, dpay)
    trc.set_devices([0, 0])
    try:
        two = trc.host_encode(codec, d)
    finally:
        trc.set_devices([])
    assert np.array_equal(one, two)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_malformed_arguments_like_rcs(torch_cuda, codec):
    """every bad call is refused with the code TRC_RCB's is refused with"""
    G.refused_like_rcb(torch_cuda, codec, 4096, L.gen("geo", 2, 50000, 1), unknown=(42, 51))


def test_corrupt_payloads_stay_inside_the_output(torch_cuda):
    """forged payloads (flipped bytes, noise, truncated lengths): decoding completes and writes nothing outside the output"""
    torch = torch_cuda
    rng = np.random.Generator(np.random.PCG64(99))
    for codec in L.CODECS:
        n, chunk = 3 * 16384 + 1003, 16384
        d = L.gen("walk", L.ES[codec], n, 12)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(to_dev(torch, d), n)
        clen, payload = dc.result(n)
        variants = []
        p = payload.copy(); p[rng.integers(0, p.size, 64)] ^= 0xFF; variants.append((clen, p))
        p = rng.integers(0, 256, payload.size, dtype=np.uint8); variants.append((clen, p))
        c2 = np.minimum(clen, 9).astype(np.uint32)             # directory entries cut short: tiny chunks of noise
        variants.append((c2, rng.integers(0, 256, int(c2.sum()), dtype=np.uint8)))
        c3 = np.minimum(clen, 2).astype(np.uint32)             # shorter than the tail (3 bytes on the 32-bit coders)
        variants.append((c3, rng.integers(0, 256, int(c3.sum()), dtype=np.uint8)))
        for i, (cl, pay) in enumerate(variants):
            _, guards = G.decode_fixture(torch, codec, n, chunk, cl, pay, front=512)
            assert guards, (L.NAMES[codec], i)


def test_reference_harness_no_mismatch(torch_cuda, tmp_path):
    """the reference's own harness linked against the library: -e6,7,8 on a 16-bit file (-Os) and a 32-bit file (-Ou)"""
    for es, rows in ((2, ("6:rc-16",)), (4, ("6:rc-32", "7:rcc-32", "8:rcc2-32"))):
        src = tmp_path / ("walk%d.bin" % (8 * es))
        src.write_bytes(L.gen("walk", es, 3 * 10**6 + 2 * es, 4).tobytes())
        G.reference_harness(["-e6,7,8", "-Os" if es == 2 else "-Ou"], src, rows, 600)
