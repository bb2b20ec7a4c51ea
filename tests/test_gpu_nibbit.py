"""Bitwise nibble and varint byte coders on the MI355X (rc4s, rc4cs, rcu3s: TRC_RC4, TRC_RC4C, TRC_RCU3): device-resident
encode bit-exact to the fixtures generated through the reference (tests/golden/make_nibbit_golden.py), the decoder on the
fixtures' payloads, the 4 MiB hashes, a payload at an odd-word offset, the host-pointer layer, argument errors and trcbench."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import trc
import nibbit_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, ROOT, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    return G.vectors("nibbit")


@pytest.fixture(scope="module")
def large():
    """the 4 MiB input, made once and left unchanged, and the recorded hashes per coder"""
    with open(os.path.join(GOLD, "nibbit_large.json")) as f:
        rec = {e["codec"]: e for e in json.load(f)}
    e = rec["rc4s"]
    d = L.gen(e["kind"], e["n"], e["seed"], e["chunk"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    d.setflags(write=False)
    return d, rec


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_fixtures_encode_and_decode(torch_cuda, vectors, codec):
    torch = torch_cuda
    z, index = vectors
    name = L.NAMES[codec]
    raw_seen = coded_seen = 0
    for ent in index:
        k, n, chunk = ent["case"], ent["n"], ent["chunk"]
        d = L.gen(ent["kind"], n, ent["seed"], chunk)          # (inputs are regenerated, not stored)
        eclen, epay = z["clen_%d_%s" % (k, name)], z["out_%d_%s" % (k, name)]
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(to_dev(torch, d), n)
        clen, payload = dc.result(n)
        tag = (name, ent["kind"], n, chunk)
        assert np.array_equal(clen, eclen), tag
        assert np.array_equal(payload, epay), tag
        out, guards = G.decode_fixture(torch, codec, n, chunk, eclen, epay)   # the FIXTURE's directory and payload
        assert np.array_equal(out, L.expected(codec, d, eclen, chunk)) and guards, tag
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        raw = int((eclen == lens).sum())
        raw_seen += raw
        coded_seen += int(eclen.size - raw)
    assert raw_seen >= 1 and coded_seen >= 40


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, large, codec):
    """4 MiB of `mixed` at chunk 1024: 4096 chunks, 64 waves, raw and coded chunks side by side -- and once more with the
    payload buffer at an even offset that is no multiple of 16 (the alignment promise of include/trc_hip.h)"""
    torch = torch_cuda
    d, rec = large
    e = rec[L.NAMES[codec]]
    n, chunk = e["n"], e["chunk"]
    dc, d_in, clen, payload = G.large_roundtrip(torch, codec, d, e, raw_chunks=True, expected=L.expected, fill=0xA5)
    # payload at offset 6 of a 256-byte aligned buffer: encode into it, decode from it
    buf = torch.zeros(n + trc.PAD + 64 + 256, dtype=torch.uint8, device="cuda:0")
    base = (buf.data_ptr() + 255) & ~255
    shifted = buf[base - buf.data_ptr() + 6:]
    assert shifted.data_ptr() % 16 == 6
    dc.payload = shifted
    dc.encode(d_in, n)
    clen2, payload2 = dc.result(n)
    assert np.array_equal(clen2, clen) and np.array_equal(payload2, payload)
    G.decode_checked(torch, dc, L.expected(codec, d, clen, chunk), n, 0xA5, "payload at offset 6")


@pytest.mark.parametrize("chunk", [0, 256], ids=["auto", "chunk256"])
@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_round_trip(torch_cuda, codec, chunk):
    """rc4senc / rc4sdec, rc4csenc / rc4csdec, rcu3senc / rcu3sdec on 1 MB + 7 bytes, automatic chunk and 256"""
    lib = trc.lib()
    n = 10**6 + 7
    prev = lib.trc_get_chunk()
    assert lib.trc_set_chunk(chunk) == 0
    try:
        for kind in ("nib_skew", "bytes_small"):
            d = L.gen(kind, n, 11)
            comp = trc.host_encode(codec, d)
            assert comp.size < n, (kind, comp.size)
            assert lib.trc_container_check(comp.ctypes.data, comp.size, codec, n) == 0
            hdr, clen, payload = trc.parse_container(comp)
            assert hdr["codec"] == codec and hdr["n"] == n
            assert hdr["chunk"] == (chunk or lib.trc_auto_chunk_codec(codec, n))
            assert np.array_equal(trc.host_decode(codec, comp, n), L.expected(codec, d, clen, hdr["chunk"])), kind
    finally:
        lib.trc_set_chunk(prev)


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_argument_errors(torch_cuda, codec):
    """refused before anything is launched: a chunk that is no multiple of 64, a workspace one byte short"""
    torch = torch_cuda
    lib = trc.lib()
    n = 100000
    buf = torch.zeros(4 * n + (1 << 20), dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    wb = lib.trc_work_bytes(codec, n, 1024)
    assert wb > n
    work = torch.zeros(wb + 4096, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    TRC_E_ARG, TRC_E_WORK = -1, -3
    assert lib.trc_encode_dev(codec, p, n, 100, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None) == TRC_E_ARG
    assert lib.trc_decode_dev(codec, p + 2 * n, p + 3 * n, n, 100, None, 0, p, w, wb, None) == TRC_E_ARG
    assert lib.trc_encode_dev(codec, p, n, 1024, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb - 1, None) == TRC_E_WORK
    assert lib.trc_decode_dev(codec, p + 2 * n, p + 3 * n, n, 1024, None, 0, p, w, wb - 1, None) == TRC_E_WORK
    torch.cuda.synchronize()
    assert not buf.any().item()                                   # nothing ran


def test_trcbench_rows(torch_cuda):
    """harness/trcbench in a child process: -e40,41 on nibble input, -e17 on text; on text the two nibble rows are absent"""
    exe = os.path.join(ROOT, "harness", "trcbench")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    r = subprocess.run([exe, "-I1", "-e40,41", "--nibble", "1000003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and "failed" not in r.stdout, r.stdout + r.stderr
    assert "40:rc4cs" in r.stdout and "41:rc4s" in r.stdout, r.stdout
    r = subprocess.run([exe, "-I1", "-e17,40,41", "--text", "1000003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and "failed" not in r.stdout, r.stdout + r.stderr
    assert "17:rcu3s" in r.stdout and "40:" not in r.stdout and "41:" not in r.stdout, r.stdout


def test_reference_harness_no_mismatch(torch_cuda, tmp_path):
    """the reference's own harness linked against the library: -e17 on a byte file, -n -e40,41 on a nibble file"""
    for kind, args, rows in (("bytes_small", ["-e17"], ("17:rcu3",)), ("nib_skew", ["-n", "-e40,41"], ("40:rc4cs", "41:rc4s"))):
        src = tmp_path / (kind + ".bin")
        src.write_bytes(L.gen(kind, 10**6 + 11, 4).tobytes())
        G.reference_harness(args, src, rows, 300)
