"""The byte-level bitwise coders on the dual-rate "ss" predictor on the MI355X (rcss, rc4ss, rc4css, rcu3ss: TRC_RCSS,
TRC_RC4SS, TRC_RC4CSS, TRC_RCU3SS): device-resident encode bit-exact to the fixtures generated through the reference
(tests/golden/make_ssbit_golden.py) for every parameter pair, the decoder and the range decoder on the fixtures' payloads, the
4 MiB hashes, the host-pointer layer and its parameter rules, argument errors, trcbench and the reference's harness."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import trc
import ssbit_lib as L
import gpu_contracts as G
from gpu_contracts import GOLD, ROOT, to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
TRC_E_ARG, TRC_E_WORK = -1, -3


@pytest.fixture(scope="module")
def vectors():
    return L.load_fixtures(os.path.join(GOLD, "ssbit_vectors.npz"))


@pytest.fixture(scope="module")
def large():
    """the 4 MiB input, made once and left unchanged, and the recorded hashes per coder"""
    with open(os.path.join(GOLD, "ssbit_large.json")) as f:
        rec = {e["codec"]: e for e in json.load(f)}
    e = rec["rcss"]
    d = L.gen(e["kind"], e["n"], e["seed"], e["chunk"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    d.setflags(write=False)
    return d, rec


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_fixtures_encode_and_decode(torch_cuda, vectors, codec):
    """every case and parameter pair: the encoder gives the fixture's directory and payload; the decoder, from the FIXTURE's
    directory and payload in a workspace of its own, gives the input back; so does the range decoder on a mid-container range"""
    torch = torch_cuda
    z, index = vectors
    name = L.NAMES[codec]
    raw_seen = coded_seen = ranges = 0
    for ent in index:
        k, n, chunk = ent["case"], ent["n"], ent["chunk"]
        d = L.gen(ent["kind"], n, ent["seed"], chunk)          # (inputs are regenerated, not stored)
        d_in = to_dev(torch, d)
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        rx = trc.DeviceCoder(codec, n, chunk, "cuda:0")        # the range decoder's own workspace, never encoded in
        for prm in ent["prms"]:
            eclen, epay = L.fixture(z, ent, codec, prm)
            dc.encode(d_in, n, prm=prm)
            clen, payload = dc.result(n)
            tag = (name, ent["kind"], n, chunk, prm)
            assert np.array_equal(clen, eclen), tag
            assert np.array_equal(payload, epay), tag
            want = L.expected(codec, d, eclen, chunk)
            out, guards = G.decode_fixture(torch, codec, n, chunk, eclen, epay, prm=prm)
            assert np.array_equal(out, want) and guards, tag
            nch = eclen.size
            if nch >= 3:                                        # a range that starts and ends inside the container
                first, count = 1, nch - 2
                b0, b1 = first * chunk, min(n, (first + count) * chunk)
                d_clen, d_pay = G.fixture_to_dev(torch, eclen, epay)
                d_out = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
                rx.decode_range(d_out, first, count, n, clen=d_clen, payload=d_pay, prm=prm)
                torch.cuda.synchronize()
                out = d_out.cpu().numpy()
                assert np.array_equal(out[:b1 - b0], want[b0:b1]), tag
                assert (out[b1 - b0:] == 0xA5).all(), tag
                ranges += 1
            lens = np.minimum(chunk, n - np.arange(0, n, chunk))
            raw = int((eclen == lens).sum())
            raw_seen += raw
            coded_seen += int(eclen.size - raw)
    assert raw_seen >= 1 and coded_seen >= 40 and ranges >= 10


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, large, codec):
    """4 MiB of `mixed` at chunk 1024, parameters (5, 6): 4096 chunks, 64 waves, raw and coded chunks side by side"""
    d, rec = large
    e = rec[L.NAMES[codec]]
    G.large_roundtrip(torch_cuda, codec, d, e, prm=e["prm"], raw_chunks=True, expected=L.expected, fill=0xA5)


@pytest.mark.parametrize("prm", [(5, 6), (1, 9)], ids=["5_6", "1_9"])
@pytest.mark.parametrize("chunk", [0, 256], ids=["auto", "chunk256"])
@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_round_trip(torch_cuda, codec, chunk, prm):
    """the eight reference-named functions on 10^6 + 11 bytes, automatic chunk and 256; the header records the parameters, and a
    decoder that states other ones returns 0"""
    lib = trc.lib()
    n = 10**6 + 11
    prev = lib.trc_get_chunk()
    assert lib.trc_set_chunk(chunk) == 0
    try:
        for kind in ("nib_skew", "bytes_small"):
            d = L.gen(kind, n, 11)
            comp = trc.host_encode(codec, d, prm=prm)
            assert comp.size < n, (kind, comp.size)
            assert lib.trc_container_check(comp.ctypes.data, comp.size, codec, n) == 0
            hdr, clen, payload = trc.parse_container(comp)
            assert hdr["codec"] == codec and hdr["n"] == n and hdr["cdfnum"] == trc.ss_prm(prm)
            assert hdr["chunk"] == (chunk or lib.trc_auto_chunk_codec(codec, n))
            want = L.expected(codec, d, clen, hdr["chunk"])
            assert np.array_equal(trc.host_decode(codec, comp, n, prm=prm), want), kind
            assert np.array_equal(trc.host_decode_range(codec, comp, n, 70001, 3000), want[70001:73001]), kind
            other = (prm[0], prm[1] + 1)
            with pytest.raises(trc.TrcError):                       # argument / header mismatch: the decoder returns 0
                trc.host_decode(codec, comp, n, prm=other)
            with pytest.raises(trc.TrcError):
                trc.host_decode_range(codec, comp, n, 70001, 3000, prm=other)
    finally:
        lib.trc_set_chunk(prev)


def test_host_layer_parameter_rules(torch_cuda):
    """trc_encode_host / trc_decode_host: NULL CDF and TRC_SS_PRM; cdfnum 0 on decode = the header's parameters; a header whose
    parameters were altered fails against an explicit cdfnum that now disagrees, and decodes to something else without one"""
    lib = trc.lib()
    n, chunk, codec = 100003, 1024, trc.RCSS
    d = L.gen("bytes_small", n, 5)
    cap = lib.trc_container_bound(n, chunk)
    out = np.zeros(cap + 1024, np.uint8)
    cdf = np.zeros(260, np.uint16)
    for bad in (0, trc.ss_prm((0, 6)), trc.ss_prm((5, 16)), 5 | 6 << 8 | 1 << 16):
        assert lib.trc_encode_host(codec, d.ctypes.data, n, chunk, out.ctypes.data, cap, None, bad) == 0, bad
    assert lib.trc_encode_host(codec, d.ctypes.data, n, chunk, out.ctypes.data, cap, cdf.ctypes.data, trc.ss_prm((5, 6))) == 0
    l = lib.trc_encode_host(codec, d.ctypes.data, n, chunk, out.ctypes.data, cap, None, trc.ss_prm((4, 7)))
    assert 32 < l < n
    hdr, clen, payload = trc.parse_container(out[:l])
    assert hdr["cdfnum"] == trc.ss_prm((4, 7)) and hdr["chunk"] == chunk
    back = np.full(n + 64, 0xA5, np.uint8)
    for cdfnum in (0, trc.ss_prm((4, 7))):
        back.fill(0xA5)
        assert lib.trc_decode_host(codec, out.ctypes.data, l, back.ctypes.data, n, None, cdfnum) == n
        assert np.array_equal(back[:n], d) and (back[n:] == 0xA5).all()
    assert lib.trc_decode_host(codec, out.ctypes.data, l, back.ctypes.data, n, None, trc.ss_prm((5, 6))) == 0
    assert lib.trc_last_error()
    forged = out.copy()
    forged[6:8] = np.frombuffer(np.uint16(trc.ss_prm((5, 6))).tobytes(), np.uint8)      # the header's cdfnum field
    assert lib.trc_decode_host(codec, forged.ctypes.data, l, back.ctypes.data, n, None, trc.ss_prm((4, 7))) == 0
    assert lib.trc_last_error()
    forged[6:8] = np.frombuffer(np.uint16(trc.ss_prm((0, 7))).tobytes(), np.uint8)      # a parameter outside 1..15: no decode at all
    assert lib.trc_decode_host(codec, forged.ctypes.data, l, back.ctypes.data, n, None, 0) == 0


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_argument_errors(torch_cuda, codec):
    """refused before anything is launched: parameters 0 and 16, bits above the parameters, a CDF, a workspace one byte short"""
    torch = torch_cuda
    lib = trc.lib()
    n = 100000
    buf = torch.zeros(4 * n + (1 << 20), dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    wb = lib.trc_work_bytes(codec, n, 1024)
    rwb = lib.trc_range_work_bytes(codec, n, 1024, 10)
    assert wb > n and rwb > 0
    work = torch.zeros(wb + 4096, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    ok = trc.ss_prm((5, 6))
    enc = lambda cdf, cdfnum, nb=wb: lib.trc_encode_dev(codec, p, n, 1024, cdf, cdfnum, p + 2 * n, p + 3 * n, p + 4 * n, w, nb, None)
    dec = lambda cdf, cdfnum, nb=wb: lib.trc_decode_dev(codec, p + 2 * n, p + 3 * n, n, 1024, cdf, cdfnum, p, w, nb, None)
    rng = lambda cdf, cdfnum, nb=rwb: lib.trc_decode_range_dev(codec, p + 2 * n, p + 3 * n, n, 1024, 3, 10, cdf, cdfnum, p, w, nb, None)
    for f in (enc, dec, rng):
        for bad in (0, trc.ss_prm((0, 6)), trc.ss_prm((5, 0)), trc.ss_prm((16, 6)), trc.ss_prm((5, 16)), ok | 1 << 16, ok | 0x80):
            assert f(None, bad) == TRC_E_ARG, bad
        assert f(p + n, ok) == TRC_E_ARG                          # a CDF
    assert enc(None, ok, wb - 1) == TRC_E_WORK and dec(None, ok, wb - 1) == TRC_E_WORK and rng(None, ok, rwb - 1) == TRC_E_WORK
    assert lib.trc_encode_dev(codec, p, n, 100, None, ok, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None) == TRC_E_ARG
    torch.cuda.synchronize()
    assert not buf.any().item() and not work.any().item()         # nothing ran


def test_trcbench_rows(torch_cuda):
    """harness/trcbench -p ss in a child process: -e1,17 on text, -e40,41 on nibble input; other ids print no row; without -p
    the rows are the "s" coders'"""
    exe = os.path.join(ROOT, "harness", "trcbench")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    r = subprocess.run([exe, "-I1", "-p", "ss", "-e1,17,40,41,46", "--text", "1000003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and "failed" not in r.stdout, r.stdout + r.stderr
    assert "1:rcss" in r.stdout and "17:rcu3ss" in r.stdout, r.stdout
    assert "40:" not in r.stdout and "41:" not in r.stdout and "46:" not in r.stdout, r.stdout
    r = subprocess.run([exe, "-I1", "-p", "ss", "-r", "47", "-e40,41", "--nibble", "1000003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and "failed" not in r.stdout, r.stdout + r.stderr
    assert "40:rc4css" in r.stdout and "41:rc4ss" in r.stdout, r.stdout
    r = subprocess.run([exe, "-I1", "-e1,17", "--text", "1000003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "1:rc o0" in r.stdout and "17:rcu3s " in r.stdout and "rcss" not in r.stdout, r.stdout + r.stderr


def test_reference_harness_no_error(torch_cuda, tmp_path):
    """the reference's own harness linked against the library, started with -pss: ids 1 and 17 on a 1 MB file"""
    src = tmp_path / "bytes_small.bin"
    src.write_bytes(L.gen("bytes_small", 10**6 + 11, 4).tobytes())
    G.reference_harness(["-e1,17", "-pss"], src, ("1:rc", "17:rcu3"), 300)
