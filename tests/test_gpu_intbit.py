"""Gamma / Rice integer coders on the MI355X (rcgs*, rcgzs*, rcrs*, rcrzs*: TRC_RCG8 .. TRC_RCRZ32): device-resident encode
bit-exact to the fixtures generated through the reference (tests/golden/make_intbit_golden.py), the decoder on the fixtures'
payloads, the 100 MB hashes, the host-pointer layer, malformed arguments and the reference harness."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import trc
import intbit_lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(GOLD, "intbit_vectors.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def to_dev(torch, a, pad=512):
    return torch.from_numpy(np.concatenate([a, np.zeros(pad, np.uint8)])).to("cuda:0")


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
        # the decoder from the FIXTURE's directory and payload, in a fresh workspace
        rx = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        d_clen = torch.from_numpy(np.concatenate([eclen, np.zeros(64, np.uint32)]).view(np.int32)).to("cuda:0")
        d_pay = to_dev(torch, epay)
        d_out = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rx.decode(d_out, n, clen=d_clen, payload=d_pay)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:n], d), tag
        assert (out[n:] == 0xA5).all(), tag
        lens = np.minimum(chunk, n - np.arange(0, n, chunk))
        raw = int((eclen == lens).sum())
        raw_seen += raw
        coded_seen += int(eclen.size - raw)
    assert raw_seen > 20 and coded_seen > 80


@pytest.mark.parametrize("codec", L.CODECS, ids=lambda c: L.NAMES[c])
def test_large_hashes(torch_cuda, codec):
    torch = torch_cuda
    with open(os.path.join(GOLD, "intbit_large.json")) as f:
        (e,) = [e for e in json.load(f) if e["codec"] == L.NAMES[codec]]
    n, chunk = e["n"], e["chunk"]
    d = L.gen(e["kind"], L.ES[codec], n, e["seed"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == e["in_sha256"]
    d_in = to_dev(torch, d)
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    dc.encode(d_in, n)
    clen, payload = dc.result(n)
    assert payload.size == e["payload_bytes"]
    assert hashlib.sha256(clen.astype("<u4").tobytes()).hexdigest() == e["clen_sha256"]
    assert hashlib.sha256(payload.tobytes()).hexdigest() == e["payload_sha256"]
    d_out = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
    dc.decode(d_out, n)
    torch.cuda.synchronize()
    assert torch.equal(d_out[:n], d_in[:n])


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
    lib.trc_host_plan.restype = ctypes.c_int
    lib.trc_host_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
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
    torch = torch_cuda
    lib = trc.lib()
    f = lib.trc_encode_dev
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    g = lib.trc_decode_dev
    g.restype = ctypes.c_int
    g.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n = 100000
    buf = torch.zeros(4 * n + (1 << 20), dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    wb = max(lib.trc_work_bytes(codec, n, 4096), lib.trc_work_bytes(trc.RCB, n, 4096))
    work = torch.zeros(wb + 4096, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    calls = [
        lambda c: f(c, p, n, 100, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),           # chunk not a multiple of 64
        lambda c: f(c, p, n, 1 << 20, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),       # chunk too large
        lambda c: f(c, p + 1, n, 4096, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),      # misaligned input
        lambda c: f(c, p, n, 4096, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, 1024, None),       # workspace too small
        lambda c: f(c, p, n, 4096, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w + 16, wb, None),    # misaligned workspace
        lambda c: g(c, p + 2 * n, p + 3 * n, n, 4096, None, 0, p + 1, w, wb, None),                 # misaligned output
        lambda c: g(c, p + 2 * n, p + 3 * n, n, 4096, None, 0, p, w, 1024, None),                   # workspace too small
    ]
    for i, call in enumerate(calls):
        want = call(trc.RCB)
        assert want < 0 and call(codec) == want, i
    torch.cuda.synchronize()
    d = L.gen("geo", 1, 50000, 1)
    comp = trc.host_encode(trc.RCB, d)
    assert comp.size < d.size
    with pytest.raises(trc.TrcError):
        trc.host_decode(codec, comp, d.size)


def test_reference_harness_no_mismatch(torch_cuda, tmp_path):
    """the reference's own harness linked against the library: -e26,27,28,29 on an 8-bit file, no mismatch reported"""
    exe = os.path.join(ROOT, "oracle", "_ref", "turborc_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/turborc_hip not built")
    src = tmp_path / "geo8.bin"
    src.write_bytes(L.gen("geo", 1, 3 * 10**6 + 11, 4).tobytes())
    r = subprocess.run([exe, "-I1", "-J1", "-e26,27,28,29", str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-2000:]
    for row in ("26:rcg-8", "27:rcgz-8", "28:rcr-8", "29:rcrz-8"):
        assert row in r.stdout, r.stdout[-3000:]
