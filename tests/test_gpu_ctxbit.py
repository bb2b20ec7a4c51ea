"""Bitwise order-1 range coders on the MI355X (rccs / rcxs: TRC_RCC1 / TRC_RCX1): device-resident encode bit-exact to the
fixtures generated through the reference (tests/golden/make_ctxbit_golden.py), the decoder on the fixtures' payloads, the 100 MB
hashes at the round chunk, the host-pointer layer and malformed arguments."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import trc
import ctxbit_lib as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODECS = [L.RCC1, L.RCX1]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(GOLD, "ctxbit_vectors.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def to_dev(torch, a, pad=512):
    return torch.from_numpy(np.concatenate([a, np.zeros(pad, np.uint8)])).to("cuda:0")


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
        d_in = to_dev(torch, L.gen(e["kind"], n, e["seed"]))
        dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        assert payload.size == e["payload_bytes"], e["kind"]
        assert hashlib.sha256(clen.astype("<u4").tobytes()).hexdigest() == e["clen_sha256"], e["kind"]
        assert hashlib.sha256(payload.tobytes()).hexdigest() == e["payload_sha256"], e["kind"]
        d_out = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
        dc.decode(d_out, n)
        torch.cuda.synchronize()
        assert torch.equal(d_out[:n], d_in[:n]), e["kind"]
        del dc, d_in, d_out


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: L.NAMES[c])
def test_host_pointer_layer(torch_cuda, codec):
    torch = torch_cuda
    lib = trc.lib()
    lib.trc_host_pin.restype = ctypes.c_int; lib.trc_host_pin.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.trc_host_unpin.restype = ctypes.c_int; lib.trc_host_unpin.argtypes = [ctypes.c_void_p]
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
    wb = max(lib.trc_work_bytes(codec, n, 16384), lib.trc_work_bytes(trc.RCB, n, 16384))
    work = torch.zeros(wb + 4096, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    calls = [
        lambda c: f(c, p, n, 100, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),           # chunk not a multiple of 64
        lambda c: f(c, p, n, 1 << 20, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),       # chunk too large
        lambda c: f(c, p + 1, n, 16384, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),     # misaligned input
        lambda c: f(c, p, n, 16384, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, 1024, None),      # workspace too small
        lambda c: f(c, p, n, 16384, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w + 16, wb, None),   # misaligned workspace
        lambda c: g(c, p + 2 * n, p + 3 * n, n, 16384, None, 0, p + 1, w, wb, None),                # misaligned output
        lambda c: g(c, p + 2 * n, p + 3 * n, n, 16384, None, 0, p, w, 1024, None),                  # workspace too small
    ]
    for i, call in enumerate(calls):
        want = call(trc.RCB)
        assert want < 0 and call(codec) == want, i
    torch.cuda.synchronize()
    # a container of another coder is refused by the host-pointer decoder
    d = L.gen("text", 50000, 1)
    comp = trc.host_encode(trc.RCB, d)
    assert comp.size < d.size
    with pytest.raises(trc.TrcError):
        trc.host_decode(codec, comp, d.size)
