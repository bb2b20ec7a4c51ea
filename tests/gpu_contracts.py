"""The workspace contracts of a device-resident coder, checked against a hash fixture entry (tests/golden/sweep.json,
bytesweep.json): the device_roundtrip sequence of test_gpu_parity.py for the coders the oracle restatement does not cover.  Every
decode is compared byte for byte with guard bytes behind n; every encode with the fixture's hashes and 64 guard bytes behind the
payload.  prm: the parameter pair of an "ss" coder, handed to DeviceCoder.encode / decode only where given.  cdf: (uint16 array,
cdfnum) of a static coder, set on the coder under test (DeviceCoder.set_cdf) before anything runs and on the decode-only receiver.

Below them, what the test_gpu_<family>.py files share: the torch_cuda fixture (imported by name), the vectors loader,
decode_fixture, large_roundtrip, refused_like_rcb and reference_harness."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import trc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_HARNESS = os.path.join(ROOT, "oracle", "_ref", "turborc_hip")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def vectors(name):
    """-> (arrays, index) of tests/golden/<name>_vectors.npz"""
    z = np.load(os.path.join(GOLD, name + "_vectors.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def to_dev(torch, a, pad=512):
    return torch.from_numpy(np.concatenate([a, np.zeros(pad, np.uint8)])).to("cuda:0")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _prm(prm):
    return {} if prm is None else {"prm": tuple(prm)}


def _set_cdf(dc, cdf):
    if cdf is not None:
        dc.set_cdf(cdf[0], cdf[1])


def encode_checked(torch, dc, d_in, n, ent, tag, diagnose=None, prm=None, cdf=None):
    """encode into a payload filled with 0x5A: lengths, payload and total hash to the fixture's, the 64 bytes behind the
    total still hold 0x5A.  diagnose(clen, payload) -> str adds detail to a mismatch (it never decides)."""
    _set_cdf(dc, cdf)
    dc.payload.fill_(0x5A)
    dc.total.fill_(-1)
    dc.encode(d_in, n, **_prm(prm))
    clen, payload = dc.result(n)
    ok = (clen.size == ent["nchunks"] and payload.size == ent["payload_bytes"] and sha(clen.astype("<u4")) == ent["clen_sha256"]
          and sha(payload) == ent["payload_sha256"])
    if not ok:
        raise AssertionError("%s: lengths / payload differ from the reference (%d bytes, fixture %d)%s"
                             % (tag, payload.size, ent["payload_bytes"], "\n" + diagnose(clen, payload) if diagnose else ""))
    behind = dc.payload[payload.size:payload.size + 64].cpu().numpy()
    assert (behind == 0x5A).all(), "%s: the encoder wrote past the payload" % (tag,)
    return clen, payload


def decode_checked(torch, dc, d, n, fill, tag, prm=None, cdf=None, **kw):
    """d: what the decoder must return (the input; for a nibble coder its low nibbles where the chunk is coded)"""
    _set_cdf(dc, cdf)
    kw.update(_prm(prm))
    d_out = torch.full((n + 512,), fill, dtype=torch.uint8, device="cuda:0")
    dc.decode(d_out, n, **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], d), "%s: decode mismatch, first byte %d" % (tag, int(np.nonzero(out[:n] != d)[0][0]))
    assert (out[n:] == fill).all(), "%s: the decoder wrote past n" % (tag,)


def roundtrip(torch, dc, d, d_in, ent, tag, diagnose=None, prm=None, cdf=None):
    """encode parity and one round trip"""
    n = d.size
    _set_cdf(dc, cdf)
    encode_checked(torch, dc, d_in, n, ent, tag + " encode", diagnose, prm)
    decode_checked(torch, dc, d, n, 0xA5, tag + " decode", prm)


def contracts(torch, dc, d, d_in, ent, tag, diagnose=None, prm=None, cdf=None):
    """encode; decode; decode under TRC_DIR_READY; encode again into the used workspace; decode under TRC_DIR_READY after that
    encode; a second coder whose workspace is 0xEE and has never encoded decodes the first one's directory and payload with
    TRC_DIR_READY off, on, on"""
    n = d.size
    _set_cdf(dc, cdf)
    encode_checked(torch, dc, d_in, n, ent, tag + " encode", diagnose, prm)
    decode_checked(torch, dc, d, n, 0xA5, tag + " decode", prm)
    decode_checked(torch, dc, d, n, 0x5A, tag + " decode with TRC_DIR_READY (after a decode)", prm, dir_ready=True)
    encode_checked(torch, dc, d_in, n, ent, tag + " second encode into the used workspace", diagnose, prm)
    decode_checked(torch, dc, d, n, 0x5A, tag + " decode with TRC_DIR_READY (after an encode)", prm, dir_ready=True)
    rx = trc.DeviceCoder(dc.codec, n, dc.chunk, "cuda:0")
    rx.work.fill_(0xEE)
    _set_cdf(rx, cdf)
    for flag in (False, True, True):
        decode_checked(torch, rx, d, n, 0x3C, tag + " decode-only workspace, dir_ready=%s" % flag, prm, clen=dc.clen, payload=dc.payload,
                       dir_ready=flag)


def fixture_to_dev(torch, clen, payload, pad=512):
    """a directory with 64 zero entries behind it and a payload with `pad` zero bytes behind it, on the device"""
    d_clen = torch.from_numpy(np.concatenate([clen, np.zeros(64, np.uint32)]).view(np.int32)).to("cuda:0")
    return d_clen, to_dev(torch, payload, pad)


def decode_fixture(torch, codec, n, chunk, clen, payload, front=0, pad=512, prm=None):
    """decode (clen, payload) in a fresh workspace into an output with 512 bytes of 0xA5 behind it and `front` bytes of it in
    front -> (decoded bytes, guards intact)"""
    rx = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    d_clen, d_pay = fixture_to_dev(torch, clen, payload, pad)
    buf = torch.full((front + n + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    rx.decode(buf[front:], n, clen=d_clen, payload=d_pay, **_prm(prm))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[front:front + n], bool((out[:front] == 0xA5).all() and (out[front + n:] == 0xA5).all())


def large_roundtrip(torch, codec, d, e, tag=None, prm=None, nchunks=False, raw_chunks=False, expected=None, fill=None):
    """encode d at the chunk of the large-fixture entry e: payload size and the two hashes to e's; nchunks / raw_chunks: the
    directory's length / its number of raw chunks to e's as well.  Then decode: with fill None into zeros, compared with the
    input on the device; else into an output filled with `fill`, compared with expected(codec, d, clen, chunk) and the fill
    behind n intact.  -> (dc, d_in, clen, payload)"""
    n, chunk = e["n"], e["chunk"]
    d_in = to_dev(torch, d)
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    dc.encode(d_in, n, **_prm(prm))
    clen, payload = dc.result(n)
    if nchunks:
        assert clen.size == e["nchunks"], tag
    assert payload.size == e["payload_bytes"], tag
    if raw_chunks:
        assert int((clen == chunk).sum()) == e["raw_chunks"], tag
    assert sha(clen.astype("<u4")) == e["clen_sha256"], tag
    assert sha(payload) == e["payload_sha256"], tag
    if fill is None:
        d_out = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
        dc.decode(d_out, n, **_prm(prm))
        torch.cuda.synchronize()
        assert torch.equal(d_out[:n], d_in[:n]), tag
    else:
        decode_checked(torch, dc, expected(codec, d, clen, chunk), n, fill, tag, prm)
    return dc, d_in, clen, payload


def refused_like_rcb(torch, codec, chunk, d, unknown=()):
    """every bad call is refused with the code TRC_RCB's is refused with; the ids in `unknown` are refused; the host-pointer
    decoder refuses TRC_RCB's container of d"""
    lib = trc.lib()
    f, g = lib.trc_encode_dev, lib.trc_decode_dev
    n = 100000
    buf = torch.zeros(4 * n + (1 << 20), dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    wb = max(lib.trc_work_bytes(codec, n, chunk), lib.trc_work_bytes(trc.RCB, n, chunk))
    work = torch.zeros(wb + 4096, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    calls = [
        lambda c: f(c, p, n, 100, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),           # chunk not a multiple of 64
        lambda c: f(c, p, n, 1 << 20, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),       # chunk too large
        lambda c: f(c, p + 1, n, chunk, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None),     # misaligned input
        lambda c: f(c, p, n, chunk, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, 1024, None),       # workspace too small
        lambda c: f(c, p, n, chunk, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w + 16, wb, None),    # misaligned workspace
        lambda c: g(c, p + 2 * n, p + 3 * n, n, chunk, None, 0, p + 1, w, wb, None),                # misaligned output
        lambda c: g(c, p + 2 * n, p + 3 * n, n, chunk, None, 0, p, w, 1024, None),                  # workspace too small
    ]
    for i, call in enumerate(calls):
        want = call(trc.RCB)
        assert want < 0 and call(codec) == want, i
    for bad in unknown:
        assert f(bad, p, n, chunk, None, 0, p + 2 * n, p + 3 * n, p + 4 * n, w, wb, None) < 0
    torch.cuda.synchronize()
    comp = trc.host_encode(trc.RCB, d)
    assert comp.size < d.size
    with pytest.raises(trc.TrcError):
        trc.host_decode(codec, comp, d.size)


def reference_harness(args, src, rows, timeout, exe=REF_HARNESS):
    """the reference's own harness linked against the library, on the file src: exit 0, no ERROR, every row of `rows` printed"""
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/turborc_hip not built")
    r = subprocess.run([exe, "-I1", "-J1"] + list(args) + [str(src)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-2000:]
    for row in rows:
        assert row in r.stdout, r.stdout[-3000:]
