"""The workspace contracts of a device-resident coder, checked against a hash fixture entry (tests/golden/sweep.json,
bytesweep.json): the device_roundtrip sequence of test_gpu_parity.py for the coders the oracle restatement does not cover.  Every
decode is compared byte for byte with guard bytes behind n; every encode with the fixture's hashes and 64 guard bytes behind the
payload.  prm: the parameter pair of an "ss" coder, handed to DeviceCoder.encode / decode only where given."""
import hashlib

import numpy as np

import trc


def to_dev(torch, a, pad=512):
    return torch.from_numpy(np.concatenate([a, np.zeros(pad, np.uint8)])).to("cuda:0")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _prm(prm):
    return {} if prm is None else {"prm": tuple(prm)}


def encode_checked(torch, dc, d_in, n, ent, tag, diagnose=None, prm=None):
    """encode into a payload filled with 0x5A: lengths, payload and total hash to the fixture's, the 64 bytes behind the
    total still hold 0x5A.  diagnose(clen, payload) -> str adds detail to a mismatch (it never decides)."""
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


def decode_checked(torch, dc, d, n, fill, tag, prm=None, **kw):
    """d: what the decoder must return (the input; for a nibble coder its low nibbles where the chunk is coded)"""
    kw.update(_prm(prm))
    d_out = torch.full((n + 512,), fill, dtype=torch.uint8, device="cuda:0")
    dc.decode(d_out, n, **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], d), "%s: decode mismatch, first byte %d" % (tag, int(np.nonzero(out[:n] != d)[0][0]))
    assert (out[n:] == fill).all(), "%s: the decoder wrote past n" % (tag,)


def roundtrip(torch, dc, d, d_in, ent, tag, diagnose=None, prm=None):
    """encode parity and one round trip"""
    n = d.size
    encode_checked(torch, dc, d_in, n, ent, tag + " encode", diagnose, prm)
    decode_checked(torch, dc, d, n, 0xA5, tag + " decode", prm)


def contracts(torch, dc, d, d_in, ent, tag, diagnose=None, prm=None):
    """encode; decode; decode under TRC_DIR_READY; encode again into the used workspace; decode under TRC_DIR_READY after that
    encode; a second coder whose workspace is 0xEE and has never encoded decodes the first one's directory and payload with
    TRC_DIR_READY off, on, on"""
    n = d.size
    encode_checked(torch, dc, d_in, n, ent, tag + " encode", diagnose, prm)
    decode_checked(torch, dc, d, n, 0xA5, tag + " decode", prm)
    decode_checked(torch, dc, d, n, 0x5A, tag + " decode with TRC_DIR_READY (after a decode)", prm, dir_ready=True)
    encode_checked(torch, dc, d_in, n, ent, tag + " second encode into the used workspace", diagnose, prm)
    decode_checked(torch, dc, d, n, 0x5A, tag + " decode with TRC_DIR_READY (after an encode)", prm, dir_ready=True)
    rx = trc.DeviceCoder(dc.codec, n, dc.chunk, "cuda:0")
    rx.work.fill_(0xEE)
    for flag in (False, True, True):
        decode_checked(torch, rx, d, n, 0x3C, tag + " decode-only workspace, dir_ready=%s" % flag, prm, clen=dc.clen, payload=dc.payload,
                       dir_ready=flag)
