"""The static rANS decoder's stream reader (csrc/trc_io.h, LaneStreamIn: behind the first fill every lane refills its own ring, 16
bytes at a time, up to two pieces per 16-symbol period) on containers made by the oracle, on data chosen to reach every branch of it:

  text        about 10 bytes per period: one piece for two lanes of three, the second request's mask empty almost always
  quiet       one repeated byte (the space) under a CDF made from text: every lane asks at the same periods
  silent      the frequent symbol of the rare CDF only: nothing but the two states, lim = 0, no piece is ever requested
  uniform     random bytes under a flat CDF: every chunk is stored raw
  mixed       text with every third chunk random bytes: raw chunks among coded ones
  burst-head  the rare CDF (255 symbols at f = 1); the first 3/8 of each chunk are rare symbols, the rest the frequent one: 30
              bytes per period for 3/8 of the chunk, which one piece per period cannot feed -- the second request has to; the
              chunk stays coded (0.70 x its length + 8 bytes by arithmetic; asserted below from the oracle's lengths)
  burst-tail  the same with the rare symbols last: the second request at the end of the chunk, up against `lim`
  islands     the rare CDF; every fifth lane of a wave all-rare (stored raw) or three-eighths-rare, the others silent

for chunk 256 and 512, 1 / 17 / 64 / 65 / 200 chunks, whole last chunks and a ragged one (101 bytes short: 3 mod 4), with the
payload at every even offset 0 .. 14 of a 16-byte-aligned buffer whose first bytes they are (the first stream is then closer than
16 bytes to the start of the buffer and takes unaligned pieces), decoded with dir_ready false, then true, everything twice: the
bytes around the payload, the workspace and the output filled with 0xA5, then with 0x5A.  Small inputs would take the two-lane
decoder, so every child runs under TRC_ANS_PAIR=0, and in each workgroup shape (TRC_DEC_WPB = 1 / 4 / 12); both are read once per
process: a fresh child for each.  The containers are the oracle's encode of every chunk, computed once and handed over in a file."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import trc
import trc_testlib as T

pytestmark = pytest.mark.gpu

CHUNKS = (256, 512)
NCHUNKS = (1, 17, 64, 65, 200)
KINDS = ("text", "quiet", "silent", "uniform", "mixed", "burst-head", "burst-tail", "islands")
OFFSETS = tuple(range(0, 16, 2))
RAGGED_CUT = 101                     # the ragged last chunk is this much short: 155 / 411 bytes, = 3 mod 4


def _cdf_of(buf):
    _, cdf, cdfnum = T.orc_cdfini(buf, 256)
    return cdf, cdfnum


def _rare_cdf():
    """every byte value occurs, 255 of them once in a million: f = 1 for those"""
    model = np.zeros(1000000, dtype=np.uint8)
    model[:255] = np.arange(1, 256, dtype=np.uint8)
    cdf, cdfnum = _cdf_of(model)
    f = np.diff(cdf[:257].astype(np.int64))
    assert (f[1:] == 1).all() and f[0] == 32768 - 255, "the model buffer no longer gives f = 1"
    return cdf, cdfnum


def _make(kind, n, chunk, seed, cdfs):
    rng = np.random.default_rng(seed)
    nch = (n + chunk - 1) // chunk
    if kind == "text":
        return T.text_bytes(n, seed), cdfs["text"]
    if kind == "quiet":
        return np.full(n, ord(" "), dtype=np.uint8), cdfs["text"]
    if kind == "silent":
        return np.zeros(n, dtype=np.uint8), cdfs["rare"]
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8), cdfs["flat"]
    if kind == "mixed":
        d = T.text_bytes(nch * chunk, seed).reshape(nch, chunk)
        noise = rng.integers(0, 256, (nch, chunk), dtype=np.uint8)
        d = np.where((np.arange(nch) % 3 == 1)[:, None], noise, d)
        return np.ascontiguousarray(d.astype(np.uint8).reshape(-1)[:n]), cdfs["text"]
    rare = rng.integers(1, 256, nch * chunk, dtype=np.uint8).reshape(nch, chunk)
    if kind in ("burst-head", "burst-tail"):
        lens = np.minimum(chunk, n - chunk * np.arange(nch))
        k = (3 * lens // 8)[:, None]                           # rare symbols per chunk: 3/8 of ITS length
        pos = np.arange(chunk)[None, :]
        where = pos < k if kind == "burst-head" else (pos >= lens[:, None] - k) & (pos < lens[:, None])
        d = np.where(where, rare, 0)
        return np.ascontiguousarray(d.astype(np.uint8).reshape(-1)[:n]), cdfs["rare"]
    part = np.where(rng.integers(0, 8, (nch, chunk)) < 3, rare, 0).astype(np.uint8)        # islands
    lane = np.arange(nch) % 64
    d = np.where((lane % 5 == 0)[:, None], np.where(((lane // 5) % 2 == 0)[:, None], rare, part), 0)
    return np.ascontiguousarray(d.astype(np.uint8).reshape(-1)[:n]), cdfs["rare"]


def _expected(d, chunk, cdf):
    """the oracle's encode of every chunk, one call each -> (clen, payload)"""
    parts = [T.orc_enc(T.ANS4S, d[o:o + chunk], cdf, 256) for o in range(0, d.size, chunk)]
    return np.array([p.size for p in parts], dtype=np.uint32), np.concatenate(parts)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs, CDFs and the oracle's containers of every case, written once for the three children"""
    cdfs = {"text": _cdf_of(T.text_bytes(1 << 20, 3)), "rare": _rare_cdf(),
            "flat": _cdf_of(np.random.default_rng(5).integers(0, 256, 1 << 20, dtype=np.uint8))}
    arrays, names, seed = {}, [], 300
    for chunk in CHUNKS:
        for nch in NCHUNKS:
            for n in (nch * chunk, nch * chunk - RAGGED_CUT):
                for kind in KINDS:
                    seed += 1
                    d, (cdf, cdfnum) = _make(kind, n, chunk, seed, cdfs)
                    assert cdfnum == 256 and d.size == n and (n == nch * chunk or n % 4 == 3)
                    clen, payload = _expected(d, chunk, cdf)
                    name = "%s:%d:%d:%d" % (kind, chunk, nch, n)
                    names.append(name)
                    for k, v in (("d", d), ("cdf", cdf), ("clen", clen), ("payload", payload)):
                        arrays[name + "/" + k] = v
                    # the data does what it is here for
                    lens = np.minimum(chunk, n - chunk * np.arange(clen.size))
                    raw = clen == lens
                    if kind == "uniform":
                        assert raw.all(), name
                    if kind in ("text", "quiet", "silent"):
                        assert not raw.any(), name
                    if kind == "silent":
                        assert (clen <= 10).all(), name
                    if kind == "mixed":
                        assert raw[1::3].all() and not raw[0::3].any() and not raw[2::3].any(), name
                    if kind in ("burst-head", "burst-tail"):   # a condition, not a measurement: every burst chunk stays coded
                        assert (clen < lens).all(), (name, np.flatnonzero(clen >= lens)[:8])
                        assert (8 * (clen - 8) >= 14 * (3 * lens // 8)).all(), name      # ... and its burst is close to 15 bits a symbol
                    if kind == "islands" and nch >= 17:
                        assert raw[0::10][:1].all() and not raw[5::320].any(), name
    path = str(tmp_path_factory.mktemp("dec_lane_refill") / "cases.npz")
    np.savez(path, names=np.array(names), **arrays)
    return path


CHILD = textwrap.dedent("""
    import sys, numpy as np, torch
    sys.path[:0] = [%r, %r]
    import trc, trc_testlib as T
    z = np.load(sys.argv[1])
    offsets = [int(x) for x in sys.argv[2].split(",")]
    dev, runs = "cuda:0", 0
    for name in z["names"]:
        name = str(name)
        kind, chunk, nch, n = name.split(":")
        chunk, n = int(chunk), int(n)
        d, cdf, clen, payload = z[name + "/d"], z[name + "/cdf"], z[name + "/clen"], z[name + "/payload"]
        total = payload.size
        d_pay, d_clen = torch.from_numpy(payload).to(dev), torch.from_numpy(clen.view(np.int32)).to(dev)
        dc = trc.DeviceCoder(trc.ANS4S, n, chunk, dev)
        for off in offsets:
            outs = []
            for fill in (0xA5, 0x5A):
                buf = torch.full((off + total + trc.PAD + 64,), fill, dtype=torch.uint8, device=dev)     # 16-byte aligned and more
                assert buf.data_ptr() %% 16 == 0
                buf[off:off + total].copy_(d_pay)
                cl = torch.full((4 * (clen.size + 64),), fill, dtype=torch.uint8, device=dev).view(torch.int32)
                cl[:clen.size].copy_(d_clen)
                dc.work.fill_(fill)
                dc.set_cdf(cdf, 256)                            # the tables live in the workspace
                for ready in (False, True):
                    out = torch.full((n + 512,), fill, dtype=torch.uint8, device=dev)
                    dc.decode(out, n, clen=cl, payload=buf[off:], dir_ready=ready)
                    torch.cuda.synchronize()
                    o = out.cpu().numpy()
                    assert np.array_equal(o[:n], d), ("decode", name, off, hex(fill), ready, np.flatnonzero(o[:n] != d)[:8])
                    assert (o[n:] == fill).all(), ("behind the output", name, off, hex(fill), ready)
                    outs.append(o[:n])
                    runs += 1
                b = buf.cpu().numpy()
                assert (b[:off] == fill).all() and np.array_equal(b[off:off + total], payload) and (b[off + total:] == fill).all(), ("payload buffer", name)
            assert all(np.array_equal(outs[0], x) for x in outs[1:]), ("fills disagree", name, off)
    print("ok", runs)
""") % (os.path.dirname(os.path.abspath(trc.__file__)), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wpb", (1, 4, 12))
def test_lane_refill_decodes_oracle_containers(cases, wpb):
    r = subprocess.run([sys.executable, "-c", CHILD, cases, ",".join(str(o) for o in OFFSETS)], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, TRC_ANS_PAIR="0", TRC_DEC_WPB=str(wpb)))
    want = "ok %d" % (len(CHUNKS) * len(NCHUNKS) * 2 * len(KINDS) * len(OFFSETS) * 2 * 2)
    assert r.returncode == 0 and want in r.stdout, (wpb, r.stdout[-2000:] + r.stderr[-3000:])
