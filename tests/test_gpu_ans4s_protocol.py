"""The static rANS encoder's drain rule (csrc/trc_io.h, StreamOut with G > 0: a non-final drain runs a round only when it is FULL --
16 lanes hold a segment -- or some lane is URGENT) against the oracle, on data chosen to reach every branch of the rule:

  text     about 10 lanes of a wave fill a segment per 16-symbol piece: rounds are put off until 16 lanes have one
  quiet    one repeated byte (the space, the most frequent one) under a CDF made from text: 2.5 bits per symbol, and every lane of
           a wave fills its segment behind the same piece -- nothing for a dozen calls, then 64 lanes ready at once
  silent   the frequent symbol of the CDF below only: nothing but the two states is emitted, no non-final round runs and the
           final drain does all the work
  hot      a CDF that gives 255 symbols f = 1; three chunks of four are made of those symbols only (15 bits per symbol: far more
           than 16 lanes are ready behind every piece, the urgent test fires, the chunks overflow and are stored raw), every
           fourth one three eighths of them and the frequent symbol (5.6 bits per symbol: it stays coded, and its rounds are checked)
  islands  the same CDF; every fifth lane of a wave is such a chunk (all-rare and three-eighths-rare in turn), the others hold the frequent
           symbol only: at most 13 lanes of a wave ever have a segment, so every round that runs before the end is an urgent one
  uniform  random bytes under the CDF of a megabyte of them: every chunk is stored raw

for chunk 256 and 512, 1 / 17 / 64 / 65 / 200 chunks (a partial wave, exactly one, one and a lane, several), whole last chunks and a
ragged one (its length no multiple of 4 or of 64), in each workgroup shape of the encoder (TRC_ENC_WPB = 1 / 4 / 12, read once per
process: a fresh child for each).  Expected lengths and payloads are the oracle's encode of every chunk, computed once here and
handed to the children in a file; the children compare the device's directory and payload with it byte for byte and decode.
The other three static coders and the other CDF shapes (frequent symbol at the top, small alphabets): tests/test_gpu_static_cdf.py."""
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
KINDS = ("text", "quiet", "silent", "hot", "islands", "uniform")
RAGGED_CUT = 101                     # the ragged last chunk is this much short: 155 / 411 bytes, = 3 mod 4, no multiple of 64


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
        d = T.text_bytes(n, seed)
        return d, cdfs["text"]
    if kind == "quiet":
        return np.full(n, ord(" "), dtype=np.uint8), cdfs["text"]
    if kind == "silent":
        return np.zeros(n, dtype=np.uint8), cdfs["rare"]
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8), cdfs["flat"]
    rare = rng.integers(1, 256, nch * chunk, dtype=np.uint8).reshape(nch, chunk)
    part = np.where(rng.integers(0, 8, (nch, chunk)) < 3, rare, 0).astype(np.uint8)
    c = np.arange(nch)
    if kind == "hot":
        d = np.where((c % 4 == 3)[:, None], part, rare)
    else:                            # islands
        lane = c % 64
        d = np.where((lane % 5 == 0)[:, None], np.where(((lane // 5) % 2 == 0)[:, None], rare, part), 0)
    return np.ascontiguousarray(d.astype(np.uint8).reshape(-1)[:n]), cdfs["rare"]


def _expected(d, chunk, cdf):
    """the oracle's encode of every chunk, one call each -> (clen, payload)"""
    parts = [T.orc_enc(T.ANS4S, d[o:o + chunk], cdf, 256) for o in range(0, d.size, chunk)]
    return np.array([p.size for p in parts], dtype=np.uint32), np.concatenate(parts)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs, CDFs and the oracle's results of every case, written once for the three children"""
    cdfs = {"text": _cdf_of(T.text_bytes(1 << 20, 3)), "rare": _rare_cdf(),
            "flat": _cdf_of(np.random.default_rng(5).integers(0, 256, 1 << 20, dtype=np.uint8))}
    arrays, names, seed = {}, [], 100
    for chunk in CHUNKS:
        for nch in NCHUNKS:
            for n in (nch * chunk, nch * chunk - RAGGED_CUT):
                for kind in KINDS:
                    seed += 1
                    d, (cdf, cdfnum) = _make(kind, n, chunk, seed, cdfs)
                    assert cdfnum == 256 and d.size == n and (n == nch * chunk or (n % 4 and n % 64))
                    clen, payload = _expected(d, chunk, cdf)
                    name = "%s-%d-%d-%d" % (kind, chunk, nch, n)
                    names.append(name)
                    for k, v in (("d", d), ("cdf", cdf), ("clen", clen), ("payload", payload)):
                        arrays[name + "/" + k] = v
                    # the data does what it is here for
                    lens = np.minimum(chunk, n - chunk * np.arange(clen.size))
                    raw = clen == lens
                    if kind == "uniform":
                        assert raw.all(), name
                    if kind in ("text", "quiet", "silent"):
                        assert not raw[:-1].any(), name
                    if kind == "silent":
                        assert (clen[lens > 10] <= 10).all(), name
                    if kind == "hot" and nch >= 17:
                        assert raw[np.arange(clen.size) % 4 != 3][:-1].all() and not raw[3::4][:-1].any(), name
                    if kind == "islands" and nch >= 17:
                        assert raw[0::10][:1].all() and not raw[5::320].any(), name
    path = str(tmp_path_factory.mktemp("ans4s_protocol") / "cases.npz")
    np.savez(path, names=np.array(names), **arrays)
    return path


CHILD = textwrap.dedent("""
    import sys, numpy as np, torch
    sys.path[:0] = [%r, %r]
    import trc, trc_testlib as T
    z = np.load(sys.argv[1])
    for name in z["names"]:
        name = str(name)
        kind, chunk, nch, n = name.split("-")
        chunk, n = int(chunk), int(n)
        d, cdf = z[name + "/d"], z[name + "/cdf"]
        dc = trc.DeviceCoder(trc.ANS4S, n, chunk, "cuda:0")
        dc.set_cdf(cdf, 256)
        d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        assert np.array_equal(clen, z[name + "/clen"]), ("clen", name, np.flatnonzero(clen != z[name + "/clen"])[:8])
        assert np.array_equal(payload, z[name + "/payload"]), ("payload", name)
        out = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
        dc.decode(out, n, dir_ready=True); torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:n], d) and (o[n:] == 0xA5).all(), ("roundtrip", name)
    print("ok", len(z["names"]))
""") % (os.path.dirname(os.path.abspath(trc.__file__)), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wpb", (1, 4, 12))
def test_drain_rule_matches_oracle(cases, wpb):
    r = subprocess.run([sys.executable, "-c", CHILD, cases], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TRC_ENC_WPB=str(wpb)))
    want = "ok %d" % (len(CHUNKS) * len(NCHUNKS) * 2 * len(KINDS))
    assert r.returncode == 0 and want in r.stdout, (wpb, r.stdout[-2000:] + r.stderr[-3000:])
