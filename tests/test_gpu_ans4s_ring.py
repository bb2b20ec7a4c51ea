"""The static rANS encoder's output ring (csrc/trc_io.h, StreamOut's layout parameter): where a lane's bytes wait inside LDS must not
show in what leaves.  tests/test_gpu_ans4s_protocol.py covers the branches of the drain RULE; this file covers what a ring LAYOUT
can get wrong -- a halfword of the wrong parity, a row of the wrong lane, the two groups of 32 lanes, a drain that reads a slot nobody
wrote -- at the smallest shapes that reach it:

  chunk sizes   256 and 512 (the ring revolves one to three times) and, on text, 4096 (about twenty revolutions: every row and both
                halfword parities are written many times)
  chunk counts  1, 31, 32, 33, 63, 64, 65, 130: lanes below and above 32, partial waves, more than one wave; each with a whole last
                chunk and with a ragged one (its length no multiple of 4 or of 64)
  staircase     the f = 1 CDF of the protocol test; chunk i starts with STEP * (i % 64) rare symbols (15 bits each) and goes on with
                the frequent one: when the lanes of a wave drain they sit at many different ring offsets of both parities (asserted
                below from the oracle's lengths)
  text          coded chunks, lanes ready a few at a time
  uniform       every chunk is stored raw: the ring is abandoned mid-way in every lane
  quiet         one repeated byte under the text CDF: 64 lanes ready at once

Expected lengths and payloads are the oracle's encode of every chunk, computed once on the CPU and handed to the children in a
file; every case runs twice, the workspace filled with 0xA5 and then with 0x5A before the encode (as tests/test_gpu_gather_lines.py
does), is compared byte for byte, decoded, and nothing behind the output's end may have been written.  One fresh child per
workgroup shape of the encoder (TRC_ENC_WPB = 1 / 4 / 12: the switch is read once per process)."""
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
NCHUNKS = (1, 31, 32, 33, 63, 64, 65, 130)
KINDS = ("staircase", "text", "uniform", "quiet")
BIG = (4096, (33, 65))               # chunk 4096, text only
RAGGED_CUT = 101                     # the ragged last chunk is this much short: = 3 mod 4, no multiple of 64 at any of the chunk sizes
# rare symbols per lane index in "staircase".  3 at chunk 512; at chunk 256 a step of 3 makes the lanes above 44 overflow (189 rare
# symbols are 354 bytes) and too few coded lanes are left for the assertion below; an even step gives even unit counts only (two
# symbols of 15 bits are two units, nearly always); so the step is 1 there
STEP = {256: 1, 512: 3}


def _cdf_of(buf):
    _, cdf, cdfnum = T.orc_cdfini(buf, 256)
    return cdf, cdfnum


def _rare_cdf():
    """every byte value occurs, 255 of them once in a million: f = 1 for those (the construction of test_gpu_ans4s_protocol.py)"""
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
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8), cdfs["flat"]
    rare = rng.integers(1, 256, (nch, chunk), dtype=np.uint8)
    head = STEP[chunk] * (np.arange(nch) % 64)
    d = np.where(np.arange(chunk)[None, :] < head[:, None], rare, 0).astype(np.uint8)
    return np.ascontiguousarray(d.reshape(-1)[:n]), cdfs["rare"]


def _expected(d, chunk, cdf):
    """the oracle's encode of every chunk, one call each -> (clen, payload)"""
    parts = [T.orc_enc(T.ANS4S, d[o:o + chunk], cdf, 256) for o in range(0, d.size, chunk)]
    return np.array([p.size for p in parts], dtype=np.uint32), np.concatenate(parts)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs, CDFs and the oracle's results of every case, written once for the three children"""
    cdfs = {"text": _cdf_of(T.text_bytes(1 << 20, 3)), "rare": _rare_cdf(),
            "flat": _cdf_of(np.random.default_rng(5).integers(0, 256, 1 << 20, dtype=np.uint8))}
    shapes = [(chunk, nch, kind) for chunk in CHUNKS for nch in NCHUNKS for kind in KINDS]
    shapes += [(BIG[0], nch, "text") for nch in BIG[1]]
    arrays, names, seed = {}, [], 300
    for chunk, nch, kind in shapes:
        for n in (nch * chunk, nch * chunk - RAGGED_CUT):
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
            if kind in ("text", "quiet"):
                assert not raw[:-1].any(), name
            if kind == "text" and chunk == 4096:
                assert clen[:-1].min() >= 16 * 128, name          # sixteen revolutions of the 128-byte ring at the least
            if kind == "staircase" and nch >= 64:
                w = np.arange(64)                                  # the first full wave
                coded = w[~raw[w]]
                units = ((clen[coded].astype(np.int64) - 8) // 2) % 64      # where the lane's cursor stands at the end, in ring halfwords
                assert np.unique(units).size >= 48 and np.unique(units % 2).size == 2, (name, np.unique(units).size)
    path = str(tmp_path_factory.mktemp("ans4s_ring") / "cases.npz")
    np.savez(path, names=np.array(names), **arrays)
    return path, len(names)


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
        exp_clen, exp_payload = z[name + "/clen"], z[name + "/payload"]
        dc = trc.DeviceCoder(trc.ANS4S, n, chunk, "cuda:0")
        d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
        for fill in (0xA5, 0x5A):
            dc.work.fill_(fill)                                 # the staging regions and everything else in the workspace
            dc.payload.fill_(fill ^ 0xFF)
            dc.total.fill_(-1)
            dc.set_cdf(cdf, 256)                                # (the coder tables live in the workspace: derived again)
            dc.encode(d_in, n)
            clen, payload = dc.result(n)
            assert int(dc.total[0].item()) == exp_payload.size, ("total", name, fill)
            assert np.array_equal(clen, exp_clen), ("clen", name, fill, np.flatnonzero(clen != exp_clen)[:8])
            assert payload.size == exp_payload.size and np.array_equal(payload, exp_payload), ("payload", name, fill, np.flatnonzero(payload != exp_payload)[:8])
            out = torch.full((n + 512,), fill, dtype=torch.uint8, device="cuda:0")
            dc.decode(out, n, dir_ready=True); torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[:n], d) and (o[n:] == fill).all(), ("roundtrip", name, fill)
    print("ok", len(z["names"]))
""") % (os.path.dirname(os.path.abspath(trc.__file__)), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wpb", (1, 4, 12))
def test_ring_layout_matches_oracle(cases, wpb):
    path, ncases = cases
    assert ncases == (len(CHUNKS) * len(NCHUNKS) * len(KINDS) + len(BIG[1])) * 2
    r = subprocess.run([sys.executable, "-c", CHILD, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TRC_ENC_WPB=str(wpb)))
    assert r.returncode == 0 and "ok %d" % ncases in r.stdout, (wpb, r.stdout[-2000:] + r.stderr[-3000:])
