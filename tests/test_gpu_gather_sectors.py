"""GPU (-m gpu): the payload gather writes whole destination-aligned 64-byte sectors (csrc/trc_dir.hip, trc_gather_kernel).

A sector belongs to the piece that holds its first byte; the last sector of a piece takes its remaining vectors from the next
piece (a clamped load of the piece's last 16 bytes spliced with the next piece's first 16, or one load inside the next piece), a
vector that needs a third piece or a piece below 16 bytes goes byte by byte, and the first and last partial sector of a group
(up to 63 bytes each, shared with the neighbouring groups) keep partial stores that write nothing outside the group's bytes.

Every case encodes on the device and compares `clen`, `total` and the whole payload with the per-chunk oracle output concatenated,
then decodes:

  chunks   256 and 512.  256 is TRC_CHUNK_MIN, the smallest chunk the library takes: it stands for the smallest pieces (a chunk of
           64 bytes is refused with TRC_E_ARG by every entry point and cannot be run)
  shapes   one group with 1, 3, 63 and 64 chunks; three groups (165 chunks) with a ragged last chunk
  data     text (pieces of roughly 330 bytes at chunk 512); (nearly) constant bytes (pieces of about 10 bytes, several per sector:
           the bytewise path); incompressible bytes (raw chunks: the piece is the input itself); an alternation of the three, so that
           sectors span piece types
  base     the payload pointer 0, 2, 16, 48 and 62 bytes past a 256-byte boundary (a view into a larger tensor): every length
           class of the first partial sector; the groups behind the first start wherever the lengths put them
  poison   the bytes in front of the base and behind base + total must be intact afterwards; every run is made twice, the workspace
           filled with 0xA5 and then with 0x5A before the encode (the staging regions are written only where a chunk's payload
           lies, so a byte taken from outside a piece would show the fill): both payloads must be the oracle's
  reuse    the coder is called once more on the same buffers, nothing refilled: the payload must be the same again (a check
           against stale lines, whatever cache policy the gather's stores carry)
  rccdfs2  one shape with the two-part coder (two pieces per chunk, two threads per piece)."""
import numpy as np
import pytest

import trc
import trc_testlib as T
from golden.make_golden import gen
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

CHUNKS = (256, 512)
SHAPES = ("1", "3", "63", "64", "3groups")
KINDS = ("text", "const", "raw", "mixed")
OFFSETS = (0, 2, 16, 48, 62)
FRONT = 256                            # poisoned bytes in front of the payload's base
REFS = {}


def size_of(shape, chunk):
    if shape == "3groups":
        return 165 * chunk - chunk // 3 - 1                        # 2 x 64 + 37 chunks, the last one ragged (odd length)
    return int(shape) * chunk


def tiny(n, chunk, seed):
    """one byte value with a different one four times in three chunks: coded chunks of 8, 10, 12 ... bytes"""
    d = np.full(n, 0x41, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    pos = rng.choice(n, size=max(1, 4 * n // (3 * chunk)), replace=False)
    d[pos] = rng.integers(0x42, 0x46, pos.size)
    return d


def make(kind, n, chunk, seed):
    if kind == "text":
        return gen("text", n, seed)
    if kind == "const":
        return tiny(n, chunk, seed)
    if kind == "raw":
        return gen("uniform", n, seed)
    d = gen("text", n, seed)                                        # mixed: text / constant / incompressible chunks in turn
    for c in range((n + chunk - 1) // chunk):
        lo, hi = c * chunk, min(n, (c + 1) * chunk)
        if c % 3 == 1:
            d[lo:hi] = 0x20
        elif c % 3 == 2:
            d[lo:hi] = gen("uniform", hi - lo, seed + c)
    return d


def reference(codec, kind, chunk, shape):
    """(input, cdf, cdfnum, payload, clen) of the per-chunk oracle calls, concatenated; computed once per case"""
    key = (codec, kind, chunk, shape)
    if key not in REFS:
        n = size_of(shape, chunk)
        d = make(kind, n, chunk, 7 + len(REFS))
        if kind == "mixed":                                         # a CDF under which text codes and the random chunks do not
            _, cdf, cdfnum = T.orc_cdfini(np.concatenate([gen("text", 1 << 16, 5), np.full(1 << 14, 0x20, np.uint8),
                                                          gen("uniform", 1 << 12, 6)]), 256)
        elif kind == "raw":                                         # the CDF of a megabyte of random bytes: no chunk codes below its length
            _, cdf, cdfnum = T.orc_cdfini(gen("uniform", 1 << 20, 4), 256)
        else:
            _, cdf, cdfnum = T.orc_cdfini(d)
        payload, clen, _ = T.orc_chunked_enc(codec, d, chunk, cdf, cdfnum)
        REFS[key] = (d, cdf, cdfnum, payload, clen)
    return REFS[key]


def check(torch, codec, kind, chunk, shape, offsets=OFFSETS):
    d, cdf, cdfnum, exp_payload, exp_clen = reference(codec, kind, chunk, shape)
    n, tot = d.size, exp_payload.size
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
    big = torch.empty(FRONT + 64 + dc.payload.numel(), dtype=torch.uint8, device="cuda:0")

    def run(tag):
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        assert int(dc.total[0].item()) == tot, ("total",) + tag
        assert np.array_equal(clen, exp_clen), ("clen",) + tag
        assert payload.size == tot and np.array_equal(payload, exp_payload), ("payload",) + tag + (np.flatnonzero(payload != exp_payload)[:8],)
        return payload

    for off in offsets:
        dc.payload = big[FRONT + off:]                               # the base: `off` bytes past a 256-byte boundary
        assert dc.payload.data_ptr() % 256 == off
        for fill in (0xA5, 0x5A):
            poison = fill ^ 0xFF
            dc.work.fill_(fill)                                     # the staging regions and everything else in the workspace
            big.fill_(poison)
            dc.total.fill_(-1)
            dc.set_cdf(cdf, cdfnum)                                 # (the coder tables live in the workspace: derived again)
            first = run((off, fill))
            whole = big.cpu().numpy()
            assert (whole[:FRONT + off] == poison).all(), ("bytes in front of the base", off, fill)
            assert (whole[FRONT + off + tot:] == poison).all(), ("bytes behind base + total", off, fill,
                                                                  np.flatnonzero(whole[FRONT + off + tot:] != poison)[:8])
            d_out = torch.full((n + 512,), fill, dtype=torch.uint8, device="cuda:0")
            dc.decode(d_out, n)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:n], d) and (out[n:] == fill).all(), ("decode", off, fill)
        again = run((off, "again"))                                 # the same buffers once more, nothing refilled
        assert np.array_equal(again, first), ("the second call's payload differs from the first", off)
        whole = big.cpu().numpy()
        assert (whole[:FRONT + off] == poison).all() and (whole[FRONT + off + tot:] == poison).all(), ("poison after the second call", off)
    return exp_clen, d


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_sectors(torch_cuda, chunk, kind, shape):
    clen, d = check(torch_cuda, trc.ANS4S, kind, chunk, shape)
    lens = np.minimum(chunk, d.size - chunk * np.arange(clen.size))
    raw = clen == lens
    # the data does what it is here for
    if kind == "text":
        assert not raw.any()
        if chunk == 512:
            assert 280 <= np.median(clen) <= 380
    if kind == "const":
        assert clen.max() <= 16 and np.median(clen) <= 12
    if kind == "raw":
        assert raw.all()
    if kind == "mixed" and clen.size >= 3:
        c = np.arange(clen.size)
        assert not raw[c % 3 == 0][:-1].any() and (clen[c % 3 == 1][:-1] < chunk // 4).all() and raw[c % 3 == 2].all()


@pytest.mark.parametrize("kind", ["text", "mixed"])
def test_two_pieces_per_chunk(torch_cuda, kind):
    """`rccdfs2`: two pieces per chunk (PARTS == 2: two threads per piece, a store instruction of a pair is an aligned half sector),
    the second piece empty for a chunk that is stored raw"""
    check(torch_cuda, trc.RCS2, kind, 512, "3groups")
