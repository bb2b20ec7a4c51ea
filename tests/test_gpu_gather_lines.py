"""GPU (-m gpu): the payload gather's loads stay inside the pieces they take bytes from ("The gather's loads stay
inside their pieces").

A vector of the gather that runs past the end of its piece takes the piece's last 16 bytes and the next piece's first 16 and
cuts itself out of the two; pieces shorter than 16 bytes go byte by byte.  Every case here encodes on the device and compares the
length directory, the total and the whole payload with the concatenation of the per-chunk reference calls, then decodes.  Every
case runs twice, the workspace filled with 0xA5 and then with 0x5A before the encode: a byte taken from outside a piece (the
staging regions are written only where a chunk's payload lies) would show the fill, so the two payloads must be identical too.

Shapes: the smallest at which the changed loads can go wrong -- pieces of 8 to 12 bytes (three or more inside one vector, both
"piece below 16 bytes" exits), a first long piece on each of the eight even residues of a 16-byte vector, raw pieces (source: the
input) next to coded ones in both orders, a coded last chunk (its piece ends at the last byte of the staging area), and the
two-pieces-per-chunk layout of `rccdfs2` with its empty second pieces for raw chunks."""
import numpy as np
import pytest

import trc
import trc_testlib as T
from golden.make_golden import gen
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def const(n, v=0x41):
    return np.full(n, v, dtype=np.uint8)


def reference(codec, d, chunk):
    """(cdf, cdfnum, payload, clen) of the per-chunk reference calls, concatenated"""
    _, cdf, cdfnum = T.orc_cdfini(d)
    payload, clen, _ = T.orc_chunked_enc(codec, d, chunk, cdf, cdfnum)
    return cdf, cdfnum, payload, clen


def check(torch, codec, d, chunk, ref=None):
    n = d.size
    cdf, cdfnum, exp_payload, exp_clen = ref or reference(codec, d, chunk)
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
    seen = []
    for fill in (0xA5, 0x5A):
        dc.work.fill_(fill)                                         # the staging regions and everything else in the workspace
        dc.payload.fill_(fill ^ 0xFF)
        dc.total.fill_(-1)
        dc.set_cdf(cdf, cdfnum)                                     # (the coder tables live in the workspace: derived again)
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        assert int(dc.total[0].item()) == exp_payload.size, ("total", fill)
        assert np.array_equal(clen, exp_clen), ("clen", fill)
        assert payload.size == exp_payload.size and np.array_equal(payload, exp_payload), ("payload", fill)
        d_out = torch.full((n + 512,), fill, dtype=torch.uint8, device="cuda:0")
        dc.decode(d_out, n)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:n], d) and (out[n:] == fill).all(), ("decode", fill)
        seen.append(payload)
    assert np.array_equal(seen[0], seen[1]), "the payload depends on what the workspace held before the encode"
    return exp_clen


def tiny(n, chunk, seed):
    """one byte value with a different one four times in three chunks: coded chunks of 8, 10, 12 ... bytes"""
    d = const(n)
    rng = np.random.default_rng(seed)
    pos = rng.choice(n, size=max(1, 4 * n // (3 * chunk)), replace=False)
    d[pos] = rng.integers(0x42, 0x46, pos.size)
    return d


@pytest.mark.parametrize("chunk", [256, 320])
@pytest.mark.parametrize("nchunks", [1, 2, 65, 130])
def test_tiny_pieces(torch_cuda, chunk, nchunks):
    """(nearly) constant bytes: the pieces are 8 to 12 bytes, now and then 14 or 16, so a vector holds parts of two or three
    pieces and both "shorter than 16 bytes" exits run.  What matters is the length of the pieces, not of the chunks: the cases
    use the two smallest chunk sizes the library takes (TRC_CHUNK_MIN = 256; 320 is no multiple of 128)."""
    n = nchunks * chunk - chunk // 3                                 # ragged last chunk
    clen = check(torch_cuda, trc.ANS4S, tiny(n, chunk, nchunks), chunk)
    assert clen.min() >= 8 and clen.max() <= 16 and (clen < 16).mean() > 0.9
    if nchunks >= 65:
        assert np.unique(clen).size >= 3


SPACE = 0x20
SHORT_RARE = (0, 1, 2, 3, 4, 5, 10)     # bytes other than SPACE in short chunk i: coded lengths 56 58 60 60 60 62 72 under TEXT_CDF
TEXT_REF = {}


def text_cdf():
    """a CDF made by the caller: text with as many spaces again, so that a chunk of spaces codes to some 60 bytes and a chunk of
    text still to fewer than 512"""
    if "cdf" not in TEXT_REF:
        _, cdf, cdfnum = T.orc_cdfini(np.concatenate([gen("text", 1 << 16, 5), const(1 << 16, SPACE)]), 256)
        TEXT_REF["cdf"] = (cdf, cdfnum)
    return TEXT_REF["cdf"]


def short_chunk(i):
    d = const(512, SPACE)
    d[7:7 + 37 * SHORT_RARE[i]:37] = 0x7a
    return d


def text_ref(nshort, nchunks):
    """(input, reference): nshort short chunks, then nchunks of text with a ragged last one; computed once per shape"""
    key = (nshort, nchunks)
    if key not in TEXT_REF:
        d = np.concatenate([short_chunk(i) for i in range(nshort)] + [gen("text", 512 * nchunks - 100, 31 + nchunks)])
        cdf, cdfnum = text_cdf()
        payload, clen, _ = T.orc_chunked_enc(trc.ANS4S, d, 512, cdf, cdfnum)
        TEXT_REF[key] = (d, (cdf, cdfnum, payload, clen))
    return TEXT_REF[key]


@pytest.mark.parametrize("nchunks", [64, 65, 129])
@pytest.mark.parametrize("nshort", range(8))
def test_text_pieces_on_every_residue(torch_cuda, nshort, nchunks):
    """text at chunk 512 (pieces of some 370 bytes under text_cdf) behind 0 .. 7 short chunks: the first text piece starts at each
    even residue of a 16-byte vector, and the pieces behind it wherever the lengths put them"""
    d, ref = text_ref(nshort, nchunks)
    clen = check(torch_cuda, trc.ANS4S, d, 512, ref)
    assert (clen[:nshort] < 128).all() and (clen[nshort:-1] >= 256).all() and (clen[nshort:] < 512).all()


def test_the_short_chunks_reach_every_even_residue():
    """what the case above relies on: the lengths of the short pieces put the first text piece on all eight even residues
    (group 0 starts on a 16-byte boundary of the payload)"""
    res = set()
    for nshort in range(8):
        clen = text_ref(nshort, 64)[1][3]
        res.add(int(clen[:nshort].sum()) % 16)
    assert res == {0, 2, 4, 6, 8, 10, 12, 14}


def mixed(order, last_coded, seed):
    kinds = {"u": lambda i: gen("uniform", 512, seed + i), "c": lambda i: const(512, SPACE), "t": lambda i: gen("text", 512, seed + i)}
    parts = [kinds[order[i % len(order)]](i) for i in range(150)]
    parts.append(gen("text", 300, seed + 999) if last_coded else gen("uniform", 300, seed + 999))
    return np.concatenate(parts)


@pytest.mark.parametrize("order", ["uct", "tcu", "ut", "uc", "uuctt"])
@pytest.mark.parametrize("last_coded", [True, False], ids=["last-coded", "last-raw"])
def test_raw_next_to_coded(torch_cuda, order, last_coded):
    """incompressible, constant and text chunks interleaved: a raw piece (source: the input chunk, end: the chunk's end) next to
    a coded one, in both orders; a coded last chunk ends at the last byte of the staging area"""
    d = mixed(order, last_coded, 500)
    clen = check(torch_cuda, trc.ANS4S, d, 512)
    raw = clen == np.minimum(512, d.size - 512 * np.arange(clen.size))
    assert raw.any() and (~raw).any() and bool(raw[-1]) != last_coded


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("kind", ["text", "const", "mixed"])
def test_two_pieces_per_chunk(torch_cuda, chunk, kind):
    """`rccdfs2`: two pieces per chunk, the second one empty for a chunk that is stored raw"""
    n = 131 * chunk + chunk // 2 + 1
    if kind == "text":
        d = gen("text", n, 9)
    elif kind == "const":
        d = const(n)
    else:
        d = gen("text", n, 9)
        for c in range(3, 131, 5):
            d[c * chunk:(c + 1) * chunk] = gen("uniform", chunk, c)
        for c in range(4, 131, 7):
            d[c * chunk:(c + 1) * chunk] = 0x41
    check(torch_cuda, trc.RCS2, d, chunk)
