"""What the coder matrix of the byte-plane calls (test_gpu_planes_matrix.py) shares with the files it grew out of: the input of
test_gpu_range.py (chunks that alternate between uniform bytes and the coder's skewed kind, so that raw and coded chunks mix in
every directory), the seven low-nibble coders the planes calls refuse, the container comparison of test_gpu_fplanes.py, and a
message that names the first differing plane, chunk and byte of two planar results."""
import numpy as np

import nibbit_lib as NL
import sweep_lib as S
import trc
import trc_testlib as T

# in[i] & 15 in, in[i] & 15 out, never stored raw (include/trc_hip.h): refused by every coded planes entry point
LOW4 = (trc.RCA4, trc.RCAI4, trc.ANSA4, trc.RC4, trc.RC4C, trc.RC4SS, trc.RC4CSS)
LOW4_TEXT = "keeps only the low four bits of a byte"
ASSIGNED = sorted(trc.CODEC_NAMES)                              # every id with a row in the codec table


def chunk_of(codec):
    """the smallest chunk the coder's GPU tests use"""
    return 1024 if codec == trc.ANSO1 else 256


def mixed_input(codec, nchunks, tail, seed=0, chunk=None):
    """nchunks - 1 chunks and a last one of `tail` bytes, alternating between uniform and skewed data of the coder's kind (the even
    chunks uniform) -> (n, chunk, bytes).  The two generators are seeded 5 + seed and 6 + seed."""
    chunk = chunk or chunk_of(codec)
    total = (nchunks - 1) * chunk + tail
    n = (total + 3) & ~3                                        # the generators of 16 / 32-bit elements make whole elements
    a, b = 5 + seed, 6 + seed
    if codec in S.FAMILY:
        skew, uni = S.gen(codec, S.HEAD[S.FAMILY[codec]], n, a), S.uniform(n, b)
    elif codec in NL.CODECS:
        nib = codec in NL.NIBBLE
        skew, uni = NL.gen("nib_skew" if nib else "bytes_small", n, a), NL.gen("nib_uniform" if nib else "bytes_uniform", n, b)
    elif codec in T.NIBBLE_CODECS:
        skew, uni = T.nibble_bytes(n, a, "geo"), T.nibble_bytes(n, b, "uniform")
    elif codec in T.VLC_CODECS:
        skew, uni = T.int_bytes(n, T.VLC_ELEM[codec], "small", a), T.int_bytes(n, T.VLC_ELEM[codec], "wide", b)
    else:
        skew, uni = T.nibble_bytes(n, a, "geo"), T.uniform_bytes(n, b)
    d = np.where((np.arange(n) // chunk) % 2 == 0, uni[:n], skew[:n]).astype(np.uint8)
    return total, chunk, d[:total].copy()


def first_difference(name, got, exp, chunk=None, clen=None):
    """'' where the arrays are equal; else where they first differ -- for a payload with its directory `clen`, the chunk and the byte
    within that chunk's payload; for decoded bytes with `chunk`, the chunk and the byte within it"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return ""
    m = min(got.size, exp.size)
    bad = np.flatnonzero(got.reshape(-1)[:m] != exp.reshape(-1)[:m])
    if not bad.size:
        return "%s: %d entries, expected %d (equal up to the shorter)" % (name, got.size, exp.size)
    i = int(bad[0])
    msg = "%s: first difference at %d (0x%x, expected 0x%x)" % (name, i, int(got.reshape(-1)[i]), int(exp.reshape(-1)[i]))
    if clen is not None:
        starts = np.concatenate([[0], np.cumsum(np.asarray(clen, dtype=np.int64))])
        k = int(np.searchsorted(starts, i, side="right")) - 1
        msg += ": chunk %d, byte %d of its %d" % (k, i - starts[k], int(clen[k]) if k < len(clen) else -1)
    elif chunk:
        msg += ": chunk %d, byte %d" % (i // chunk, i % chunk)
    return msg


def assert_same_container(fc, pc, esize, codec, tag):
    """the planar results two PlanesCoders hold are the same: tail, and per plane total, directory, payload and (static coders) CDF
    and cdfini status; the 64 bytes behind each of fc's payloads still hold the 0x5A they were filled with; something is coded"""
    assert np.array_equal(fc.tail[:esize - 1].cpu().numpy(), pc.tail[:esize - 1].cpu().numpy()), tag + ": tail"
    coded_chunks = 0
    for k in range(esize):
        clen, payload, total = fc.result(k)
        exp_clen, exp_payload, exp_total = pc.result(k)
        assert total == exp_total, tag + ": total of plane %d" % k
        assert np.array_equal(clen, exp_clen), tag + ": directory of plane %d" % k
        assert np.array_equal(payload, exp_payload), tag + ": payload of plane %d" % k
        assert (fc.payload[k * fc.pitch + total:k * fc.pitch + total + 64].cpu().numpy() == 0x5A).all(), tag + ": bytes behind the payload"
        if codec in trc.STATIC:
            (cdf, status), (exp_cdf, exp_status) = fc.cdf_of(k), pc.cdf_of(k)
            assert status == exp_status == fc.m and np.array_equal(cdf, exp_cdf), tag + ": CDF of plane %d" % k
        coded_chunks += int((clen < np.minimum(fc.chunk, fc.m - np.arange(0, fc.m, fc.chunk))).sum())
    assert coded_chunks, tag + ": the input is meant to compress somewhere"
