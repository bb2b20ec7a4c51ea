"""Filtered byte planes on the MI355X.  The whole contract is fplanes(filter, ..., in) == planes(..., F(filter, chunk, esize, in)) with F
the numpy model of fplanes_lib, so every comparison is byte equality: the two kernels alone against the model at the edges of a
vector, a tile, a restart segment and the grid; the coded calls against the unfiltered calls on the model-filtered input; chunk
ranges; argument errors; the TRCF container through host pointers and `trcfile f / d / x`; and what it is for: sorted ids store
fewer bytes.  Every device buffer is followed by a 512-byte guard of 0xA5 that must survive (the kernels' buffers have one on both
sides).  The device calls and comparisons shared with the other plane files are in gpu_planes.py."""
import numpy as np
import pytest

import fplanes_lib as FL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (CHUNK, GUARD, coded_flat, decodes_flat, decodes_ranges_flat, guarded, host_container_filtered, padded, rejected_flat,
                        split_join_flat, trcfile, trcfile_round_trip)
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu
SEGS = (256, 320, 4096, 65536)
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
M6 = 5 * CHUNK + 3                                              # 6 chunks per plane, the last one of 3 elements


def sizes(seg):
    """elements: one, around a thread's vector, around a restart, several segments and a ragged end, and (small segments) more
    segments than one workgroup has waves"""
    return [1, 7, 8, 9, seg - 1, seg, seg + 1, 3 * seg + 5] + ([64 * seg + 8] if seg <= 320 else [])


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, filt, seg, m, t, kind):
    d = FL.gen(kind, esize, m, t, 100 * m + 10 * esize + t)
    planes, tail = PL.split(FL.forward(d, esize, filt, seg), esize)
    tag = "esize %d, filter %s, seg %d, m %d, t %d, %s" % (esize, FL.FILTER_NAMES[filt], seg, m, t, kind)
    split_join_flat(torch, d, esize, m, t, planes, tail, tag, filt=filt, seg=seg)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_split_join(torch_cuda, esize, filt, seg):
    for i, m in enumerate(sizes(seg)):
        for t in (0, esize - 1):
            split_join_case(torch_cuda, esize, filt, seg, m, t, FL.KINDS[(i + (t > 0)) % 4])


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_split_join_grid_capped(torch_cuda, esize, monkeypatch):
    """one workgroup = 4 waves: the split's loop turns 9 and 19 times; the join's waves take 2 or 3 of the 9 spans of 8 segments
    of 256 (4 tiles each; the 65th segment is a span of its own), 3 or 4 of the 13 spans of 5 segments of 320 + 5 elements, and 2 or
    3 of the 10 segments of 4096 (8 tiles each)"""
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    for filt in FL.FILTERS:
        split_join_case(torch_cuda, esize, filt, 256, 64 * 256 + 8, esize - 1, "wrap")
        split_join_case(torch_cuda, esize, filt, 320, 100 * 320 + 5, 0, "walk")
        split_join_case(torch_cuda, esize, filt, 4096, 9 * 4096 + 5, esize - 1, "monotone")


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_largest_input(torch_cuda, esize):
    """2^20 elements: every workgroup of the split's full grid at esize 2 upwards, 16 segments of 65536 with 128 tiles each"""
    split_join_case(torch_cuda, esize, FL.ZDELTA, 65536, 1 << 20, 0, "walk")
    split_join_case(torch_cuda, esize, FL.XOR, 256, (1 << 20) - 3, esize - 1, "monotone")


def test_filter_none_is_the_unfiltered_kernel(torch_cuda):
    torch = torch_cuda
    esize, m, t = 4, 1000, 3
    n = m * esize + t
    d = FL.gen("random", esize, m, t, 1)
    planes, tail = PL.split(d, esize)
    d_in, d_planes, d_tail, d_out = guarded(torch, n, d), guarded(torch, esize * 1024), guarded(torch, 8), guarded(torch, n)
    trc.planes_split_filter(trc.FILTER_NONE, d_in, n, esize, 256, d_planes, 1024, d_tail)
    trc.planes_join_filter(trc.FILTER_NONE, d_planes, 1024, d_tail, n, esize, 256, d_out)
    torch.cuda.synchronize()
    got = d_planes.cpu().numpy()
    for k in range(esize):
        assert np.array_equal(got[k * 1024:k * 1024 + m], planes[k]) and (got[k * 1024 + m:(k + 1) * 1024] == 0xA5).all()
    assert np.array_equal(d_tail.cpu().numpy()[:t], tail)
    assert np.array_equal(d_out.cpu().numpy()[:n], d) and (d_out.cpu().numpy()[n:] == 0xA5).all()


def test_split_join_argument_errors(torch_cuda):
    torch = torch_cuda
    d_in, d_planes, d_tail = guarded(torch, 4096), guarded(torch, 8 * 1024), guarded(torch, 8)
    bad = [(f, 4096, 2, 256, 2048, None) for f in (-1, 3)]                                     # the filter
    bad += [(f, 4096, 2, seg, 2048, None) for f in (0, 1, 2) for seg in (100, 128, 65600, 0)]   # the restart length
    bad += [(1, 4096, 3, 256, 2048, None), (2, 1, 2, 256, 256, d_tail), (1, 3, 4, 256, 256, d_tail)]      # esize 3, no whole element
    bad += [(1, 4096, 2, 256, 2000, None), (1, 4096, 2, 256, 1792, None), (2, 4097, 2, 256, 2048, None)]  # pitch, a tail without a buffer
    for filt, n, esize, seg, pitch, tail in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_filter(filt, d_in, n, esize, seg, d_planes, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_filter(filt, d_planes, pitch, tail, n, esize, seg, d_in)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_split_filter(1, d_in[8:], 1024, 2, 256, d_planes, 1024, None)              # an input that is not 16-byte aligned
    torch.cuda.synchronize()
    assert (d_planes.cpu().numpy() == 0xA5).all() and (d_in.cpu().numpy() == 0xA5).all() and (d_tail.cpu().numpy() == 0xA5).all()


# ---- the coded calls ---------------------------------------------------------------------------------------------------
def coded(torch, codec, esize, filt, chunk=CHUNK, m=M6):
    """-> (input bytes, FilteredPlanesCoder holding their container, PlanesCoder holding the container of the model-filtered input):
    computed once per key, shared, left unchanged"""
    d = FL.gen("monotone" if esize > 2 else "walk", esize, m, esize - 1, 17 * esize + filt)
    return (d,) + coded_flat(torch, codec, esize, chunk, d, trc.FilteredPlanesCoder, lambda: FL.forward(d, esize, filt, chunk), filter=filt)


@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract_and_every_range(torch_cuda, codec, filt):
    torch = torch_cuda
    esize = 4
    d, fc, pc = coded(torch, codec, esize, filt)
    tag = "%s filter %s" % (trc.CODEC_NAMES[codec], FL.FILTER_NAMES[filt])
    assert fc.nch == 6
    assert_same_container(fc, pc, esize, codec, tag)
    decodes_flat(torch, fc, d, tag)
    decodes_ranges_flat(torch, fc, d, esize, CHUNK, [(first, count) for first in range(6) for count in range(1, 6 - first + 1)], tag)


@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("esize,codec", [(2, trc.RCA), (8, trc.ANS4S)])
def test_encode_contract_other_widths(torch_cuda, esize, codec, filt):
    torch = torch_cuda
    chunk, m = 4096, 2 * 4096 + 77
    d, fc, pc = coded(torch, codec, esize, filt, chunk, m)
    tag = "%s esize %d filter %s" % (trc.CODEC_NAMES[codec], esize, FL.FILTER_NAMES[filt])
    assert_same_container(fc, pc, esize, codec, tag)
    decodes_flat(torch, fc, d, tag)
    decodes_ranges_flat(torch, fc, d, esize, chunk, [(1, 2)], tag)


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_filter_none_is_the_unfiltered_call(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d = FL.gen("monotone", esize, M6, esize - 1, 3)
    n = d.size
    fc = trc.FilteredPlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    assert fc.filter == trc.FILTER_NONE
    pc = trc.PlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    d_in = padded(torch, d)
    for c in (fc, pc):
        c.payload[:esize * c.pitch] = 0x5A
        c.encode(d_in, n)
    assert_same_container(fc, pc, esize, codec, trc.CODEC_NAMES[codec] + " filter none")
    for name in ("clen", "total", "tail", "cdf", "status"):
        assert torch.equal(getattr(fc, name), getattr(pc, name)), name
    decodes_flat(torch, fc, d, "filter none")
    decodes_ranges_flat(torch, fc, d, esize, CHUNK, [(2, 2)], "filter none")


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d, fc, _ = coded(torch, codec, esize, FL.ZDELTA)
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    d_in = padded(torch, d)
    names = ("clen", "payload", "total", "tail", "cdf")
    before = [getattr(fc, x).clone() for x in names]

    def rejected(**kw):
        rejected_flat(fc, d_in, d_out, n, **kw)

    for filt in (-1, 3):
        rejected(filter=filt)
    for chunk in (100, 128, 65600):
        rejected(chunk=chunk)
    for flag in (trc.TABLES_READY, trc.DIR_READY):
        rejected(flags=flag)
    rejected(esize=3)
    rejected(nbytes=esize - 1)                                  # m == 0
    for first, count in ((6, 1), (0, 7), (3, 4)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            fc.decode_range(d_out, first, count, n)
    fc.decode_range(d_out, 2, 0, n)                             # count 0: TRC_OK, nothing launched
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its output"
    for x, b in zip(names, before):
        assert torch.equal(getattr(fc, x), b), "a rejected encode changed the container"
    assert fc.guards_ok()


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (256, 0))
@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S))
def test_host_container(torch_cuda, codec, filt, chunk):
    esize, m = 4, 9 * 256 + 3
    d = FL.gen("monotone", esize, m, esize - 1, 23)
    host_container_filtered(codec, d, esize, m, chunk, b"TRCF", (filt, 1, 0, 0), lambda x, ch: trc.host_encode_fplanes(codec, filt, x, esize, ch),
                            trc.fplanes_check, trc.host_decode_fplanes, trc.host_decode_fplanes_range, lambda seg: FL.forward(d, esize, filt, seg))
    with pytest.raises(trc.TrcError, match="filter 0"):
        trc.host_encode_fplanes(codec, trc.FILTER_NONE, d, esize, chunk)


def test_sorted_ids_store_fewer_bytes_with_zdelta(torch_cuda):
    """1 MiB of sorted 32-bit ids (2^18 draws from [0, 2^32), sorted: neighbours differ by 2^14 on average) through rccdf at the
    automatic chunk: order-0 entropy 7.75 bits per byte as planes, 3.1 behind the zigzag delta"""
    m = 1 << 18
    ids = np.sort(np.random.default_rng(7).integers(0, 1 << 32, m, dtype=np.uint64)).astype("<u4")
    d = ids.view(np.uint8)
    plain = trc.host_encode_planes(trc.RCA, d, 4, 0)
    filtered = trc.host_encode_fplanes(trc.RCA, trc.FILTER_ZDELTA, d, 4, 0)
    xored = trc.host_encode_fplanes(trc.RCA, trc.FILTER_XOR, d, 4, 0)
    print("sorted u32 ids, %d bytes: planes %d, zigzag delta + planes %d, xor + planes %d" % (d.size, plain.size, filtered.size, xored.size))
    assert filtered.size < plain.size
    assert np.array_equal(trc.host_decode_fplanes(filtered, d.size), d)


def test_trcfile_fplanes(torch_cuda, tmp_path):
    d = FL.gen("monotone", 4, 40000, 3, 9)
    for letter, filt in (("z", 1), ("x", 2)):
        head = trcfile_round_trip(tmp_path, d, "trcf", ["f", "46", "4", letter], 70001, 3000)
        assert head[:4].tobytes() == b"TRCF" and head[4] == filt and head[16:20].tobytes() == b"TRCP"
    r = trcfile("f", "46", "4", "q", tmp_path / "in.bin", tmp_path / "in.trcf", rc=2)
    assert "filter" in r.stderr
