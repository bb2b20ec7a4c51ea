"""Strided filtered byte planes on the MI355X.  The whole contract is splanes(filter, S, ..., in) == planes(..., F_S(filter, chunk, esize,
in)) with F_S the numpy model of splanes_lib, so every comparison is byte equality: the two kernels alone against the model at the
edges of the stride, a vector, a tile, a restart segment, a span and the grid; stride 1 and TRC_FILTER_NONE against the existing
calls; the coded calls against the unfiltered calls on the model-filtered input; chunk ranges; argument errors; the histograms of
trc_planes_hist_stride_dev against numpy bincounts; the TRCS container through host pointers and `trcfile s / d / x`; and what it
is for: a row-major table stores fewer bytes.  The kernel tests put 512 guard bytes of 0xA5 on both sides of every device buffer.
The device calls and comparisons shared with the other plane files are in gpu_planes.py."""
import numpy as np
import pytest

import fplanes_lib as FL
import planes_lib as PL
import splanes_lib as SL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (GUARD, Guarded, assert_hists, coded_flat, decodes_flat, decodes_ranges_flat, device_hists, guarded, host_container_filtered,
                        padded, rejected_flat, split_join_flat, trcfile, trcfile_round_trip, up256)
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu


def shapes(stride):
    """(seg, m): one element, around the stride, a vector, a restart, a tile and a span of 8 short segments, several long segments"""
    return [(256, 1), (256, stride), (256, stride + 1), (256, 9), (256, 257), (320, 3 * 320 + 5), (512, 512 + 7), (256, 2 * 8 * 256 + 13),
            (4096, 4097), (4096, 3 * 4096 + 5), (65536, 65536 + 9)]


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, filt, stride, seg, m, t, kind):
    d = SL.gen(kind, esize, m, t, 100 * m + 10 * esize + t + stride, stride)
    planes, tail = PL.split(SL.forward(d, esize, filt, seg, stride), esize)
    tag = "esize %d, filter %s, stride %d, seg %d, m %d, t %d, %s" % (esize, FL.FILTER_NAMES[filt], stride, seg, m, t, kind)
    split_join_flat(torch, d, esize, m, t, planes, tail, tag, filt=filt, stride=stride, seg=seg)


@pytest.mark.parametrize("stride", SL.STRIDES)
@pytest.mark.parametrize("filt", SL.FILTERS)
@pytest.mark.parametrize("esize", SL.ESIZES)
def test_split_join(torch_cuda, esize, filt, stride):
    for i, (seg, m) in enumerate(shapes(stride)):
        for t in (0, esize - 1):
            split_join_case(torch_cuda, esize, filt, stride, seg, m, t, ("random", "wrap", "interleaved")[(i + (t > 0) + stride) % 3])


@pytest.mark.parametrize("esize", SL.ESIZES)
def test_split_join_grid_capped(torch_cuda, esize, monkeypatch):
    """one workgroup = 4 waves: the split's loop turns 9 and 19 times; the join's waves take 2 or 3 of the 9 spans of 8 segments of
    256 (4 tiles each), 3 or 4 of the 13 spans of 5 segments of 320, and 2 or 3 of the 10 segments of 4096 (8 tiles each)"""
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    for filt, strides in ((FL.ZDELTA, (3, 8)), (FL.XOR, (2, 7))):
        for stride in strides:
            split_join_case(torch_cuda, esize, filt, stride, 256, 64 * 256 + 8, esize - 1, "wrap")
            split_join_case(torch_cuda, esize, filt, stride, 320, 100 * 320 + 5, 0, "interleaved")
            split_join_case(torch_cuda, esize, filt, stride, 4096, 9 * 4096 + 5, esize - 1, "random")


def test_stride_one_and_filter_none_are_the_existing_kernels(torch_cuda):
    torch = torch_cuda
    for esize in SL.ESIZES:
        m, t, seg = 3 * 256 + 5, esize - 1, 256
        n, pitch = m * esize + t, up256(m)
        d = FL.gen("random", esize, m, t, esize)
        for filt, stride in ((FL.ZDELTA, 1), (FL.XOR, 1), (FL.NONE, 1), (FL.NONE, 5), (FL.NONE, 8)):
            bufs = []
            for strided in (True, False):
                d_in, d_planes, d_tail, d_out = Guarded(torch, n, d), Guarded(torch, esize * pitch), Guarded(torch, 8), Guarded(torch, n)
                if strided:
                    trc.planes_split_sfilter(filt, stride, d_in.t, n, esize, seg, d_planes.t, pitch, d_tail.t)
                    trc.planes_join_sfilter(filt, stride, d_planes.t, pitch, d_tail.t, n, esize, seg, d_out.t)
                else:
                    trc.planes_split_filter(filt, d_in.t, n, esize, seg, d_planes.t, pitch, d_tail.t)
                    trc.planes_join_filter(filt, d_planes.t, pitch, d_tail.t, n, esize, seg, d_out.t)
                torch.cuda.synchronize()
                bufs.append([b.whole.cpu().numpy() for b in (d_planes, d_tail, d_out)])
            for a, b, what in zip(bufs[0], bufs[1], ("planes", "tail", "output")):
                assert np.array_equal(a, b), (esize, filt, stride, what)
            assert np.array_equal(bufs[0][2][GUARD:GUARD + n], d)


def test_split_join_argument_errors_launch_nothing(torch_cuda):
    torch = torch_cuda
    d_in, d_planes, d_tail = Guarded(torch, 4096), Guarded(torch, 8 * 1024), Guarded(torch, 8)
    bad = [(f, s, 4096, 2, 256, 2048, None) for f in (0, 1, 2) for s in (0, 9, -1)]                      # the stride
    bad += [(f, 3, 4096, 2, 256, 2048, None) for f in (-1, 3)]                                            # the filter
    bad += [(f, 3, 4096, 2, seg, 2048, None) for f in (0, 1, 2) for seg in (100, 128, 65600, 0)]          # the restart length
    bad += [(1, 2, 4096, 3, 256, 2048, None), (2, 8, 1, 2, 256, 256, d_tail.t), (1, 4, 3, 4, 256, 256, d_tail.t)]      # esize 3, no whole element
    bad += [(1, 5, 4096, 2, 256, 2000, None), (1, 6, 4096, 2, 256, 1792, None), (2, 7, 4097, 2, 256, 2048, None)]      # pitch, a tail without a buffer
    for filt, stride, n, esize, seg, pitch, tail in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_sfilter(filt, stride, d_in.t, n, esize, seg, d_planes.t, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_sfilter(filt, stride, d_planes.t, pitch, tail, n, esize, seg, d_in.t)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_split_sfilter(1, 3, d_in.t[8:], 1024, 2, 256, d_planes.t, 1024, None)               # an input that is not 16-byte aligned
    d_hist = Guarded(torch, trc.planes_hist_bytes(4))
    for filters, stride, esize, seg in ((7, 0, 4, 256), (7, 9, 4, 256), (0, 3, 4, 256), (8, 3, 4, 256), (6, 3, 3, 256), (6, 3, 4, 100)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_hist_stride(filters, stride, d_in.t, 4096, esize, seg, d_hist.t)
    torch.cuda.synchronize()
    for b in (d_in, d_planes, d_tail, d_hist):
        assert (b.whole.cpu().numpy() == 0xA5).all(), "a rejected call wrote something"


# ---- the histograms -----------------------------------------------------------------------------------------------------
def hist_case(torch, esize, stride, seg, m, filters=7):
    d = SL.gen("interleaved", esize, m, esize - 1, 31 * m + esize, stride)
    got, _ = device_hists(torch, esize, seg, filters, d=d, strides=stride)
    assert_hists(got, SL.hist3(d, esize, seg, stride), [m], filters, "esize %d, stride %d, seg %d, m %d, filters %d" % (esize, stride, seg, m, filters))


@pytest.mark.parametrize("esize,stride", [(2, 3), (4, 4), (8, 7)])
def test_hist_stride(torch_cuda, esize, stride, monkeypatch):
    for m in (1, stride, 7, 8, 9, 255, 256, 257, 3 * 256 + 5, 40 * 256 + 3):
        hist_case(torch_cuda, esize, stride, 256, m)
    hist_case(torch_cuda, esize, stride, 4096, 2 * 4096 + 77)
    for filters in (2, 4, 5, 6):
        hist_case(torch_cuda, esize, stride, 320, 3 * 320 + 5, filters)
    # stride 1 is trc_planes_hist_dev
    n = 1000 * esize
    d = FL.gen("walk", esize, 1000, 0, 3)
    d_in, a, b = Guarded(torch_cuda, n, d), Guarded(torch_cuda, trc.planes_hist_bytes(esize)), Guarded(torch_cuda, trc.planes_hist_bytes(esize))
    trc.planes_hist_stride(7, 1, d_in.t, n, esize, 256, a.t)
    trc.planes_hist(7, d_in.t, n, esize, 256, b.t)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(a.whole.cpu().numpy(), b.whole.cpu().numpy())
    # one workgroup: its loop turns 11 times
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    hist_case(torch_cuda, esize, stride, 256, 10 * 2048 + 13)


# ---- the coded calls ---------------------------------------------------------------------------------------------------
def coded(torch, codec, esize, filt, stride, chunk, m):
    """-> (input bytes, StridedPlanesCoder holding their container, PlanesCoder holding the container of the model-filtered input):
    computed once per key, shared, left unchanged"""
    d = SL.gen("interleaved", esize, m, esize - 1, 17 * esize + filt + stride, stride)
    return (d,) + coded_flat(torch, codec, esize, chunk, d, trc.StridedPlanesCoder, lambda: SL.forward(d, esize, filt, chunk, stride),
                             filter=filt, stride=stride)


CODED = [(4, c, chunk) for c in (trc.ANS4S, trc.RCA, trc.RCB) for chunk in (256, 4096)] + [(2, trc.RCA, 256), (8, trc.ANS4S, 256)]


@pytest.mark.parametrize("stride", (2, 3, 8))
@pytest.mark.parametrize("esize,codec,chunk", CODED, ids=["%d-%s-%d" % (e, trc.CODEC_NAMES[c], ch) for e, c, ch in CODED])
def test_encode_contract_decode_and_ranges(torch_cuda, esize, codec, chunk, stride):
    torch = torch_cuda
    m = 5 * chunk + 3 if chunk == 256 else 2 * chunk + 77
    for filt in SL.FILTERS:
        d, sc, pc = coded(torch, codec, esize, filt, stride, chunk, m)
        tag = "%s esize %d chunk %d filter %s stride %d" % (trc.CODEC_NAMES[codec], esize, chunk, FL.FILTER_NAMES[filt], stride)
        nch = sc.nch
        assert nch == (m + chunk - 1) // chunk
        assert_same_container(sc, pc, esize, codec, tag)
        assert torch.equal(sc.total, pc.total) and torch.equal(sc.clen, pc.clen), tag + ": totals or directory"
        decodes_flat(torch, sc, d, tag)
        decodes_ranges_flat(torch, sc, d, esize, chunk, ((0, 1), (1, 1), (nch - 1, 1), (1, nch - 1)), tag)


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_stride_one_and_filter_none_are_the_existing_calls(torch_cuda, codec):
    torch = torch_cuda
    esize, chunk, m = 4, 256, 5 * 256 + 3
    d = FL.gen("monotone", esize, m, esize - 1, 3)
    n = d.size
    d_in = padded(torch, d)
    for filt, stride in ((FL.ZDELTA, 1), (FL.XOR, 1), (FL.NONE, 1), (FL.NONE, 6)):
        sc = trc.StridedPlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, guard=GUARD, filter=filt, stride=stride)
        fc = trc.FilteredPlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, guard=GUARD, filter=filt)
        for c in (sc, fc):
            c.payload[:esize * c.pitch] = 0x5A
            c.encode(d_in, n)
        tag = "%s filter %d stride %d" % (trc.CODEC_NAMES[codec], filt, stride)
        assert_same_container(sc, fc, esize, codec, tag)
        for name in ("clen", "total", "tail", "cdf", "status"):
            assert torch.equal(getattr(sc, name), getattr(fc, name)), tag + ": " + name
        decodes_flat(torch, sc, d, tag)
        decodes_ranges_flat(torch, sc, d, esize, chunk, [(2, 2)], tag)


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize, chunk, m = 4, 256, 5 * 256 + 3
    d, sc, _ = coded(torch, codec, esize, FL.ZDELTA, 3, chunk, m)
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    d_in = padded(torch, d)
    names = ("clen", "payload", "total", "tail", "cdf")
    before = [getattr(sc, x).clone() for x in names]

    def rejected(**kw):
        rejected_flat(sc, d_in, d_out, n, **kw)

    for stride in (0, 9, -1):
        rejected(stride=stride)
        rejected(stride=stride, filter=trc.FILTER_NONE)
    for filt in (-1, 3):
        rejected(filter=filt)
    for ch in (100, 128, 65600):
        rejected(chunk=ch)
    for flag in (trc.TABLES_READY, trc.DIR_READY):
        rejected(flags=flag)
    rejected(esize=3)
    rejected(nbytes=esize - 1)                                  # m == 0
    rejected(codec=trc.RC4)                                     # a low-nibble coder
    for first, count in ((6, 1), (0, 7), (3, 4)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            sc.decode_range(d_out, first, count, n)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its output"
    for x, b in zip(names, before):
        assert torch.equal(getattr(sc, x), b), "a rejected encode changed the container"
    assert sc.guards_ok()


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (256, 0))
@pytest.mark.parametrize("filt,stride", [(FL.ZDELTA, 4), (FL.XOR, 3), (FL.ZDELTA, 7)])
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S))
def test_host_container(torch_cuda, codec, filt, stride, chunk):
    esize, m = 4, 9 * 256 + 3
    d = SL.gen("interleaved", esize, m, esize - 1, 23, stride)
    n = d.size
    comp, _ = host_container_filtered(codec, d, esize, m, chunk, b"TRCS", (filt, 1, stride, 0),
                                      lambda x, ch: trc.host_encode_splanes(codec, filt, stride, x, esize, ch), trc.splanes_check,
                                      trc.host_decode_splanes, trc.host_decode_splanes_range, lambda seg: SL.forward(d, esize, filt, seg, stride),
                                      more_ranges=lambda c: [(c + 5, 3 * c + 1)])
    assert np.array_equal(trc.host_decode_xplanes(comp, n), d)
    with pytest.raises(trc.TrcError, match="trc_encode_fplanes_host"):
        trc.host_encode_splanes(codec, filt, 1, d, esize, chunk)
    with pytest.raises(trc.TrcError, match="magic"):
        trc.host_decode_fplanes(comp, n)                        # a TRCS container is not a TRCF container


def test_a_table_of_four_fields_stores_fewer_bytes_with_stride_four(torch_cuda):
    """1 MiB of rows of 4 u32 fields (a sorted id, two timestamps, a counter) through rccdf at the automatic chunk: as planes, behind the
    zigzag delta against the previous element (another column), and behind the zigzag delta against the element 4 back (the same
    column of the previous row)"""
    d = SL.table_rows(1 << 16)
    plain = trc.host_encode_planes(trc.RCA, d, 4, 0)
    stride1 = trc.host_encode_fplanes(trc.RCA, trc.FILTER_ZDELTA, d, 4, 0)
    stride4 = trc.host_encode_splanes(trc.RCA, trc.FILTER_ZDELTA, 4, d, 4, 0)
    print("rows of 4 u32 fields, %d bytes: TRCP %d, TRCF zigzag delta %d, TRCS zigzag delta stride 4 %d" % (d.size, plain.size, stride1.size, stride4.size))
    assert stride4.size < plain.size and stride4.size < stride1.size
    assert np.array_equal(trc.host_decode_splanes(stride4, d.size), d)


def test_trcfile_splanes(torch_cuda, tmp_path):
    d = np.concatenate([SL.table_rows(10000), np.array([1, 2, 3], dtype=np.uint8)])
    for letter, filt, stride in (("z", 1, 4), ("x", 2, 3)):
        head = trcfile_round_trip(tmp_path, d, "trcs", ["s", "46", "4", letter, stride], 70001, 3000)
        assert head[:4].tobytes() == b"TRCS" and head[4] == filt and head[6] == stride and head[16:20].tobytes() == b"TRCP"
    r = trcfile("s", "46", "4", "z", "9", tmp_path / "in.bin", tmp_path / "in.trcs", rc=2)
    assert "stride" in r.stderr
