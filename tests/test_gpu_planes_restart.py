"""The five scanning joins of the byte planes (trc_fplanes_join_kernel, trc_fplanes_join_batch_kernel,
trc_splanes_join_batch_kernel, trc_oplanes_join_kernel, trc_oplanes_join_batch_kernel) on the MI355X at restart lengths that leave
a PARTIAL tile inside a span.  A wave walks a span in tiles of 512 elements; at 256, 320, 512, 4096 and 65536 -- the lengths of the
other plane files -- every full-length span is a whole number of tiles, so the lane's place in its segment at a span's end is the
same whether it is reset or merely advanced.  At 576, 960 and 1984 it is not: the last tile of a span has lanes without elements,
and under a capped grid the wave's prefetch goes from that tile into its next span.

  seg   384, 448   spans of 8 segments, 6 and 7 whole tiles: segment edges at places in a tile that 256 and 320 do not reach
        576        one tile + 8 lanes
        960        one tile + 448 elements
        1984       3 tiles + 448 elements (the coder sweeps' odd chunk)
        2560       5 whole tiles: the control

Every flat case has m = 5 spans + half a span + 5 elements and esize - 1 tail bytes -- six spans, the last one partial and ending in
a partial vector -- and runs uncapped (a wave per span) and under TRC_PLANES_GRID=1 (one workgroup: its four waves share the six
spans, waves 0 and 1 go on from a partial tile into a second span).  The batches run at chunks 448, 576 and 1984 uncapped and under
the grid cap of their own files.  Histograms and coded calls at the same lengths.  Every comparison is byte or counter equality
against the numpy models (fplanes_lib, splanes_lib, oplanes_lib and their batch forms); the device calls and comparisons are those of
gpu_planes.py."""
import pytest

import fplanes_batch_lib as FBL
import fplanes_lib as FL
import gpu_planes as GP
import obatch_lib as OBL
import oplanes_lib as OL
import planes_lib as PL
import splanes_batch_lib as SBL
import splanes_lib as SL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (assert_hists, assert_order_hists, coded_flat, decodes_flat, decodes_ranges_flat, device_hists, device_order_hists,
                        split_join_batch, split_join_flat)
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu

RESTARTS = FL.RESTARTS
TILE = 512                                                     # TRC_FPLANES_TILE
CAPS = (None, "1")                                             # TRC_PLANES_GRID: uncapped, one workgroup
S_STRIDES = (3, 6, 8)
O_STRIDES = (1, 3, 6, 7, 8)                                    # 6: the rotating even stride; 7: the half-filled last pair at 16 bits


def elements(seg):
    """five spans, half a span and 5 elements: six spans, the last one partial and ending in a partial vector"""
    span = 8 * seg if seg < TILE else seg
    return 5 * span + span // 2 + 5


def capped(monkeypatch, cap):
    """the cap is read per call"""
    if cap is None:
        monkeypatch.delenv("TRC_PLANES_GRID", raising=False)
    else:
        monkeypatch.setenv("TRC_PLANES_GRID", cap)


def test_the_restart_lengths_are_what_the_matrix_is_for():
    """from a tile upwards every length but the control leaves a partial tile at the end of a full-length span; below a tile the
    spans are 6 and 7 whole tiles with segment edges inside the tiles; every shape has six spans"""
    for seg in RESTARTS:
        span = 8 * seg if seg < TILE else seg
        assert seg % 64 == 0 and (span % TILE != 0) == (seg > TILE and seg != 2560), seg
        assert -(-elements(seg) // span) == 6 and elements(seg) % 8 == 5, seg
    assert [8 * seg // TILE for seg in RESTARTS[:2]] == [6, 7]


# ---- the flat joins --------------------------------------------------------------------------------------------------------
def flat_case(torch, fam, esize, seg, m, kind, cap):
    """fam: ("f", filter), ("s", filter, stride) or ("o", order, stride); cap: for the message"""
    t = esize - 1
    tag = "%r, esize %d, seg %d, m %d, %s, grid %s" % (fam, esize, seg, m, kind, cap)
    if fam[0] == "f":
        d = FL.gen(kind, esize, m, t, 100 * m + 10 * esize + fam[1])
        kw, y = dict(filt=fam[1], seg=seg), FL.forward(d, esize, fam[1], seg)
    elif fam[0] == "s":
        d = SL.gen(kind, esize, m, t, 100 * m + 10 * esize + fam[1] + fam[2], fam[2])
        kw, y = dict(filt=fam[1], stride=fam[2], seg=seg), SL.forward(d, esize, fam[1], seg, fam[2])
    else:
        d = OL.gen(kind, esize, m, t, 100 * m + 10 * esize + fam[1] + fam[2], fam[2])
        kw, y = dict(order=fam[1], stride=fam[2], seg=seg), OL.forward(d, esize, fam[1], seg, fam[2])
    planes, tail = PL.split(y, esize)
    split_join_flat(torch, d, esize, m, t, planes, tail, tag, **kw)


FLAT = {"fplanes": ([("f", f) for f in FL.FILTERS], ("wrap", "random")),
        "sfilter": ([("s", f, s) for s in S_STRIDES for f in FL.FILTERS], ("wrap", "random", "interleaved")),
        "ofilter": ([("o", k, s) for s in O_STRIDES for k in OL.ORDERS], ("wrap", "random", "smooth"))}


@pytest.mark.parametrize("seg", RESTARTS)
@pytest.mark.parametrize("esize", FL.ESIZES)
@pytest.mark.parametrize("family", sorted(FLAT))
def test_flat_split_join(torch_cuda, family, esize, seg, monkeypatch):
    fams, kinds = FLAT[family]
    for cap in CAPS:
        capped(monkeypatch, cap)
        for i, fam in enumerate(fams):
            flat_case(torch_cuda, fam, esize, seg, elements(seg), kinds[(i + (cap is not None)) % len(kinds)], cap)


@pytest.mark.parametrize("order,stride", [(2, 6), (3, 7)])
def test_order_join_with_128_tiles_to_a_segment(torch_cuda, order, stride, monkeypatch):
    """seg 65536, which test_gpu_fplanes.py has at stride 1: the carries of every level and class cross 127 tile edges"""
    for cap in CAPS:
        capped(monkeypatch, cap)
        flat_case(torch_cuda, ("o", order, stride), 4, 65536, elements(65536), "smooth" if cap else "random", cap)


# ---- the batched joins -----------------------------------------------------------------------------------------------------
B_CHUNKS = (448, 576, 1984)
B_GRIDS = (None, "3")                                          # LOOP_GRID of the batch files: 12 waves over the spans
# m[i], in elements: the lists of test_gpu_fplanes_batch.py / test_gpu_splanes_batch.py and of test_gpu_obatch.py, which end items mid-tile
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]
O_SIZES = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]


def batch_esize(family, chunk):
    """one width per (family, chunk); every family and every chunk sees all three"""
    return FL.ESIZES[(B_CHUNKS.index(chunk) + ("fbatch", "sbatch", "obatch").index(family)) % 3]


@pytest.mark.parametrize("chunk", B_CHUNKS)
def test_fbatch_split_join(torch_cuda, chunk, monkeypatch):
    esize = batch_esize("fbatch", chunk)
    datas = FBL.gen_items(esize, SIZES, 1000 * esize + chunk)
    for grid in B_GRIDS:
        capped(monkeypatch, grid)
        for name in ("cycle", "delta"):
            filters = FBL.assignments(len(datas), chunk + esize)[name]
            split_join_batch(torch_cuda, datas, esize, chunk, FBL.virtual_filtered(datas, filters, esize, chunk),
                             "fbatch esize %d, chunk %d, grid %s, filters %s" % (esize, chunk, grid, name), filters=filters, partial=grid is None)


@pytest.mark.parametrize("chunk", B_CHUNKS)
def test_sbatch_split_join(torch_cuda, chunk, monkeypatch):
    esize = batch_esize("sbatch", chunk)
    datas = FBL.gen_items(esize, SIZES, 1000 * esize + chunk)
    strides = SBL.stride_assignments(len(datas), chunk + esize)["cycle"]
    for grid in B_GRIDS:
        capped(monkeypatch, grid)
        for fname in ("cycle", "delta"):
            filters = SBL.filter_assignments(len(datas))[fname]
            split_join_batch(torch_cuda, datas, esize, chunk, SBL.virtual_filtered(datas, filters, strides, esize, chunk),
                             "sbatch esize %d, chunk %d, grid %s, strides cycle, filters %s" % (esize, chunk, grid, fname), filters=filters,
                             strides=strides, partial=grid is None)


@pytest.mark.parametrize("chunk", B_CHUNKS)
def test_obatch_split_join(torch_cuda, chunk, monkeypatch):
    """all delta under the cycling orders (1, 2, 3, ..), and the cycling filters under a random order assignment: with both
    cycling, a zigzag-delta item would always have order 2"""
    esize = batch_esize("obatch", chunk)
    count = len(O_SIZES)
    strides = OBL.stride_assignments(count)["cycle"]
    datas = OBL.gen_items(esize, O_SIZES, 1000 * esize + chunk, lambda i: strides[i])
    for grid in B_GRIDS:
        capped(monkeypatch, grid)
        for oname, fname in (("cycle", "delta"), ("random", "cycle")):
            orders = OBL.order_assignments(count, chunk + esize)[oname]
            filters = OBL.filter_assignments(count)[fname]
            monkeypatch.setattr(GP, "batch_calls", lambda filters=None, strides=None, orders=orders:
                                (trc.planes_split_obatch, trc.planes_join_obatch, (filters, strides, orders)))
            split_join_batch(torch_cuda, datas, esize, chunk, OBL.virtual_filtered(datas, filters, strides, orders, esize, chunk),
                             "obatch esize %d, chunk %d, grid %s, orders %s, strides cycle, filters %s" % (esize, chunk, grid, oname, fname),
                             filters=filters, strides=strides, partial=grid is None)


# ---- the histograms --------------------------------------------------------------------------------------------------------
H_SEGS = (448, 576, 1984)


@pytest.mark.parametrize("seg", H_SEGS)
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_histograms(torch_cuda, esize, seg, monkeypatch):
    """trc_planes_hist_dev, trc_planes_hist_stride_dev at strides 3 and 6 and trc_planes_hist_order_dev (all four orders) at strides
    3 and 7 against the models' bincounts, uncapped and with one workgroup"""
    torch, m = torch_cuda, elements(seg)
    for cap in CAPS:
        capped(monkeypatch, cap)
        tag = "esize %d, seg %d, m %d, grid %s" % (esize, seg, m, cap)
        d = FL.gen("walk", esize, m, esize - 1, 31 * m + esize)
        got, _ = device_hists(torch, esize, seg, 7, d=d)
        assert_hists(got, SL.hist3(d, esize, seg, 1), [m], 7, tag)
        for stride in (3, 6):
            d = SL.gen("interleaved", esize, m, esize - 1, 31 * m + esize, stride)
            got, _ = device_hists(torch, esize, seg, 7, d=d, strides=stride)
            assert_hists(got, SL.hist3(d, esize, seg, stride), [m], 7, tag + ", stride %d" % stride)
        for stride in (3, 7):
            d = OL.gen("smooth", esize, m, esize - 1, 31 * m + esize, stride)
            got = device_order_hists(torch, d, esize, stride, seg, 15).reshape(4, esize, 256)
            assert_order_hists(got, OL.hist4(d, esize, seg, stride).reshape(4, esize, 256), m, 15, tag + ", orders 15, stride %d" % stride)


# ---- the coded calls -------------------------------------------------------------------------------------------------------
C_FAMILIES = (("o", 2, 6), ("o", 3, 7), ("s", FL.ZDELTA, 6))


@pytest.mark.parametrize("fam", C_FAMILIES, ids=lambda f: "%s%d-s%d" % f)
@pytest.mark.parametrize("chunk", (576, 1984))
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S), ids=lambda c: trc.CODEC_NAMES[c])
def test_coded(torch_cuda, codec, chunk, fam, monkeypatch):
    """seg = chunk: directory, payload, totals and CDFs are those of the unfiltered planes call on the model-filtered input; the
    whole decode and two chunk ranges, one ending in the ragged last chunk, uncapped and with the six chunks on one workgroup"""
    torch, esize = torch_cuda, 4
    m = elements(chunk)
    kind, a, stride = fam
    if kind == "o":
        d = OL.gen("smooth", esize, m, esize - 1, 17 * esize + a + stride, stride)
        c, pc = coded_flat(torch, codec, esize, chunk, d, trc.OrderPlanesCoder, lambda: OL.forward(d, esize, a, chunk, stride), order=a, stride=stride)
    else:
        d = SL.gen("interleaved", esize, m, esize - 1, 17 * esize + a + stride, stride)
        c, pc = coded_flat(torch, codec, esize, chunk, d, trc.StridedPlanesCoder, lambda: SL.forward(d, esize, a, chunk, stride), filter=a, stride=stride)
    tag = "%s esize %d chunk %d %r" % (trc.CODEC_NAMES[codec], esize, chunk, fam)
    nch = c.nch
    assert nch == 6 and m % chunk != 0, tag
    assert_same_container(c, pc, esize, codec, tag)
    assert torch.equal(c.total, pc.total) and torch.equal(c.clen, pc.clen), tag + ": totals or directory"
    for cap in CAPS:
        capped(monkeypatch, cap)
        decodes_flat(torch, c, d, tag + ", grid %s" % cap)
        decodes_ranges_flat(torch, c, d, esize, chunk, ((1, 2), (nch - 3, 3)), tag + ", grid %s" % cap)
