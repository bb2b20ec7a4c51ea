"""Batched byte planes with a base per item on the MI355X: the gathering split and the elementwise, scattering join against bases at
the edges of a thread's vector, a chunk, an item and the grid-stride loop, under uniform and mixed filter assignments, by item range
and in place; the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on the virtual buffer of the
items filtered against their bases, byte for byte); decode of item ranges and in place; argument errors.  Items and bases each lie
in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of their own; every other device buffer is followed by a
512-byte guard of 0xA5; every comparison is byte equality against the numpy model (bplanes_lib)."""
import numpy as np
import pytest

import bplanes_lib as BP
import fplanes_batch_lib as FBL
import planes_batch_lib as BL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, GUARD, PRM, Packed, decodes_whole_batch, encode_contract_batch, first_diff, guarded, ranges, up256

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
CHUNKS = (256, 320, 4096)
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
NAMES = ("delta", "xor", "cycle", "random")


def base_views(bsrc, filters, only=None):
    """the bases of the filtered items of `only` (default: all); None for an unfiltered item and outside the range"""
    return [v if f != BP.NONE and (only is None or i in only) else None for i, (v, f) in enumerate(zip(bsrc.views(), filters))]


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, name, partial=True):
    datas, bases = BP.gen_batch(esize, SIZES, 1000 * esize + chunk)
    count = len(datas)
    filters = FBL.assignments(count, chunk + esize)[name]
    tag = "esize %d, chunk %d, filters %s" % (esize, chunk, name)
    src, bsrc = Packed(torch, datas, seed=chunk), Packed(torch, bases, seed=chunk + 1)
    pl, first = BL.plan(src.sizes, esize, chunk)
    M = pl["m_total"]
    pitch = up256(M)
    planes, _ = PL.split(BP.virtual_batch(datas, bases, filters, esize, chunk), esize)
    tb = trc.lib().trc_planes_bbatch_table_bytes(count, pl["chunks"])
    d_planes, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_bbatch(src.items(), base_views(bsrc, filters), filters, count, esize, chunk, d_planes, pitch, d_table, tb)
    torch.cuda.synchronize()
    exp = np.full(esize * pitch + GUARD, 0xA5, dtype=np.uint8)
    for k in range(esize):
        exp[k * pitch:k * pitch + M] = planes[k]
    got = d_planes.cpu().numpy()
    assert np.array_equal(got, exp), tag + ": planes, their pad zeros or the bytes behind them (first difference at %d)" % first_diff(got, exp)
    assert src.unchanged() and bsrc.unchanged(), tag + ": split changed its input or a base"
    assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": split wrote behind its table"
    # join, whole: every item back, every gap and the guard untouched, the bases unchanged
    dst = src.blank()
    d_table2 = guarded(torch, tb)
    trc.planes_join_bbatch(d_planes, 0, pitch, dst.items(), base_views(bsrc, filters), filters, count, 0, count, esize, chunk, d_table2, tb)
    torch.cuda.synchronize()
    got = dst.buf.cpu().numpy()
    assert np.array_equal(got, src.img), tag + ": join(split(x)) != x, or a gap or the guard was written (first difference at byte %d)" % first_diff(got, src.img)
    assert (d_table2.cpu().numpy()[tb:] == 0xA5).all() and bsrc.unchanged(), tag + ": join wrote behind its table or to a base"
    # in place: the bases' own allocation is where the items go (unfiltered items are written there as well)
    inp = Packed(torch, bases, seed=chunk + 1)
    trc.planes_join_bbatch(d_planes, 0, pitch, inp.items(), inp.views(), filters, count, 0, count, esize, chunk, d_table2, tb)
    torch.cuda.synchronize()
    want = BL.image(datas, inp.offs, inp.total)
    got = inp.buf.cpu().numpy()
    assert np.array_equal(got, want), tag + ": the join in place (first difference at byte %d)" % first_diff(got, want)
    assert np.array_equal(d_planes.cpu().numpy(), exp), tag + ": join changed the planes"
    if not partial:
        return
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        dst = src.blank()
        tbr = trc.lib().trc_planes_bbatch_table_bytes(ic, first[fi + ic] - first[fi])
        d_table3 = guarded(torch, tbr)
        trc.planes_join_bbatch(d_planes, first[fi] * chunk, pitch, dst.items(only), base_views(bsrc, filters, only), filters, count, fi, ic, esize, chunk,
                               d_table3, tbr)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag + " items (%d, %d)" % (fi, ic)
        assert (d_table3.cpu().numpy()[tbr:] == 0xA5).all(), tag + " items (%d, %d): join wrote behind its table" % (fi, ic)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join(torch_cuda, esize, chunk):
    for name in NAMES:
        split_join_case(torch_cuda, esize, chunk, name)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", "3")                  # 768 threads over 10 000 vectors
    for name in ("cycle", "delta"):
        split_join_case(torch_cuda, esize, 256, name, partial=False)


def test_all_none_is_the_unfiltered_split(torch_cuda):
    torch = torch_cuda
    esize, chunk = 4, 320
    datas, _ = BP.gen_batch(esize, SIZES, 77)
    src = Packed(torch, datas)
    count = len(datas)
    pl, _ = BL.plan(src.sizes, esize, chunk)
    pitch = up256(pl["m_total"])
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])          # (the unfiltered call's table is enough)
    want, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_batch(src.items(), count, esize, chunk, want, pitch, d_table, tb)
    for filters in (None, 0, [0] * count):
        got = guarded(torch, esize * pitch)
        trc.planes_split_bbatch(src.items(), None, filters, count, esize, chunk, got, pitch, d_table, tb)
        assert torch.equal(got, want)
        dst = Packed(torch, datas, data=False)
        trc.planes_join_bbatch(got, 0, pitch, dst.items(), None, filters, count, 0, count, esize, chunk, d_table, tb)
        assert np.array_equal(dst.buf.cpu().numpy(), src.img)


def test_argument_errors_write_nothing(torch_cuda):
    torch = torch_cuda
    esize, chunk = 4, 256
    datas, bases = BP.gen_batch(esize, [300, 5, 1000], 5)
    src, bsrc = Packed(torch, datas), Packed(torch, bases, seed=1)
    pl, _ = BL.plan(src.sizes, esize, chunk)
    pitch = up256(pl["m_total"])
    tb = trc.lib().trc_planes_bbatch_table_bytes(3, pl["chunks"])
    d_planes, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    bv = bsrc.views()
    L = trc.lib()
    cases = [([1, 3, 0], bv, "item 1: filter 3"), ([1, 2, 1], [bv[0], None, bv[2]], "item 1"), ([0, 0, 2], [None, None, bv[2][8:]], "item 2"),
             ([1, 0, 0], None, "item 0")]
    for filters, b, text in cases:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_bbatch(src.items(), b, filters, 3, esize, chunk, d_planes, pitch, d_table, tb)
        assert text in L.trc_last_error().decode()
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_bbatch(d_planes, 0, pitch, src.items(), b, filters, 3, 0, 3, esize, chunk, d_table, tb)
        assert text in L.trc_last_error().decode()
    with pytest.raises(trc.TrcError, match="rc=-3"):            # the unfiltered batch's table is one array short
        trc.planes_split_bbatch(src.items(), bv, [1, 1, 1], 3, esize, chunk, d_planes, pitch, d_table, tb - 256)
    trc.planes_join_bbatch(d_planes, 0, pitch, src.items(), [bv[0], None, None], [1, 0, 2], 3, 0, 0, esize, chunk, d_table, tb)      # no item: TRC_OK
    trc.planes_join_bbatch(d_planes, 0, pitch, src.blank().items(range(1, 2)), None, [1, 0, 2], 3, 1, 1, esize, chunk, d_table, tb)     # bases outside the range are not looked at
    torch.cuda.synchronize()
    assert src.unchanged() and bsrc.unchanged()


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads
_cache = {}


def coded(torch, codec, esize, name):
    """-> (Packed source, Packed bases, filters, PlanesBatchCoder holding the coded batch, the model's virtual buffer): once per key"""
    key = (codec, esize, name)
    if key not in _cache:
        datas, bases = BP.gen_batch(esize, W_SIZES, 50 + esize)
        filters = FBL.assignments(len(datas), 9 + esize)[name]
        src, bsrc = Packed(torch, datas, seed=esize), Packed(torch, bases, seed=esize + 1)
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters, bases=base_views(bsrc, filters))
        bc.payload[:esize * bc.pitch] = 0x5A
        bc.encode()
        assert bc.guards_ok(), "encode wrote behind one of its buffers"
        assert src.unchanged() and bsrc.unchanged(), "encode changed its input or a base"
        _cache[key] = (src, bsrc, filters, bc, BP.virtual_batch(datas, bases, filters, esize, CHUNK))
    return _cache[key]


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract_and_decode(torch_cuda, codec, esize):
    torch = torch_cuda
    L = trc.lib()
    for name in ("cycle", "delta") if codec != trc.RCA else NAMES:
        src, bsrc, filters, bc, virtual = coded(torch, codec, esize, name)
        tag = "%s esize %d filters %s" % (trc.CODEC_NAMES[codec], esize, name)
        encode_contract_batch(torch, src, bc, codec, esize, virtual, tag)
        decodes_whole_batch(torch, src, bc, tag)
        for fi, ic in ranges(bc.count):                         # each range in a fresh workspace of exactly the required size
            only = range(fi, fi + ic)
            dst = src.blank()
            need = L.trc_planes_bbatch_range_work_bytes(codec, dst.items(only), bc.count, esize, bc.chunk, fi, ic)
            bc.range_work, bc.range_work_bytes = None, 0
            bc.decode(fi, ic, out=dst.views(only), bases=base_views(bsrc, filters, only))
            assert bc.range_work_bytes == need > 0, "%s items (%d, %d): a range workspace of %d bytes, required %d" % (tag, fi, ic, bc.range_work_bytes, need)
            torch.cuda.synchronize()
            assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), "%s items (%d, %d)" % (tag, fi, ic)
            assert bc.guards_ok()
        assert src.unchanged() and bsrc.unchanged(), tag + ": decode changed the source or a base"


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_decode_in_place_and_workspace(torch_cuda, codec):
    """the bases' own allocation becomes the items; a workspace one byte short is TRC_E_WORK and writes nothing"""
    torch = torch_cuda
    esize = 2
    src, bsrc, filters, bc, _ = coded(torch, codec, esize, "cycle")
    inp = Packed(torch, bsrc.datas, seed=esize + 1)
    L = trc.lib()
    need = L.trc_planes_bbatch_range_work_bytes(codec, inp.items(), bc.count, esize, bc.chunk, 0, bc.count)
    d_work = guarded(torch, need)
    args = (bc.codec, bc.clen.data_ptr(), bc.payload.data_ptr(), inp.items(), trc.planes_bases(inp.views(), bc.count), bc.filters, bc.count, 0, bc.count,
            esize, bc.chunk, bc.cdf.data_ptr() if codec in trc.STATIC else None, bc.cdfnum, d_work.data_ptr())
    assert L.trc_decode_bplanes_batch_dev(*args, need - 1, bc._stream()) == -3
    torch.cuda.synchronize()
    assert inp.unchanged() and (d_work.cpu().numpy() == 0xA5).all(), "a rejected call wrote"
    assert L.trc_encode_bplanes_batch_dev(bc.codec, bc.items, bc.bases, bc.filters, bc.count, esize, bc.chunk, bc.cdf.data_ptr() if codec in trc.STATIC else None,
                                          bc.cdfnum, bc.status.data_ptr() if codec in trc.STATIC else None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                          bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes - 1, bc._stream()) == -3
    bc.decode(out=inp.views(), bases=inp.views())
    torch.cuda.synchronize()
    assert np.array_equal(inp.buf.cpu().numpy(), BL.image(src.datas, inp.offs, inp.total)), "the decode in place"
    assert bc.guards_ok()


def test_planes_batch_coder_rules(torch_cuda):
    torch = torch_cuda
    g = torch.Generator(device="cpu").manual_seed(1)
    base = [torch.randn(n, generator=g).to(torch.bfloat16).to("cuda:0") for n in (5000, 77, 4097)]
    new = [(b.float() + 1e-4 * torch.randn(b.numel(), generator=g).to("cuda:0")).to(torch.bfloat16) for b in base]
    keep = [t.clone() for t in new]
    with pytest.raises(ValueError):
        trc.PlanesBatchCoder(trc.RCA, new, chunk=512, filters=1, bases=base, strides=2)
    with pytest.raises(ValueError):
        trc.PlanesBatchCoder(trc.RCA, new, chunk=512, filters="auto", bases=base)
    bc = trc.PlanesBatchCoder(trc.RCA, new, chunk=512, guard=GUARD, filters=[1, 0, 2], bases=[base[0], None, base[2]])
    bc.encode()
    plain = trc.PlanesBatchCoder(trc.RCA, new, chunk=512, guard=GUARD)
    plain.encode()
    print("bf16 fine-tune of 3 tensors: planes %d bytes, against the bases %d" % (plain.stored_bytes(), bc.stored_bytes()))
    assert 0 < bc.stored_bytes() < 0.8 * plain.stored_bytes(), "the delta against the base is meant to code shorter"
    with pytest.raises(trc.TrcError, match="no place for a base"):
        bc.pack()
    for t in new:
        t.zero_()
    bc.decode()
    torch.cuda.synchronize()
    assert all(torch.equal(t.view(torch.uint8), k.view(torch.uint8)) for t, k in zip(new, keep)) and bc.guards_ok()
