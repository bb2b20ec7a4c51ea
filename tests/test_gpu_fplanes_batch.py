"""Batched byte planes with a filter per item on the MI355X: the filtered gathering split and the scanning, scattering join at the
edges of a thread's vector, a tile, a chunk, a span, an item and the grid-stride loop, under uniform and mixed filter assignments;
the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on VF, byte for byte); decode of item ranges.
As in test_gpu_planes_batch.py the items of a batch lie in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of
their own, every other device buffer is followed by a 512-byte guard of 0xA5, and every comparison is byte equality against the
numpy model (fplanes_batch_lib) or against the unbatched calls."""
import numpy as np
import pytest

import fplanes_batch_lib as FBL
import fplanes_lib as FL
import planes_batch_lib as BL
import planes_lib as PL
import trc
from test_gpu_planes_batch import Packed, assert_same_outputs, guarded, planes_reference, ranges

pytestmark = pytest.mark.gpu
GUARD = BL.GUARD
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
SHUFFLED = [SIZES[i] for i in np.random.default_rng(5).permutation(len(SIZES))]
CHUNKS = (256, 320, 512, 4096)          # 8-chunk spans / not a power of two, a span of 5 tiles / exactly one tile / 8 tiles: the carry
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
PRM = (4, 7)
CHUNK = 256
LOOP_GRID = 3
E_WORK = -3


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def pad_mask(sizes, esize, chunk, M):
    """True at the elements of V that are pad"""
    _, first = BL.plan(sizes, esize, chunk)
    mask = np.zeros(M, dtype=bool)
    for i, n in enumerate(sizes[:-1]):
        mask[first[i] * chunk + n // esize:first[i + 1] * chunk] = True
    return mask


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, order, name, partial=True):
    datas = FBL.gen_items(esize, order, 1000 * esize + chunk)
    count = len(datas)
    filters = FBL.assignments(count, chunk + esize)[name]
    src = Packed(torch, datas, seed=chunk)
    pl, first = BL.plan(src.sizes, esize, chunk)
    M = pl["m_total"]
    pitch = BL.up256(M)                                         # the smallest pitch the call takes
    planes, _ = PL.split(FBL.virtual_filtered(datas, filters, esize, chunk), esize)
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    d_planes, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_fbatch(src.items(), filters, count, esize, chunk, d_planes, pitch, d_table, tb)
    torch.cuda.synchronize()
    tag = "esize %d, chunk %d, filters %s" % (esize, chunk, name)
    exp = np.full(esize * pitch + GUARD, 0xA5, dtype=np.uint8)
    for k in range(esize):
        exp[k * pitch:k * pitch + M] = planes[k]
    assert np.array_equal(d_planes.cpu().numpy(), exp), tag + ": planes, their pad zeros or the bytes behind them"
    assert np.array_equal(src.buf.cpu().numpy(), src.img), tag + ": split changed its input"
    assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": split wrote behind its table"
    # the same planes with every pad byte 0xFF: what the join restores must not depend on the pad
    loud = exp.copy()
    mask = pad_mask(src.sizes, esize, chunk, M)
    assert int(mask.sum()) == pl["pad_elems"] > 0
    for k in range(esize):
        loud[k * pitch:k * pitch + M][mask] = 0xFF
    d_loud = torch.from_numpy(loud).to("cuda:0")
    # join, whole: every item back, every gap and the guard untouched
    for d_pl, what in ((d_planes, "zero pad"), (d_loud, "0xFF pad")):
        dst = Packed(torch, datas, seed=chunk, data=False)
        d_table2 = guarded(torch, tb)
        trc.planes_join_fbatch(d_pl, 0, pitch, dst.items(), filters, count, 0, count, esize, chunk, d_table2, tb)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), src.img), tag + ", " + what + ": join(split(x)) != x, or a gap or the guard was written"
        assert (d_table2.cpu().numpy()[tb:] == 0xA5).all()
    assert np.array_equal(d_planes.cpu().numpy(), exp) and np.array_equal(d_loud.cpu().numpy(), loud), tag + ": join changed the planes"
    if not partial:
        return
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        dst = Packed(torch, datas, seed=chunk, data=False)
        chunks = first[fi + ic] - first[fi]
        tbr = trc.lib().trc_planes_batch_table_bytes(ic, chunks)
        d_table3 = guarded(torch, tbr)
        items = dst.items(only)                                 # NULL outside the range
        trc.planes_join_fbatch(d_loud, first[fi] * chunk, pitch, items, filters, count, fi, ic, esize, chunk, d_table3, tbr)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag + " items (%d, %d)" % (fi, ic)
        assert (d_table3.cpu().numpy()[tbr:] == 0xA5).all()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join(torch_cuda, esize, chunk):
    for order in (SIZES, SHUFFLED):
        for name in ("delta", "xor", "cycle", "random"):
            split_join_case(torch_cuda, esize, chunk, order, name)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, chunk, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", str(LOOP_GRID))       # 3 workgroups: 12 waves over the spans, 768 threads over 10 000 vectors
    for name in ("delta", "xor", "cycle", "random"):
        split_join_case(torch_cuda, esize, chunk, SIZES, name)


def test_all_none_is_the_unfiltered_split(torch_cuda):
    torch = torch_cuda
    esize, chunk = 4, 320
    datas = FBL.gen_items(esize, SIZES, 77)
    src = Packed(torch, datas)
    count = len(datas)
    pl, _ = BL.plan(src.sizes, esize, chunk)
    pitch = BL.up256(pl["m_total"])
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    want, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_batch(src.items(), count, esize, chunk, want, pitch, d_table, tb)
    for filters in (None, 0, [0] * count):
        got = guarded(torch, esize * pitch)
        trc.planes_split_fbatch(src.items(), filters, count, esize, chunk, got, pitch, d_table, tb)
        assert torch.equal(got, want)
        dst = Packed(torch, datas, data=False)
        trc.planes_join_fbatch(got, 0, pitch, dst.items(), filters, count, 0, count, esize, chunk, d_table, tb)
        assert np.array_equal(dst.buf.cpu().numpy(), src.img)


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads
NAMES = ("delta", "xor", "cycle", "random")
_cache = {}


def coded(torch, codec, esize, name):
    """-> (Packed source, filters, PlanesBatchCoder holding its coded batch): computed once per key, shared, left unchanged"""
    key = (codec, esize, name)
    if key not in _cache:
        datas = FBL.gen_items(esize, W_SIZES, 50 + esize)
        filters = FBL.assignments(len(datas), 9 + esize)[name]
        src = Packed(torch, datas, seed=esize)
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters)
        bc.payload[:esize * bc.pitch] = 0x5A
        bc.encode()
        assert bc.guards_ok(), "encode wrote behind one of its buffers"
        assert np.array_equal(src.buf.cpu().numpy(), src.img), "encode changed its input"
        _cache[key] = (src, filters, bc)
    return _cache[key]


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    for name in NAMES:
        src, filters, bc = coded(torch, codec, esize, name)
        vf = FBL.virtual_filtered(src.datas, filters, esize, CHUNK)
        assert vf.size == bc.plan["n_virtual"] and bc.plan["pad_elems"] > 0
        pc = planes_reference(torch, codec, esize, vf)
        tag = "%s esize %d filters %s" % (trc.CODEC_NAMES[codec], esize, name)
        assert_same_outputs(torch, bc, pc, codec, esize, tag)
        for k in range(esize):
            total = bc.result(k)[2]
            assert (bc.payload[k * bc.pitch + total:k * bc.pitch + total + 64].cpu().numpy() == 0x5A).all(), tag + ": bytes behind payload %d" % k


@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("codec", CODECS)
def test_one_item_is_the_filtered_plain_call(torch_cuda, codec, filt):
    torch = torch_cuda
    esize, m = 2, 5 * CHUNK + 77                                # m % chunk != 0
    d = FL.gen("walk", esize, m, 0, 3)
    src = Packed(torch, [d])
    bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filt)
    bc.encode()
    assert bc.guards_ok()
    pc = trc.FilteredPlanesCoder(codec, d.size, esize, CHUNK, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, filter=filt)
    pc.encode(guarded(torch, d.size + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)])), d.size)
    assert pc.guards_ok()
    assert_same_outputs(torch, bc, pc, codec, esize, "%s filter %d one item" % (trc.CODEC_NAMES[codec], filt))
    dst = Packed(torch, [d], data=False)
    bc.decode(0, 1, out=dst.views())
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), src.img) and bc.guards_ok()


def raw_encode(bc, filters, work_bytes=None):
    st = bc.codec in trc.STATIC
    return trc.lib().trc_encode_fplanes_batch_dev(bc.codec, bc.items, filters, bc.count, bc.esize, bc.chunk, bc.cdf.data_ptr() if st else None,
                                                  bc.cdfnum, bc.status.data_ptr() if st else None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                                  bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes if work_bytes is None else work_bytes,
                                                  bc._stream())


@pytest.mark.parametrize("codec", CODECS)
def test_null_filters_is_the_unfiltered_batch(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    src = Packed(torch, FBL.gen_items(esize, W_SIZES, 50 + esize), seed=esize)
    want = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize)
    want.encode()                                               # trc_encode_planes_batch_dev
    for filters in (None, trc.planes_filters(0, want.count)):
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize)
        assert raw_encode(bc, filters) == 0
        assert_same_outputs(torch, bc, want, codec, esize, trc.CODEC_NAMES[codec] + (" NULL filters" if filters is None else " filters all NONE"))
        assert bc.guards_ok()


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_items(torch_cuda, codec, esize):
    torch = torch_cuda
    L = trc.lib()
    for name in ("cycle", "random", "delta"):
        src, filters, bc = coded(torch, codec, esize, name)
        count = bc.count
        for fi, ic in ranges(count):
            only = range(fi, fi + ic)
            dst = Packed(torch, src.datas, seed=esize, data=False)
            need = L.trc_planes_batch_range_work_bytes(codec, dst.items(only), count, esize, CHUNK, fi, ic)
            bc.range_work, bc.range_work_bytes = None, 0        # a workspace of exactly that size, guarded, for every range
            bc.decode(fi, ic, out=dst.views(only))
            assert bc.range_work_bytes == need > 0
            torch.cuda.synchronize()
            tag = "%s esize %d filters %s items (%d, %d)" % (trc.CODEC_NAMES[codec], esize, name, fi, ic)
            assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag
            assert bc.guards_ok(), tag
        assert np.array_equal(src.buf.cpu().numpy(), src.img)


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_workspace_one_byte_short(torch_cuda, codec):
    torch = torch_cuda
    esize = 2
    src, filters, bc = coded(torch, codec, esize, "cycle")
    L = trc.lib()
    outputs = (bc.clen, bc.payload, bc.total, bc.cdf, bc.status, bc.work)
    before = [x.clone() for x in outputs]
    assert raw_encode(bc, bc.filters, bc.work_bytes - 1) == E_WORK
    dst = Packed(torch, src.datas, seed=esize, data=False)
    for fi, ic in ((0, bc.count), (3, 1)):
        need = L.trc_planes_batch_range_work_bytes(codec, dst.items(), bc.count, esize, CHUNK, fi, ic)
        d_work = guarded(torch, need)
        st = codec in trc.STATIC
        assert L.trc_decode_fplanes_batch_dev(codec, bc.clen.data_ptr(), bc.payload.data_ptr(), dst.items(), bc.filters, bc.count, fi, ic, esize, CHUNK,
                                              bc.cdf.data_ptr() if st else None, bc.cdfnum, d_work.data_ptr(), need - 1, bc._stream()) == E_WORK
        torch.cuda.synchronize()
        assert (d_work.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its workspace"
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(0))), "a rejected call wrote to an item, a gap or the guard"
    for x, b in zip(outputs, before):
        assert torch.equal(x, b), "a rejected call changed the coded buffers or the encode workspace"


# ---- the torch helper --------------------------------------------------------------------------------------------------
def table_columns(torch):
    """the columns of a table at one element width: sorted ids, timestamps with small steps, float values, a short and a one-row column"""
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.cumsum(torch.randint(1, 200, (5000,), generator=g), 0).to(torch.int32)
    stamps = (1_700_000_000 + torch.cumsum(torch.randint(0, 3, (4097,), generator=g), 0)).to(torch.int32)
    values = torch.randn(3000, generator=g)
    return [t.to("cuda:0") for t in (ids, stamps, values, ids[:77].clone(), stamps[:1].clone())]


@pytest.mark.parametrize("filters", [trc.FILTER_ZDELTA, trc.FILTER_XOR, [1, 1, 0, 2, 1]])
def test_planes_batch_coder_with_filters(torch_cuda, filters):
    torch = torch_cuda
    tensors = table_columns(torch)
    keep = [t.clone() for t in tensors]
    bc = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=512, guard=GUARD, filters=filters)
    assert bc.esize == 4 and bc.count == 5 and list(bc.filters) == ([filters] * 5 if isinstance(filters, int) else filters)
    bc.encode()
    if not isinstance(filters, int):                            # ids and timestamps behind the delta, the floats as they are
        plain = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=512, guard=GUARD)
        plain.encode()
        assert 0 < bc.stored_bytes() < plain.stored_bytes(), "the delta of sorted ids and timestamps is meant to code shorter"
    for t in tensors:
        t.zero_()
    bc.decode(3, 1)                                             # one item into the encoded tensors
    torch.cuda.synchronize()
    for i, (t, k) in enumerate(zip(tensors, keep)):
        assert torch.equal(t.view(torch.uint8), (k if i == 3 else torch.zeros_like(k)).view(torch.uint8)), i
    out = [torch.empty_like(k) for k in keep]
    bc.decode(out=out)
    torch.cuda.synchronize()
    assert all(torch.equal(o.view(torch.uint8), k.view(torch.uint8)) for o, k in zip(out, keep)) and bc.guards_ok()
