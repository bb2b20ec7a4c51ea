"""Batched byte planes on the MI355X: the gathering split and the scattering join at the edges of a thread's vector, a chunk, an
item and the grid-stride loop; the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on the
virtual buffer, byte for byte); decode of item ranges; and the errors.  The items of a batch lie in ONE allocation with 16 to 48
bytes of 0xA5 between them and no slack of their own (planes_batch_lib), every other device buffer is followed by a 512-byte guard
of 0xA5, and every comparison is byte equality against numpy or against the unbatched calls."""
import numpy as np
import pytest

import planes_batch_lib as BL
import planes_lib as PL
import trc

pytestmark = pytest.mark.gpu
GUARD = BL.GUARD
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
CHUNKS = (256, 320, 4096)                                       # 320: 40 vectors per chunk, not a power of two
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
PRM = (4, 7)
CHUNK = 256
LOOP_GRID = 3


def ranges(count):
    return [(0, 1), (3, 1), (count - 1, 1), (2, 5), (0, count)]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def guarded(torch, nbytes, data=None):
    """a device buffer of nbytes (from `data`, else 0xA5 throughout) followed by the guard"""
    a = np.full(nbytes + GUARD, 0xA5, dtype=np.uint8)
    if data is not None:
        a[:nbytes] = data
    return torch.from_numpy(a).to("cuda:0")


class Packed:
    """the items of a batch in one device allocation (BL.offsets / BL.image), or -- data = False -- their places filled with 0xA5"""

    def __init__(self, torch, datas, seed=0, data=True):
        self.datas = datas
        self.sizes = [d.size for d in datas]
        self.offs, self.total = BL.offsets(self.sizes, seed)
        self.img = BL.image(datas if data else [None] * len(datas), self.offs, self.total)
        self.buf = torch.from_numpy(self.img).to("cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    def views(self, only=None):
        return BL.views(self.buf, self.offs, self.sizes, only)

    def items(self, only=None):
        return trc.planes_items([(v.data_ptr() if v is not None else None, n) for v, n in zip(self.views(only), self.sizes)])

    def expect(self, only=None):
        """the allocation with the items of `only` (default: all) in place and 0xA5 everywhere else"""
        return BL.image([d if only is None or i in only else None for i, d in enumerate(self.datas)], self.offs, self.total)


def batch_data(esize, order, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, m * esize, dtype=np.uint8) for m in order]


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, order):
    datas = batch_data(esize, order, 1000 * esize + chunk)
    src = Packed(torch, datas, seed=chunk)
    count = len(datas)
    pl, first = BL.plan(src.sizes, esize, chunk)
    got, got_first = trc.planes_batch_plan(src.items(), count, esize, chunk)
    assert got == pl and got_first == first
    M = pl["m_total"]
    pitch = BL.up256(M)                                         # the smallest pitch the call takes
    planes, _ = PL.split(BL.virtual(datas, esize, chunk), esize)
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    d_planes, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_batch(src.items(), count, esize, chunk, d_planes, pitch, d_table, tb)
    torch.cuda.synchronize()
    tag = "esize %d, chunk %d" % (esize, chunk)
    exp = np.full(esize * pitch + GUARD, 0xA5, dtype=np.uint8)
    for k in range(esize):
        exp[k * pitch:k * pitch + M] = planes[k]
    assert np.array_equal(d_planes.cpu().numpy(), exp), tag + ": planes, their pad zeros or the bytes behind them"
    assert np.array_equal(src.buf.cpu().numpy(), src.img), tag + ": split changed its input"
    assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": split wrote behind its table"
    # join, whole: every item back, every gap and the guard untouched
    dst = Packed(torch, datas, seed=chunk, data=False)
    d_table2 = guarded(torch, tb)
    trc.planes_join_batch(d_planes, 0, pitch, dst.items(), count, 0, count, esize, chunk, d_table2, tb)
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), src.img), tag + ": join(split(x)) != x, or a gap or the guard was written"
    assert np.array_equal(d_planes.cpu().numpy(), exp) and (d_table2.cpu().numpy()[tb:] == 0xA5).all()
    return src, d_planes, pitch, first


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join(torch_cuda, esize):
    shuffled = [SIZES[i] for i in np.random.default_rng(5).permutation(len(SIZES))]
    for chunk in CHUNKS:
        for order in (SIZES, shuffled):
            split_join_case(torch_cuda, esize, chunk, order)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", str(LOOP_GRID))       # 3 workgroups over more than 10 000 vectors
    for chunk in CHUNKS:
        split_join_case(torch_cuda, esize, chunk, SIZES)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_partial_join(torch_cuda, esize):
    torch = torch_cuda
    for chunk in (256, 320):
        src, d_planes, pitch, first = split_join_case(torch, esize, chunk, SIZES)
        count = len(SIZES)
        for fi, ic in ranges(count):
            only = range(fi, fi + ic)
            dst = Packed(torch, src.datas, seed=chunk, data=False)
            chunks = first[fi + ic] - first[fi]
            tb = trc.lib().trc_planes_batch_table_bytes(ic, chunks)
            d_table = guarded(torch, tb)
            items = dst.items(only)                             # NULL outside the range
            assert all((items[i].d_ptr is None) == (i not in only) for i in range(count))
            trc.planes_join_batch(d_planes, first[fi] * chunk, pitch, items, count, fi, ic, esize, chunk, d_table, tb)
            torch.cuda.synchronize()
            assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), "esize %d chunk %d items (%d, %d)" % (esize, chunk, fi, ic)
            assert (d_table.cpu().numpy()[tb:] == 0xA5).all()


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads


def weights_items(esize, sizes=W_SIZES):
    return [PL.weights(m, esize, seed=11 + i) for i, m in enumerate(sizes)]


_cache = {}


def coded(torch, codec, esize):
    """-> (Packed source, PlanesBatchCoder holding its coded batch): computed once per (codec, esize), shared, left unchanged"""
    key = (codec, esize)
    if key not in _cache:
        src = Packed(torch, weights_items(esize), seed=esize)
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize)
        bc.payload[:esize * bc.pitch] = 0x5A
        bc.encode()
        assert bc.guards_ok(), "encode wrote behind one of its buffers"
        assert np.array_equal(src.buf.cpu().numpy(), src.img), "encode changed its input"
        _cache[key] = (src, bc)
    return _cache[key]


def assert_same_outputs(torch, bc, pc, codec, esize, tag):
    """every output of the batch call against the planes call's: directory, totals, payloads, CDFs, statuses"""
    assert (bc.nch, bc.pitch) == (pc.nch, pc.pitch), tag
    assert torch.equal(bc.clen[:4 * esize * bc.nch], pc.clen[:4 * esize * pc.nch]), tag + ": d_clen"
    assert torch.equal(bc.total[:8 * esize], pc.total[:8 * esize]), tag + ": d_total"
    for k in range(esize):
        clen, payload, total = bc.result(k)
        exp_clen, exp_payload, exp_total = pc.result(k)
        assert total == exp_total and np.array_equal(clen, exp_clen) and np.array_equal(payload, exp_payload), tag + ": plane %d" % k
    if codec in trc.STATIC:
        assert torch.equal(bc.cdf[:2 * esize * trc.PLANES_CDF_STRIDE], pc.cdf[:2 * esize * trc.PLANES_CDF_STRIDE]), tag + ": d_cdf"
        assert torch.equal(bc.status[:4 * esize], pc.status[:4 * esize]), tag + ": d_status"
        assert all(bc.cdf_of(k)[1] == bc.plan["m_total"] for k in range(esize))


def planes_reference(torch, codec, esize, data):
    """trc_encode_planes_dev on `data` uploaded as one buffer"""
    pc = trc.PlanesCoder(codec, data.size, esize, CHUNK, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD)
    d_in = guarded(torch, data.size + trc.PAD, np.concatenate([data, np.zeros(trc.PAD, np.uint8)]))
    pc.encode(d_in, data.size)
    assert pc.guards_ok()
    return pc


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    src, bc = coded(torch, codec, esize)
    v = BL.virtual(src.datas, esize, CHUNK)
    assert v.size == bc.plan["n_virtual"] and bc.plan["pad_elems"] > 0
    pc = planes_reference(torch, codec, esize, v)
    tag = "%s esize %d" % (trc.CODEC_NAMES[codec], esize)
    assert_same_outputs(torch, bc, pc, codec, esize, tag)
    for k in range(esize):
        total = bc.result(k)[2]
        assert (bc.payload[k * bc.pitch + total:k * bc.pitch + total + 64].cpu().numpy() == 0x5A).all(), tag + ": bytes behind payload %d" % k


@pytest.mark.parametrize("codec", CODECS)
def test_one_item_is_the_plain_call(torch_cuda, codec):
    torch = torch_cuda
    esize, m = 2, 5 * CHUNK + 77                                # m % chunk != 0
    d = PL.weights(m, esize, seed=3)
    src = Packed(torch, [d])
    bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize)
    assert bc.plan == {"m_total": m, "n_virtual": d.size, "chunks": 6, "pitch": trc.planes_pitch(d.size, esize), "pad_elems": 0}
    bc.encode()
    assert bc.guards_ok()
    assert_same_outputs(torch, bc, planes_reference(torch, codec, esize, d), codec, esize, trc.CODEC_NAMES[codec] + " one item")
    dst = Packed(torch, [d], data=False)
    bc.decode(0, 1, out=dst.views())
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), src.img) and bc.guards_ok()


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_items(torch_cuda, codec, esize):
    torch = torch_cuda
    src, bc = coded(torch, codec, esize)
    count = bc.count
    L = trc.lib()
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        dst = Packed(torch, src.datas, seed=esize, data=False)
        out = dst.views(only)
        need = L.trc_planes_batch_range_work_bytes(codec, dst.items(only), count, esize, CHUNK, fi, ic)
        bc.range_work, bc.range_work_bytes = None, 0            # a workspace of exactly that size, guarded, for every range
        bc.decode(fi, ic, out=out)
        assert bc.range_work_bytes == need > 0
        torch.cuda.synchronize()
        tag = "%s esize %d items (%d, %d)" % (trc.CODEC_NAMES[codec], esize, fi, ic)
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag
        assert bc.guards_ok(), tag
    assert np.array_equal(src.buf.cpu().numpy(), src.img)


def test_single_item_of_many_in_a_small_workspace(torch_cuda):
    torch = torch_cuda
    esize, count = 2, 240
    sizes = [300 + 37 * (i % 9) for i in range(count)]
    datas = [PL.weights(m, esize, seed=100 + i) for i, m in enumerate(sizes)]
    src = Packed(torch, datas, seed=9)
    bc = trc.PlanesBatchCoder(trc.RCA, src.views(), CHUNK, guard=GUARD, esize=esize)
    bc.encode()
    L = trc.lib()
    whole = L.trc_planes_batch_range_work_bytes(trc.RCA, src.items(), count, esize, CHUNK, 0, count)
    for i in (0, 123, count - 1):
        dst = Packed(torch, datas, seed=9, data=False)
        one = L.trc_planes_batch_range_work_bytes(trc.RCA, dst.items(range(i, i + 1)), count, esize, CHUNK, i, 1)
        assert 0 < one < whole and one < bc.work_bytes
        bc.range_work, bc.range_work_bytes = None, 0
        bc.decode(i, 1, out=dst.views(range(i, i + 1)))
        assert bc.range_work_bytes == one
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(i, i + 1))), "item %d of %d" % (i, count)
    assert bc.guards_ok()


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_mixed_raw_and_coded_chunks(torch_cuda, codec):
    """uniform-random items (stored raw) beside constant items (coded to almost nothing) in one batch"""
    torch = torch_cuda
    esize = 4
    rng = np.random.default_rng(2)
    sizes = [700, 256, 1025, 300, 4096, 9]
    datas = [rng.integers(0, 256, m * esize, dtype=np.uint8) if i % 2 == 0 else np.full(m * esize, 0x3C + i, dtype=np.uint8) for i, m in enumerate(sizes)]
    src = Packed(torch, datas, seed=4)
    bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, guard=GUARD, esize=esize)
    bc.encode()
    assert_same_outputs(torch, bc, planes_reference(torch, codec, esize, BL.virtual(datas, esize, CHUNK)), codec, esize, "mixed")
    M = bc.plan["m_total"]
    lens = np.minimum(CHUNK, M - np.arange(0, M, CHUNK))
    for k in range(esize):
        clen = bc.result(k)[0]
        assert int((clen == lens).sum()) and int((clen < lens).sum()), "plane %d is meant to mix raw and coded chunks" % k
    dst = Packed(torch, datas, seed=4, data=False)
    bc.decode(out=dst.views())
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), src.img) and bc.guards_ok()


# ---- errors ------------------------------------------------------------------------------------------------------------
def raw_encode(bc, codec, items, count, work_bytes=None):
    st = (codec & 0xff) in trc.STATIC
    return trc.lib().trc_encode_planes_batch_dev(codec, items, count, bc.esize, bc.chunk, bc.cdf.data_ptr() if st else None, bc.cdfnum,
                                                 bc.status.data_ptr() if st else None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                                 bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes if work_bytes is None else work_bytes,
                                                 bc._stream())


def raw_decode(bc, codec, items, count, fi, ic, d_work, work_bytes):
    return trc.lib().trc_decode_planes_batch_dev(codec, bc.clen.data_ptr(), bc.payload.data_ptr(), items, count, fi, ic, bc.esize, bc.chunk,
                                                 bc.cdf.data_ptr() if (codec & 0xff) in trc.STATIC else None, bc.cdfnum,
                                                 d_work.data_ptr(), work_bytes, bc._stream())


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize = 2
    src, bc = coded(torch, codec, esize)
    count, L = bc.count, trc.lib()
    E_ARG, E_WORK = -1, -3
    outputs = (bc.clen, bc.payload, bc.total, bc.cdf, bc.status, bc.work)
    before = [x.clone() for x in outputs]
    dst = Packed(torch, src.datas, seed=esize, data=False)
    need = L.trc_planes_batch_range_work_bytes(codec, dst.items(), count, esize, CHUNK, 0, count)
    d_work = guarded(torch, need)

    def items_with(i, ptr=None, n=None):
        pairs = [(v.data_ptr(), s) for v, s in zip(dst.views(), dst.sizes)]
        pairs[i] = (pairs[i][0] if ptr is None else ptr, pairs[i][1] if n is None else n)
        return trc.planes_items(pairs)
    base2 = dst.views()[2].data_ptr()
    bad = [(items_with(2, ptr=base2 + 8), count, "aligned"),                   # a misaligned item pointer
           (items_with(2, n=dst.sizes[2] + 1), count, "whole number"),          # n[i] % esize != 0
           (dst.items(), 0, "items")]                                          # count == 0
    for items, cnt, text in bad:
        assert raw_encode(bc, codec, items, cnt) == E_ARG and text in L.trc_last_error().decode(), text
        assert raw_decode(bc, codec, items, cnt, 0, cnt, d_work, need) == E_ARG and text in L.trc_last_error().decode(), text
    assert L.trc_planes_batch_range_work_bytes(codec, items_with(2, ptr=base2 + 8), count, esize, CHUNK, 0, count) == 0
    # a misaligned or NULL pointer outside the requested range is not looked at: checked with a decode that runs, below
    assert raw_encode(bc, codec, dst.items(), count, bc.work_bytes - 1) == E_WORK
    assert raw_decode(bc, codec, dst.items(), count, 0, count, d_work, need - 1) == E_WORK
    one = L.trc_planes_batch_range_work_bytes(codec, dst.items(), count, esize, CHUNK, 3, 1)
    assert raw_decode(bc, codec, dst.items(), count, 3, 1, d_work, one - 1) == E_WORK
    for low4 in (trc.RCA4, trc.RC4):
        assert raw_encode(bc, low4, dst.items(), count) == E_ARG and "low four bits" in L.trc_last_error().decode()
        assert raw_decode(bc, low4, dst.items(), count, 0, count, d_work, need) == E_ARG and "low four bits" in L.trc_last_error().decode()
    for flag in (trc.DIR_READY, trc.TABLES_READY):
        assert raw_encode(bc, codec | flag, dst.items(), count) == E_ARG
        assert raw_decode(bc, codec | flag, dst.items(), count, 0, count, d_work, need) == E_ARG
    for fi, ic in ((0, count + 1), (count, 1), (count + 1, 0), (3, count - 2)):  # first_item + item_count > count
        assert raw_decode(bc, codec, dst.items(), count, fi, ic, d_work, need) == E_ARG, (fi, ic)
        tb = L.trc_planes_batch_table_bytes(count, bc.nch)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_batch(bc.work, 0, bc.pitch, dst.items(), count, fi, ic, esize, CHUNK, d_work, tb)
    assert raw_decode(bc, codec, dst.items(), count, 4, 0, d_work, need) == 0   # item_count 0: TRC_OK, nothing enqueued
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(0))), "a rejected call wrote to an item, a gap or the guard"
    assert (d_work.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its workspace"
    for x, b in zip(outputs, before):
        assert torch.equal(x, b), "a rejected call changed the coded buffers or the encode workspace"
    assert bc.guards_ok() and np.array_equal(src.buf.cpu().numpy(), src.img)
    # ... and the decode that does run with a misaligned pointer outside its range
    assert raw_decode(bc, codec, items_with(2, ptr=base2 + 8), count, 3, 2, d_work, need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(3, 5)))
    assert (d_work.cpu().numpy()[need:] == 0xA5).all()


# ---- the torch helper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,codec", [("bfloat16", trc.RCA), ("float32", trc.ANS4S)])
def test_planes_batch_coder_round_trips_tensors(torch_cuda, dtype, codec):
    torch = torch_cuda
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cpu").manual_seed(1)
    shapes = [(3,), (64, 65), (1,), (257, 16), (4096,), (7, 11, 13), (5000,)]
    tensors = [(0.02 * torch.randn(s, generator=g)).to(dt).to("cuda:0") for s in shapes]
    keep = [t.clone() for t in tensors]
    bc = trc.PlanesBatchCoder(codec, tensors, chunk=512, guard=GUARD)
    assert bc.esize == tensors[0].element_size() and bc.count == len(shapes)
    bc.encode()
    assert 0 < bc.stored_bytes() <= bc.plan["n_virtual"] + bc.esize * (4 * bc.nch + 514), "stored more than raw chunks, directories and CDFs"
    for t in tensors:
        t.zero_()
    bc.decode(2, 3)                                             # items 2, 3, 4 into the encoded tensors
    torch.cuda.synchronize()
    for i, (t, k) in enumerate(zip(tensors, keep)):
        assert torch.equal(t.view(torch.uint8), (k if 2 <= i < 5 else torch.zeros_like(k)).view(torch.uint8)), i
    out = [torch.empty_like(k) for k in keep]
    bc.decode(out=out)
    torch.cuda.synchronize()
    assert all(torch.equal(o.view(torch.uint8), k.view(torch.uint8)) for o, k in zip(out, keep)) and bc.guards_ok()
