"""Batched byte planes with a filter, a stride and a predictor order per item on the MI355X: the gathering split with its reach of
1 .. 3 vectors and the scanning join with its levels at the edges of a thread's vector, the reach, a tile, a chunk, a span, an item
and the grid-stride loop, under uniform and mixed order, stride and filter assignments; the routing of order 1 to the strided batch;
the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on VO, byte for byte); decode of item ranges;
the calls at their documented minimum buffers in the audited arena; the histograms of orders 0 .. 3 per item and the order advisor on
them; the TRCU container; the torch helper; the harness.
Buffers, guards and comparisons are those of test_gpu_splanes_batch.py (gpu_planes.py, gpu_planes_arena.py); every comparison is
byte equality against the numpy model (obatch_lib) or against the unbatched calls."""
import struct

import numpy as np
import pytest

import gpu_arena as GA
import gpu_planes as GP
import gpu_planes_arena as P
import obatch_lib as OBL
import oplanes_lib as OL
import planes_batch_lib as BL
import planes_container_lib as CL
import planes_lib as PL
import planes_matrix_lib as PM
import splanes_lib as SL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (CHUNK, GUARD, PRM, Guarded, Packed, assert_same_outputs, decode_items_batch, decodes_whole_batch, encode_contract_batch,
                        guarded, item_ranges, padded, split_join_batch, trcfile, workspace_one_byte_short)

pytestmark = pytest.mark.gpu
# m[i], in elements: around 8, 16 and 24 the reach of 1, 2 and 3 vectors; then a tile, a chunk of each length, a span, the grid
SIZES = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]
SHUFFLED = [SIZES[i] for i in np.random.default_rng(5).permutation(len(SIZES))]
CHUNKS = (256, 320, 512, 4096)          # 8-chunk spans, triples mixed in a tile / 3, 6, 7 do not divide it / exactly one tile / 8 tiles: the carry
ORDER_NAMES = OBL.ORDER_NAMES
STRIDE_NAMES = ("1", "3", "8", "cycle")
FILTER_NAMES = ("delta", "cycle")
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
LOOP_GRID = 3


def obatch_calls(orders):
    """gpu_planes.batch_calls for the ordered pair: split_join_batch then runs trc_planes_split_obatch_dev / _join_obatch_dev"""
    return lambda filters=None, strides=None: (trc.planes_split_obatch, trc.planes_join_obatch, (filters, strides, orders))


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, monkeypatch, esize, chunk, oname, sname, fname, partial):
    count = len(SHUFFLED)
    strides = OBL.stride_assignments(count)[sname]
    orders = OBL.order_assignments(count, chunk + esize)[oname]
    filters = OBL.filter_assignments(count)[fname]
    datas = OBL.gen_items(esize, SHUFFLED, 1000 * esize + chunk, lambda i: strides[i])      # "random", "smooth", "wrap", "ones" in turn
    monkeypatch.setattr(GP, "batch_calls", obatch_calls(orders))
    split_join_batch(torch, datas, esize, chunk, OBL.virtual_filtered(datas, filters, strides, orders, esize, chunk),
                     "esize %d, chunk %d, orders %s, strides %s, filters %s" % (esize, chunk, oname, sname, fname), filters=filters, strides=strides,
                     partial=partial)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join(torch_cuda, esize, chunk, monkeypatch):
    for oname in ORDER_NAMES:
        for sname in STRIDE_NAMES:
            for fname in FILTER_NAMES:
                split_join_case(torch_cuda, monkeypatch, esize, chunk, oname, sname, fname, partial=(fname == "cycle") == (oname in ("cycle", "2")))


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", str(LOOP_GRID))       # 3 workgroups: 12 waves over the spans, 768 threads over 10 000 vectors
    for chunk, oname, sname, fname in ((256, "cycle", "cycle", "cycle"), (4096, "random", "3", "delta"), (320, "3", "8", "delta")):
        split_join_case(torch_cuda, monkeypatch, esize, chunk, oname, sname, fname, partial=False)


def test_order_one_is_the_strided_batch(torch_cuda):
    """orders None, 1 and [1] * count, and any order on items without the zigzag delta, give the planes of trc_planes_split_sbatch_dev"""
    torch = torch_cuda
    esize, chunk = 4, 320
    count = len(SIZES)
    datas = OBL.gen_items(esize, SIZES, 77)
    src = Packed(torch, datas)
    pl, _ = BL.plan(src.sizes, esize, chunk)
    pitch = BL.up256(pl["m_total"])
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    filters = OBL.filter_assignments(count)["cycle"]
    strides = OBL.stride_assignments(count)["cycle"]
    want, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_sbatch(src.items(), filters, strides, count, esize, chunk, want, pitch, d_table, tb)
    others = [1 if f == SL.ZDELTA else 3 for f in filters]      # an order above 1 where there is no zigzag delta: no effect
    for orders in (None, 1, [1] * count, others):
        got = guarded(torch, esize * pitch)
        trc.planes_split_obatch(src.items(), filters, strides, orders, count, esize, chunk, got, pitch, d_table, tb)
        assert torch.equal(got, want), orders
        dst = Packed(torch, datas, data=False)
        trc.planes_join_obatch(got, 0, pitch, dst.items(), filters, strides, orders, count, 0, count, esize, chunk, d_table, tb)
        assert np.array_equal(dst.buf.cpu().numpy(), src.img), orders
    plain = guarded(torch, esize * pitch)
    trc.planes_split_batch(src.items(), count, esize, chunk, plain, pitch, d_table, tb)
    got = guarded(torch, esize * pitch)
    trc.planes_split_obatch(src.items(), 0, 7, 3, count, esize, chunk, got, pitch, d_table, tb)
    assert torch.equal(got, plain)
    # the coded calls likewise: every output of the ordered call with orders 1 is the strided call's
    cdatas = OBL.gen_items(esize, W_SIZES, 9)
    csrc = Packed(torch, cdatas, seed=esize)
    f8, s8 = OBL.filter_assignments(8)["cycle"], OBL.stride_assignments(8)["cycle"]
    ref = trc.PlanesBatchCoder(trc.RCA, csrc.views(), CHUNK, guard=GUARD, esize=esize, filters=f8, strides=s8)
    ref.encode()
    for orders in (1, [1 if f == SL.ZDELTA else 2 for f in f8]):
        bc = trc.PlanesBatchCoder(trc.RCA, csrc.views(), CHUNK, guard=GUARD, esize=esize, filters=f8, strides=s8, orders=orders)
        assert not bc.ordered() and bc.strided()
        bc.encode()
        assert_same_outputs(torch, bc, ref, trc.RCA, esize, "orders %r" % (orders,))
        st = bc.codec in trc.STATIC
        rc = trc.lib().trc_encode_oplanes_batch_dev(bc.codec, bc.items, bc.filters, bc.strides, bc.orders, bc.count, esize, CHUNK, None, 0, None, bc.clen.data_ptr(),
                                                    bc.payload.data_ptr(), bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes, bc._stream())
        assert rc == 0 and not st
        assert_same_outputs(torch, bc, ref, trc.RCA, esize, "trc_encode_oplanes_batch_dev, orders %r" % (orders,))


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads (the batch of test_gpu_splanes_batch.py)
_coded = {}


def coded(torch, codec, esize, oname):
    """-> (Packed source, filters, strides, orders, PlanesBatchCoder holding its coded batch): computed once per key, shared, left unchanged"""
    key = (codec, esize, oname)
    if key not in _coded:
        count = len(W_SIZES)
        strides = OBL.stride_assignments(count)["cycle" if oname in ("cycle", "random") else "3" if oname == "2" else "1"]
        orders = OBL.order_assignments(count, 9 + esize)[oname]
        filters = OBL.filter_assignments(count)["delta"]
        if oname == "cycle":
            filters = [1, 1, 1, 2, 1, 0, 1, 1]                  # orders 1, 2 and 3 meet the zigzag delta, next to an xor item and one without a filter
        datas = OBL.gen_items(esize, W_SIZES, 50 + esize, lambda i: strides[i])
        src = Packed(torch, datas, seed=esize)
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters, strides=strides, orders=orders)
        bc.payload[:esize * bc.pitch] = 0x5A
        bc.encode()
        assert bc.ordered() and bc.guards_ok() and src.unchanged(), "%s esize %d orders %s" % (trc.CODEC_NAMES[codec], esize, oname)
        _coded[key] = (src, filters, strides, orders, bc)
    return _coded[key]


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    for oname in ORDER_NAMES:
        src, filters, strides, orders, bc = coded(torch, codec, esize, oname)
        encode_contract_batch(torch, src, bc, codec, esize, OBL.virtual_filtered(src.datas, filters, strides, orders, esize, CHUNK),
                              "%s esize %d orders %s" % (trc.CODEC_NAMES[codec], esize, oname))


@pytest.mark.parametrize("stride", (1, 3, 8))
@pytest.mark.parametrize("order", (2, 3))
@pytest.mark.parametrize("codec", CODECS)
def test_one_item_is_the_order_plain_call(torch_cuda, codec, order, stride):
    torch = torch_cuda
    esize, m = (2, 4, 8)[(order + stride) % 3], 5 * CHUNK + 77  # m % chunk != 0
    d = OL.gen("smooth", esize, m, 0, 3, stride)
    src = Packed(torch, [d])
    bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=SL.ZDELTA, strides=stride, orders=order)
    bc.encode()
    assert bc.guards_ok() and bc.ordered()
    pc = trc.OrderPlanesCoder(codec, d.size, esize, CHUNK, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, order=order, stride=stride)
    pc.encode(padded(torch, d), d.size)
    assert pc.guards_ok()
    tag = "%s order %d stride %d one item" % (trc.CODEC_NAMES[codec], order, stride)
    assert_same_outputs(torch, bc, pc, codec, esize, tag)
    decodes_whole_batch(torch, src, bc, tag)


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_items(torch_cuda, codec, esize):
    torch = torch_cuda
    for oname in ("cycle", "random", "3"):
        src, filters, strides, orders, bc = coded(torch, codec, esize, oname)
        decode_items_batch(torch, src, bc, codec, esize, "%s esize %d orders %s" % (trc.CODEC_NAMES[codec], esize, oname))


def raw_encode_obatch(bc, work_bytes):
    st = bc.codec in trc.STATIC
    return trc.lib().trc_encode_oplanes_batch_dev(bc.codec, bc.items, bc.filters, bc.strides, bc.orders, bc.count, bc.esize, bc.chunk,
                                                  bc.cdf.data_ptr() if st else None, bc.cdfnum, bc.status.data_ptr() if st else None, bc.clen.data_ptr(),
                                                  bc.payload.data_ptr(), bc.total.data_ptr(), bc.work.data_ptr(), work_bytes, bc._stream())


def raw_decode_obatch(bc, items, fi, ic, d_work, work_bytes):
    return trc.lib().trc_decode_oplanes_batch_dev(bc.codec, bc.clen.data_ptr(), bc.payload.data_ptr(), items, bc.filters, bc.strides, bc.orders, bc.count, fi, ic,
                                                  bc.esize, bc.chunk, bc.cdf.data_ptr() if bc.codec in trc.STATIC else None, bc.cdfnum, d_work.data_ptr(),
                                                  work_bytes, bc._stream())


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_workspace_one_byte_short(torch_cuda, codec, monkeypatch):
    torch = torch_cuda
    src, filters, strides, orders, bc = coded(torch, codec, 2, "cycle")
    monkeypatch.setattr(GP, "raw_encode_batch", raw_encode_obatch)
    monkeypatch.setattr(GP, "raw_decode_batch", raw_decode_obatch)
    workspace_one_byte_short(torch, src, bc, trc.CODEC_NAMES[codec] + " orders cycle")


# ---- the documented minimum buffers, no slack: the audited arena -------------------------------------------------------------------
_Batch = P.Batch                                               # (the fixture below puts OBatch in its place)


class OBatch(_Batch):
    """gpu_planes_arena.Batch for the family "obatch": the strided batch's items, filters and strides with an order per item"""

    def __init__(self, fam, esize, coded_for=None):
        assert fam == "obatch"
        _Batch.__init__(self, "sbatch", esize, coded_for)
        self.fam = fam
        self.orders = [1 + (i + i // 3) % 3 for i in range(self.count)]
        assert {(f, o) for f, o in zip(self.filters, self.orders)} >= {(1, 1), (1, 2), (1, 3)}
        self.virtual = OBL.virtual_filtered(self.datas, self.filters, self.strides, self.orders, esize, self.chunk)
        assert self.virtual.size == self.plan["n_virtual"]

    def fam_args(self, A, only=None, onto=None):
        return (trc.planes_filters(self.filters, self.count), trc.planes_strides(self.strides, self.count), trc.planes_orders(self.orders, self.count))


def obatch_fn(fam, what):
    assert fam == "obatch"
    return getattr(trc.lib(), "trc_" + (what % "obatch" if what.startswith("planes_") else what % "oplanes_batch"))


@pytest.fixture
def obatch_arena(monkeypatch):
    monkeypatch.setattr(P, "Batch", OBatch)
    monkeypatch.setattr(P, "_bfn", obatch_fn)


def both(run, tag, *args):
    a = run(*args, "random", 7)
    b = run(*args, "ff", 0)
    GA.same_outputs(a, b, tag)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_arena_split_join(torch_cuda, esize, obatch_arena):
    both(P.run_batch_kernels, "obatch esize %d" % esize, torch_cuda, "obatch", esize)


@pytest.mark.parametrize("codec", P.BATCH_CODERS, ids=lambda c: trc.CODEC_NAMES[c])
def test_arena_coded(torch_cuda, codec, obatch_arena):
    both(P.run_batch_coded, "obatch %s" % trc.CODEC_NAMES[codec], torch_cuda, "obatch", codec)


def run_arena_hist(torch, esize, poison, seed):
    """trc_planes_hist_obatch_dev, all four orders, for every range of ranges(count): histograms and table of exactly their bytes, NULL
    pointers outside the range"""
    b = OBatch("obatch", esize)
    count, L = b.count, trc.lib()
    specs = b.item_specs()
    for j, (fi, ic) in enumerate(P.ranges(count)):
        specs += [("r%d.hist" % j, L.trc_planes_hist_obatch_bytes(ic, esize)), ("r%d.table" % j, L.trc_planes_batch_table_bytes(ic, b.first[fi + ic] - b.first[fi]))]
    A = P.arena(torch, specs, poison, seed)
    b.put(A)
    got = dict(out=[])
    strides = trc.planes_strides(b.strides, count)
    for j, (fi, ic) in enumerate(P.ranges(count)):
        tag = "hist obatch esize %d items (%d, %d), poison %s" % (esize, fi, ic, poison)
        hb, tb = A.layout["r%d.hist" % j].size, A.layout["r%d.table" % j].size
        assert hb == ic * 4 * esize * 256 * 8 and tb
        items = b.items(A, only=range(fi, fi + ic))
        P.ok(A.call(lambda: L.trc_planes_hist_obatch_dev(15, items, strides, count, fi, ic, esize, b.chunk, A.ptr("r%d.hist" % j), A.ptr("r%d.table" % j), tb, None), tag,
                    [("r%d.hist" % j, 0, hb), ("r%d.table" % j, 0, tb)]), tag)
        h = A.get("r%d.hist" % j, hb).view("<u8").reshape(ic, 4 * esize * 256).copy()
        for i in range(fi, fi + ic):
            exp = OL.hist4(b.datas[i], esize, b.chunk, b.strides[i])
            assert np.array_equal(h[i - fi], exp), "%s: item %d: %s" % (tag, i, PM.first_difference("counters", h[i - fi], exp))
        got["out"].append(h)
    return got


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_arena_hist(torch_cuda, esize):
    both(run_arena_hist, "hist obatch esize %d" % esize, torch_cuda, esize)


# ---- the histograms and the advisor ----------------------------------------------------------------------------------------
_hists = {}


def hist_model(esize, chunk):
    """-> (items, their strides, uint64 [count, 4 * esize * 256] of oplanes_lib.hist4): computed once per key, shared, left unchanged"""
    key = (esize, chunk)
    if key not in _hists:
        strides = OBL.stride_assignments(len(SIZES))["cycle"]
        datas = OBL.gen_items(esize, SIZES, 300 * esize + chunk, lambda i: strides[i])
        h = np.stack([OL.hist4(d, esize, chunk, s) for d, s in zip(datas, strides)])
        h.setflags(write=False)
        _hists[key] = (datas, strides, h)
    return _hists[key]


def device_ohists(torch, src, esize, chunk, orders_set, strides, fi=0, ic=None, null_outside=False):
    """one trc_planes_hist_obatch_dev call into a buffer guarded on both sides, with a guarded table of exactly the range's size
    -> uint64 [items, 4 * esize * 256]"""
    count = len(src.sizes)
    ic = count - fi if ic is None else ic
    _, first = BL.plan(src.sizes, esize, chunk)
    tb = trc.lib().trc_planes_batch_table_bytes(ic, first[fi + ic] - first[fi])
    hb = trc.planes_hist_obatch_bytes(ic, esize)
    assert hb == ic * trc.planes_hist_order_bytes(esize) and tb > 0
    d_hist, d_table = Guarded(torch, hb), guarded(torch, tb)
    trc.planes_hist_obatch(orders_set, src.items(range(fi, fi + ic)) if null_outside else src.items(), strides, count, fi, ic, esize, chunk, d_hist.t, d_table, tb)
    torch.cuda.synchronize()
    got, intact = d_hist.get()
    assert intact, "the call wrote outside the histograms of its range"
    assert (d_table.cpu().numpy()[tb:] == 0xA5).all() and src.unchanged()
    return got.view("<u8").reshape(ic, 4 * esize * 256).copy()


def hist_case(torch, esize, chunk):
    datas, strides, h = hist_model(esize, chunk)
    src = Packed(torch, datas, seed=chunk + esize)
    got = device_ohists(torch, src, esize, chunk, 15, strides)
    for i in range(len(datas)):
        assert np.array_equal(got[i], h[i]), "esize %d chunk %d item %d (%d elements, stride %d): %s" % (
            esize, chunk, i, SIZES[i], strides[i], PM.first_difference("counters", got[i], h[i]))
    return src, datas, strides, h, got


@pytest.mark.parametrize("chunk", (256, 4096))
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_histograms(torch_cuda, esize, chunk, monkeypatch):
    torch = torch_cuda
    src, datas, strides, h, got = hist_case(torch, esize, chunk)
    hb = trc.planes_hist_order_bytes(esize)
    for i in (0, 5, 9, len(datas) - 3, len(datas) - 1):         # the contract as it is written: the unbatched call on a padded copy
        d = datas[i]
        d_in = guarded(torch, d.size + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
        d_one = guarded(torch, hb)
        trc.planes_hist_order(15, strides[i], d_in, d.size, esize, chunk, d_one)
        torch.cuda.synchronize()
        assert np.array_equal(d_one.cpu().numpy()[:hb].view("<u8"), got[i]), "item %d" % i
    # a partial item range with NULL pointers outside it; rows that were not requested stay zero
    part = device_ohists(torch, src, esize, chunk, 15, strides, fi=7, ic=9, null_outside=True)
    assert np.array_equal(part, h[7:16])
    for orders_set in (6, 9):
        some = device_ohists(torch, src, esize, chunk, orders_set, strides, fi=20, ic=6).reshape(6, 4, esize * 256)
        want = h[20:26].reshape(6, 4, esize * 256)
        for k in range(4):
            assert np.array_equal(some[:, k], want[:, k] if orders_set >> k & 1 else np.zeros_like(want[:, k])), (orders_set, k)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "1")       # a flush at every turn
    hist_case(torch, esize, chunk)


def test_advise_obatch_dev(torch_cuda, monkeypatch):
    torch = torch_cuda
    esize, chunk = 4, 256
    datas = [d[:4 * m] for (_, _, d), m in zip(OBL.table_batch(1 << 12), (4096, 3000, 1025, 4096, 4096))] + OBL.gen_items(esize, [300, 2049, 5], 3)
    count = len(datas)
    strides = [1, 1, 1, 1, 4, 3, 8, 2]
    src = Packed(torch, datas, seed=2)
    h = device_ohists(torch, src, esize, chunk, 15, strides)
    by_hand = trc.planes_advise_obatch(h, 15, esize, src.items(), count)
    assert [k if f else 0 for f, k in zip(*by_hand[:2])] == [OL.advise(OL.hist4(d, esize, chunk, s), 15, esize, d.size // esize) for d, s in zip(datas, strides)]
    monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", "3")     # three slabs
    got = trc.planes_advise_obatch_dev(src.items(), esize, chunk, 15, count, "cuda:0", strides=strides)
    assert got[:2] == by_hand[:2] and all(np.array_equal(a[k], b[k]) for a, b in zip(got[2], by_hand[2]) for k in a)
    assert got[0][:4] == [1, 1, 1, 0] and got[1][0] >= 2 and got[1][1:4] == [1, 1, 1]
    assert src.unchanged()
    tensors = src.views()
    assert trc.planes_advise_obatch_dev(tensors, esize, chunk, strides=strides, advice=False)[:2] == by_hand[:2]


# ---- the TRCU container ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S, trc.RCSS))
def test_container(torch_cuda, codec, esize):
    torch = torch_cuda
    L = trc.lib()
    src, filters, strides, orders, bc = coded(torch, codec, esize, "cycle")
    count = bc.count
    d_cont, size = bc.pack(guard=GUARD)
    torch.cuda.synchronize()
    tag = "%s esize %d" % (trc.CODEC_NAMES[codec], esize)
    assert bc.guards_ok(), tag + ": pack wrote behind one of the coded buffers"
    cont = d_cont.cpu().numpy().copy()
    cdfnum = 256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0
    bound = trc.planes_obatch_bound(codec, src.sizes, esize, CHUNK, cdfnum)
    assert 0 < size == cont.size <= bound - trc.PAD
    assert bc.pack_guard.numel() == bound + GUARD - size and (bc.pack_guard == 0xA5).all().item(), tag + ": a byte at or behind d_out + size was written"
    # what the definition says: the prefix, the TRCB front, the parent's TRCP container of the materialised VO
    prefix = trc.planes_obatch_prefix(count)
    st, od = OBL.stored(filters, strides, orders)
    vo = OBL.virtual_filtered(src.datas, filters, strides, orders, esize, CHUNK)
    want = np.concatenate([OBL.prefix(filters, strides, orders),
                           CL.expected(src.datas, filters, esize, CHUNK, trc.host_encode_planes(codec, vo, esize, CHUNK, cdfnum=256, prm=PRM))])
    assert want[:16].tobytes() == struct.pack("<IBBHQ", trc.OBATCH_MAGIC, 1, 0, 0, count)
    assert np.array_equal(cont, want), tag + ": the packed container is not the definition's"
    # ... and what the host encoder writes, for items on the device and on the host
    for arrays in (src.views(), src.datas):
        got = trc.host_encode_planes_batch(codec, arrays, esize, CHUNK, filters=filters, cdfnum=256, prm=PRM, strides=strides, orders=orders)
        assert np.array_equal(got, cont), tag + ": trc_encode_oplanes_batch_host"
    trc.planes_obatch_check(cont, count)
    h, n, f, s, o = trc.planes_obatch_info(cont)
    assert n == src.sizes and f == filters and s == st and o == od and h["size"] == size - prefix
    trc.planes_batch_check(cont[prefix:], count)
    assert L.trc_planes_check(cont[prefix + h["inner"]:].ctypes.data, cont.size - prefix - h["inner"], bc.plan["n_virtual"]) == 0
    # any item range back: from the container where it lies, and through host pointers
    total = trc.parse_planes_batch(cont[prefix:])["total"]
    for fi, ic in item_ranges(count, [(2, 5)]):
        only = range(fi, fi + ic)
        dst = Packed(torch, src.datas, seed=esize, data=False)
        bc.range_work, bc.range_work_bytes = None, 0
        bc.decode_packed(bc.packed, total, fi, ic, out=dst.views(only), cont_bytes=size)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag + " decode_packed items (%d, %d)" % (fi, ic)
        assert bc.guards_ok()
        back = trc.host_decode_planes_batch(cont, fi, ic)
        assert all(np.array_equal(b, src.datas[i]) for b, i in zip(back, only)), tag + " host decode items (%d, %d)" % (fi, ic)
    dst = Packed(torch, src.datas, seed=esize, data=False)
    assert trc.host_decode_planes_batch(cont, 3, 2, out=dst.views(range(3, 5))) == src.sizes[3] + src.sizes[4]
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(3, 5)))
    assert np.array_equal(bc.packed[:size].cpu().numpy(), want) and np.array_equal(src.buf.cpu().numpy(), src.img)
    with pytest.raises(trc.TrcError, match="rc=-1"):           # one byte of the container missing
        bc.decode_packed(bc.packed, total, 0, 1, out=dst.views(range(1)), cont_bytes=size - 1)


def test_container_routing(torch_cuda):
    """orders that change nothing give the TRCT container of the strided batch or the TRCB container of the filtered batch, from
    pack() and from the host encoder"""
    torch = torch_cuda
    esize = 4
    datas = OBL.gen_items(esize, W_SIZES, 5)
    src = Packed(torch, datas)
    filters = [1, 0, 2, 0, 1, 0, 2, 0]
    for strides, magic, strided in (([2, 1, 3, 1, 1, 1, 1, 1], trc.SBATCH_MAGIC, True), (None, CL.MAGIC, False), ([1, 7, 1, 8, 1, 2, 1, 3], CL.MAGIC, False)):
        want = trc.host_encode_planes_batch(trc.RCA, datas, esize, CHUNK, filters=filters, strides=strides)
        assert int(want[:4].view("<u4")[0]) == magic
        for orders in (None, 1, [1, 3, 2, 3, 1, 2, 3, 2]):
            bc = trc.PlanesBatchCoder(trc.RCA, src.views(), CHUNK, guard=GUARD, esize=esize, filters=filters, strides=strides, orders=orders)
            assert not bc.ordered() and bc.strided() == strided
            bc.encode()
            d_cont, size = bc.pack(guard=GUARD)
            assert np.array_equal(d_cont.cpu().numpy(), want) and (bc.pack_guard == 0xA5).all().item()
            assert np.array_equal(trc.host_encode_planes_batch(trc.RCA, datas, esize, CHUNK, filters=filters, strides=strides, orders=orders), want)


def test_auto_orders_is_the_explicit_call(torch_cuda):
    """trc_encode_aoplanes_batch_host writes byte for byte what the explicit call writes for the advisor's choice: TRCU where an order
    above 1 is chosen, TRCT where only a stride is left, TRCB otherwise"""
    torch = torch_cuda
    esize, chunk = 4, 256
    table = [d[:4 * m] for (_, _, d), m in zip(OBL.table_batch(1 << 12), (4096, 3000, 1025, 4096, 4096))]
    rows = np.frombuffer(SL.table_rows(1024).tobytes(), dtype=np.uint8).copy()       # rows of 4 int32 fields: the delta at stride 4, order 1
    cases = ((table, [1, 1, 1, 1, 4], trc.OBATCH_MAGIC), ([table[1], rows, table[3]], [1, 4, 1], trc.SBATCH_MAGIC), ([table[1], table[2], table[3]], None, CL.MAGIC),
             ([table[3], table[3][:400]], [2, 2], CL.MAGIC))
    for datas, strides, magic in cases:
        for arrays in (datas, Packed(torch, datas).views()):
            cont, f, o = trc.host_encode_planes_batch(trc.RCA, arrays, esize, chunk, strides=strides, orders="auto")
            assert int(cont[:4].view("<u4")[0]) == magic, (f, o)
            want = [OL.advise(OL.hist4(d, esize, chunk, 1 if strides is None else s), 15, esize, d.size // esize)
                    for d, s in zip(datas, strides or [1] * len(datas))]
            assert [k if ff else 0 for ff, k in zip(f, o)] == want
            explicit = trc.host_encode_planes_batch(trc.RCA, datas, esize, chunk, filters=f, strides=strides, orders=o)
            assert np.array_equal(cont, explicit)
            back = trc.host_decode_planes_batch(cont)
            assert all(np.array_equal(b, d) for b, d in zip(back, datas))


# ---- the torch helper --------------------------------------------------------------------------------------------------
def test_planes_batch_coder_with_orders(torch_cuda):
    torch = torch_cuda
    named = OBL.table_batch(1 << 14)
    arrays = [np.frombuffer(d.tobytes(), dtype="<f4" if "fp32" in name else "<i4").copy() for name, _, d in named]
    strides = [s for _, s, _ in named]
    tensors = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    keep = [t.clone() for t in tensors]
    bc = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=4096, guard=GUARD, filters=[1, 1, 1, 0, 1], strides=strides, orders=[3, 1, 1, 1, 3])
    assert bc.esize == 4 and bc.count == 5 and bc.ordered() and bc.strided()
    bc.encode()
    auto = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=4096, guard=GUARD, strides=strides, orders="auto")
    auto.encode()
    assert list(auto.filters[:5]) == [1, 1, 1, 0, 1] and list(auto.orders[1:4]) == [1, 1, 1] and min(auto.orders[0], auto.orders[4]) >= 2
    assert auto.ordered() and len(auto.advice) == 5 and [a["order"] for a in auto.advice] == [o if f else 0 for f, o in zip(auto.filters[:5], auto.orders[:5])]
    ref = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=4096, guard=GUARD, filters=[1, 1, 1, 0, 1], strides=strides)
    ref.encode()
    assert 0 < bc.stored_bytes() < 0.9 * ref.stored_bytes(), "smooth series are meant to code shorter behind order 3 than behind the zigzag delta"
    assert auto.stored_bytes() <= bc.stored_bytes()
    for coder in (bc, auto):
        for t in tensors:
            t.zero_()
        coder.decode(4, 1)                                      # the woven series alone into the encoded tensors
        torch.cuda.synchronize()
        for i, (t, k) in enumerate(zip(tensors, keep)):
            assert torch.equal(t.view(torch.uint8), (k if i == 4 else torch.zeros_like(k)).view(torch.uint8)), i
        out = [torch.empty_like(k) for k in keep]
        coder.decode(out=out)
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.uint8), k.view(torch.uint8)) for o, k in zip(out, keep)) and coder.guards_ok()
        for t, k in zip(tensors, keep):
            t.copy_(k)
    d_cont, size = auto.pack()
    assert trc.is_planes_obatch(d_cont.cpu().numpy())
    with pytest.raises(ValueError):
        trc.PlanesBatchCoder(trc.RCA, tensors, filters=1, orders="auto")
    with pytest.raises(ValueError):
        trc.PlanesBatchCoder(trc.RCA, tensors, filters=1, orders=2, bases=[None] * 5)


# ---- the harness -------------------------------------------------------------------------------------------------------------
def test_trcfile_round_trip(torch_cuda, tmp_path):
    named = OBL.table_batch(1 << 12)
    paths = []
    for i, (_, _, d) in enumerate(named[:4]):
        paths.append(str(tmp_path / ("item%d.bin" % i)))
        d.tofile(paths[-1])
    comp = str(tmp_path / "batch.trcu")
    r = trcfile("b", 46, 4, 256, "o", comp, *paths)             # id 46: the adaptive range coder (trc.RCA)
    want = [OL.advise(OL.hist4(d, 4, 256, 1), 15, 4, d.size // 4) for _, _, d in named[:4]]
    assert max(want) > 1 and want[3] == 0
    assert [int(line.split("choice order ")[1].split()[0]) for line in r.stdout.splitlines() if "choice order" in line] == want
    cont = np.fromfile(comp, dtype=np.uint8)
    assert trc.is_planes_obatch(cont)
    trc.planes_obatch_check(cont, 4)
    lines = trcfile("l", comp).stdout.splitlines()
    assert lines[1:] == ["item %d: %d bytes, filter %s, stride 1, order %d" % (i, named[i][2].size, "nz"[k > 0], max(k, 1)) for i, k in enumerate(want)]
    for first, cnt in ((0, 1), (1, 2), (0, 4)):
        back = str(tmp_path / "back.bin")
        trcfile("B", comp, first, cnt, back)
        assert np.array_equal(np.fromfile(back, dtype=np.uint8), np.concatenate([named[i][2] for i in range(first, first + cnt)]))
    # a batch in which the advisor chooses no order above 1 is a TRCB file
    trcfile("b", 46, 4, 256, "o", comp, paths[1], paths[3])
    assert np.fromfile(comp, dtype=np.uint8)[:4].tobytes() == b"TRCB"
    assert trcfile("l", comp).stdout.splitlines()[1:] == ["item 0: %d bytes, filter z" % named[1][2].size, "item 1: %d bytes, filter n" % named[3][2].size]
