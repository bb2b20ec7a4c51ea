"""Batched byte planes with a filter and a stride per item on the MI355X: the strided gathering split and the scanning, scattering
join at the edges of a thread's vector, a tile, a chunk, a span, an item and the grid-stride loop, under uniform and mixed stride and
filter assignments -- items shorter than their stride, partial last vectors whose predecessors lie in the vector in front,
neighbours of different strides in one wave and in one tile, strides that do not divide the chunk; the routing of stride 1 to the
filtered batch; the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on VS, byte for byte); decode of
item ranges; the histograms per item under the items' strides and the advisor on them; the TRCT container; the torch helper.
As in test_gpu_planes_batch.py the items of a batch lie in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of
their own, every other device buffer is followed by a 512-byte guard of 0xA5, and every comparison is byte equality against the
numpy model (splanes_batch_lib) or against the unbatched calls.  The device calls and comparisons shared with the other plane files
are in gpu_planes.py."""
import struct

import numpy as np
import pytest

import fplanes_batch_lib as FBL
import planes_batch_lib as BL
import planes_container_lib as CL
import planes_lib as PL
import splanes_batch_lib as SBL
import splanes_lib as SL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (CHUNK, GUARD, PRM, Packed, assert_hists, assert_same_outputs, coded_batch, decode_items_batch, decodes_whole_batch,
                        device_hists, encode_contract_batch, guarded, item_ranges, padded, split_join_batch, workspace_one_byte_short)

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
SHUFFLED = [SIZES[i] for i in np.random.default_rng(5).permutation(len(SIZES))]
CHUNKS = (256, 320, 512, 4096)          # 8-chunk spans, strides mixed in a tile / 3, 6, 7 do not divide it / exactly one tile / 8 tiles: the carry
STRIDE_NAMES = ("3", "8", "cycle", "random")
FILTER_NAMES = ("delta", "xor", "cycle")
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
LOOP_GRID = 3


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, order, sname, fname, partial=True):
    datas = FBL.gen_items(esize, order, 1000 * esize + chunk)
    strides = SBL.stride_assignments(len(datas), chunk + esize)[sname]
    filters = SBL.filter_assignments(len(datas))[fname]
    split_join_batch(torch, datas, esize, chunk, SBL.virtual_filtered(datas, filters, strides, esize, chunk),
                     "esize %d, chunk %d, strides %s, filters %s" % (esize, chunk, sname, fname), filters=filters, strides=strides, partial=partial)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join(torch_cuda, esize, chunk):
    for order in (SIZES, SHUFFLED):
        for sname in STRIDE_NAMES:
            for fname in FILTER_NAMES:
                split_join_case(torch_cuda, esize, chunk, order, sname, fname)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, chunk, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", str(LOOP_GRID))       # 3 workgroups: 12 waves over the spans, 768 threads over 10 000 vectors
    for sname in STRIDE_NAMES:
        for fname in FILTER_NAMES:
            split_join_case(torch_cuda, esize, chunk, SIZES, sname, fname)


def test_stride_one_is_the_filtered_batch(torch_cuda):
    """strides None, 1 and [1] * count, and any stride on items without a filter, give the planes of trc_planes_split_fbatch_dev"""
    torch = torch_cuda
    esize, chunk = 4, 320
    datas = FBL.gen_items(esize, SIZES, 77)
    src = Packed(torch, datas)
    count = len(datas)
    pl, _ = BL.plan(src.sizes, esize, chunk)
    pitch = BL.up256(pl["m_total"])
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    filters = SBL.filter_assignments(count)["cycle"]
    want, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    trc.planes_split_fbatch(src.items(), filters, count, esize, chunk, want, pitch, d_table, tb)
    none_only = [5 if f == SL.NONE else 1 for f in filters]     # a stride above 1 where there is no filter: no effect
    for strides in (None, 1, [1] * count, none_only):
        got = guarded(torch, esize * pitch)
        trc.planes_split_sbatch(src.items(), filters, strides, count, esize, chunk, got, pitch, d_table, tb)
        assert torch.equal(got, want), strides
        dst = Packed(torch, datas, data=False)
        trc.planes_join_sbatch(got, 0, pitch, dst.items(), filters, strides, count, 0, count, esize, chunk, d_table, tb)
        assert np.array_equal(dst.buf.cpu().numpy(), src.img), strides
    plain = guarded(torch, esize * pitch)
    trc.planes_split_batch(src.items(), count, esize, chunk, plain, pitch, d_table, tb)
    got = guarded(torch, esize * pitch)
    trc.planes_split_sbatch(src.items(), 0, 7, count, esize, chunk, got, pitch, d_table, tb)
    assert torch.equal(got, plain)


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads


def coded(torch, codec, esize, sname):
    """-> (Packed source, filters, strides, PlanesBatchCoder holding its coded batch): computed once per key, shared, left unchanged"""
    datas = FBL.gen_items(esize, W_SIZES, 50 + esize)
    strides = SBL.stride_assignments(len(datas), 9 + esize)[sname]
    filters = SBL.filter_assignments(len(datas))["cycle" if sname == "cycle" else "delta" if sname == "3" else "xor"]
    if sname == "cycle":
        filters = filters[1:] + filters[:1]                     # (1, 2, 0, ..): strides 1, 2, 4, 5, 7, 8 meet a filter
    src, bc = coded_batch(torch, codec, esize, datas, filters=filters, strides=strides)
    assert bc.strided()
    return src, filters, strides, bc


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    for sname in STRIDE_NAMES:
        src, filters, strides, bc = coded(torch, codec, esize, sname)
        encode_contract_batch(torch, src, bc, codec, esize, SBL.virtual_filtered(src.datas, filters, strides, esize, CHUNK),
                              "%s esize %d strides %s" % (trc.CODEC_NAMES[codec], esize, sname))


@pytest.mark.parametrize("stride", (2, 3, 8))
@pytest.mark.parametrize("codec", CODECS)
def test_one_item_is_the_strided_plain_call(torch_cuda, codec, stride):
    torch = torch_cuda
    esize, m = 2, 5 * CHUNK + 77                                # m % chunk != 0
    filt = SL.FILTERS[stride % 2]
    d = SL.gen("interleaved", esize, m, 0, 3, stride)
    src = Packed(torch, [d])
    bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filt, strides=stride)
    bc.encode()
    assert bc.guards_ok()
    pc = trc.StridedPlanesCoder(codec, d.size, esize, CHUNK, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, filter=filt, stride=stride)
    pc.encode(padded(torch, d), d.size)
    assert pc.guards_ok()
    assert_same_outputs(torch, bc, pc, codec, esize, "%s filter %d stride %d one item" % (trc.CODEC_NAMES[codec], filt, stride))
    decodes_whole_batch(torch, src, bc, "%s filter %d stride %d one item" % (trc.CODEC_NAMES[codec], filt, stride))


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_items(torch_cuda, codec, esize):
    torch = torch_cuda
    for sname in ("cycle", "random", "3"):
        src, filters, strides, bc = coded(torch, codec, esize, sname)
        decode_items_batch(torch, src, bc, codec, esize, "%s esize %d strides %s" % (trc.CODEC_NAMES[codec], esize, sname))


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_workspace_one_byte_short(torch_cuda, codec):
    torch = torch_cuda
    esize = 2
    src, filters, strides, bc = coded(torch, codec, esize, "cycle")
    workspace_one_byte_short(torch, src, bc, trc.CODEC_NAMES[codec] + " strides cycle")


# ---- the histograms and the advisor ----------------------------------------------------------------------------------------
_hists = {}


def hist_model(esize, chunk):
    """-> (items, their strides, uint64 [count, 3 * esize * 256] of splanes_lib.hist3): computed once per key, shared, left unchanged"""
    key = (esize, chunk)
    if key not in _hists:
        datas = FBL.gen_items(esize, SIZES, 300 * esize + chunk)
        strides = SBL.stride_assignments(len(datas), 0)["cycle"]
        h = np.stack([SL.hist3(d, esize, chunk, s) for d, s in zip(datas, strides)])
        h.setflags(write=False)
        _hists[key] = (datas, strides, h)
    return _hists[key]


def hist_case(torch, esize, chunk):
    datas, strides, h = hist_model(esize, chunk)
    got, _ = device_hists(torch, esize, chunk, 7, src=Packed(torch, datas, seed=chunk + esize), strides=strides)
    assert_hists(got, h, SIZES, 7, "esize %d chunk %d strides cycle" % (esize, chunk))
    return datas, strides, got


@pytest.mark.parametrize("chunk", (256, 4096))
@pytest.mark.parametrize("esize", PL.ESIZES)
def test_histograms(torch_cuda, esize, chunk, monkeypatch):
    torch = torch_cuda
    datas, strides, got = hist_case(torch, esize, chunk)
    hb = trc.planes_hist_bytes(esize)
    for i, (d, s) in enumerate(zip(datas, strides)):           # the contract as it is written: the unbatched call on a padded copy
        d_in = guarded(torch, d.size + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
        d_one = guarded(torch, hb)
        trc.planes_hist_stride(7, s, d_in, d.size, esize, chunk, d_one)
        torch.cuda.synchronize()
        assert np.array_equal(d_one.cpu().numpy()[:hb].view("<u8"), got[i].reshape(-1)), "item %d" % i
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "1")       # a flush at every turn
    hist_case(torch, esize, chunk)


def test_advise_sbatch_dev(torch_cuda, monkeypatch):
    torch = torch_cuda
    esize, chunk = 4, 256
    datas = [SL.gen("interleaved", esize, m, 0, 40 + i, 1 + i % 8) for i, m in enumerate(W_SIZES)] + FBL.gen_items(esize, [300, 2049], 3)
    count = len(datas)
    strides = [1 + i % 8 for i in range(count)]
    src = Packed(torch, datas, seed=2)
    h, _ = device_hists(torch, esize, chunk, 7, src=src, strides=strides)
    by_hand, by_hand_advice = trc.planes_advise_batch(h, 7, esize, src.items(), count)
    monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", "3")
    got, advice = trc.planes_advise_batch_dev(src.items(), esize, chunk, count=count, device="cuda:0", strides=strides)
    assert got == by_hand and all(np.array_equal(a[k], b[k]) for a, b in zip(advice, by_hand_advice) for k in a)
    assert np.array_equal(src.buf.cpu().numpy(), src.img)


# ---- the TRCT container ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S, trc.RCSS))
def test_container(torch_cuda, codec, esize):
    torch = torch_cuda
    L = trc.lib()
    src, filters, strides, bc = coded(torch, codec, esize, "cycle")
    count = bc.count
    d_cont, size = bc.pack(guard=GUARD)
    torch.cuda.synchronize()
    tag = "%s esize %d" % (trc.CODEC_NAMES[codec], esize)
    assert bc.guards_ok(), tag + ": pack wrote behind one of the coded buffers"
    cont = d_cont.cpu().numpy().copy()
    cdfnum = 256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0
    bound = trc.planes_sbatch_bound(codec, src.sizes, esize, CHUNK, cdfnum)
    assert 0 < size == cont.size <= bound - trc.PAD
    assert bc.pack_guard.numel() == bound + GUARD - size and (bc.pack_guard == 0xA5).all().item(), tag + ": a byte at or behind d_out + size was written"
    # what the definition says: the prefix, the TRCB front, the parent's TRCP container of the materialised VS
    prefix = trc.planes_sbatch_prefix(count)
    stored = [1 if f == SL.NONE else s for f, s in zip(filters, strides)]
    vs = SBL.virtual_filtered(src.datas, filters, strides, esize, CHUNK)
    want = np.concatenate([np.frombuffer(struct.pack("<IBBHQ", trc.SBATCH_MAGIC, 1, 0, 0, count) + bytes(stored) + bytes(-count % 16), dtype=np.uint8),
                           CL.expected(src.datas, filters, esize, CHUNK, trc.host_encode_planes(codec, vs, esize, CHUNK, cdfnum=256, prm=PRM))])
    assert np.array_equal(cont, want), tag + ": the packed container is not the definition's"
    # ... and what the host encoder writes, for items on the device and on the host
    for arrays in (src.views(), src.datas):
        got = trc.host_encode_planes_batch(codec, arrays, esize, CHUNK, filters=filters, cdfnum=256, prm=PRM, strides=strides)
        assert np.array_equal(got, cont), tag + ": trc_encode_splanes_batch_host"
    trc.planes_sbatch_check(cont, count)
    h, n, f, s = trc.planes_sbatch_info(cont)
    assert n == src.sizes and f == filters and s == stored and h["size"] == size - prefix
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
    """strides that change nothing give the TRCB container of the filtered batch, from pack() and from the host encoder"""
    torch = torch_cuda
    esize = 4
    datas = FBL.gen_items(esize, W_SIZES, 5)
    src = Packed(torch, datas)
    filters = [1, 0, 2, 0, 1, 0, 2, 0]
    want = trc.host_encode_planes_batch(trc.RCA, datas, esize, CHUNK, filters=filters)
    for strides in (None, 1, [1, 7, 1, 8, 1, 2, 1, 3]):
        bc = trc.PlanesBatchCoder(trc.RCA, src.views(), CHUNK, guard=GUARD, esize=esize, filters=filters, strides=strides)
        assert not bc.strided()
        bc.encode()
        d_cont, size = bc.pack(guard=GUARD)
        assert np.array_equal(d_cont.cpu().numpy(), want) and (bc.pack_guard == 0xA5).all().item()
        assert np.array_equal(trc.host_encode_planes_batch(trc.RCA, datas, esize, CHUNK, filters=filters, strides=strides), want)


# ---- the torch helper --------------------------------------------------------------------------------------------------
def test_planes_batch_coder_with_strides(torch_cuda):
    torch = torch_cuda
    arrays, filters, strides = SBL.table_batch()
    tensors = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    assert tensors[0].shape == (4096, 4) and tensors[0].dtype == torch.int32
    keep = [t.clone() for t in tensors]
    bc = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=512, guard=GUARD, filters=filters, strides=strides)
    assert bc.esize == 4 and bc.count == 3 and bc.strided()
    bc.encode()
    for other in (dict(filters=filters), dict(filters=[0, 1, 0])):
        ref = trc.PlanesBatchCoder(trc.RCA, tensors, chunk=512, guard=GUARD, **other)
        assert not ref.strided()
        ref.encode()
        assert 0 < bc.stored_bytes() < ref.stored_bytes(), "rows of 4 fields are meant to code shorter behind the delta at stride 4: %r" % other
    for t in tensors:
        t.zero_()
    bc.decode(0, 1)                                             # the table alone into the encoded tensors
    torch.cuda.synchronize()
    for i, (t, k) in enumerate(zip(tensors, keep)):
        assert torch.equal(t.view(torch.uint8), (k if i == 0 else torch.zeros_like(k)).view(torch.uint8)), i
    out = [torch.empty_like(k) for k in keep]
    bc.decode(out=out)
    torch.cuda.synchronize()
    assert all(torch.equal(o.view(torch.uint8), k.view(torch.uint8)) for o, k in zip(out, keep)) and bc.guards_ok()
