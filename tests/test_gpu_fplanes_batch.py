"""Batched byte planes with a filter per item on the MI355X: the filtered gathering split and the scanning, scattering join at the
edges of a thread's vector, a tile, a chunk, a span, an item and the grid-stride loop, under uniform and mixed filter assignments;
the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on VF, byte for byte); decode of item ranges.
As in test_gpu_planes_batch.py the items of a batch lie in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of
their own, every other device buffer is followed by a 512-byte guard of 0xA5, and every comparison is byte equality against the
numpy model (fplanes_batch_lib) or against the unbatched calls.  The device calls and comparisons shared with the other plane files
are in gpu_planes.py."""
import numpy as np
import pytest

import fplanes_batch_lib as FBL
import fplanes_lib as FL
import planes_batch_lib as BL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (CHUNK, GUARD, PRM, Packed, assert_same_outputs, coded_batch, decode_items_batch, decodes_whole_batch, encode_contract_batch,
                        guarded, padded, split_join_batch, workspace_one_byte_short)

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
SHUFFLED = [SIZES[i] for i in np.random.default_rng(5).permutation(len(SIZES))]
CHUNKS = (256, 320, 512, 4096)          # 8-chunk spans / not a power of two, a span of 5 tiles / exactly one tile / 8 tiles: the carry
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
LOOP_GRID = 3


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, order, name, partial=True):
    datas = FBL.gen_items(esize, order, 1000 * esize + chunk)
    filters = FBL.assignments(len(datas), chunk + esize)[name]
    split_join_batch(torch, datas, esize, chunk, FBL.virtual_filtered(datas, filters, esize, chunk),
                     "esize %d, chunk %d, filters %s" % (esize, chunk, name), filters=filters, partial=partial)


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


def coded(torch, codec, esize, name):
    """-> (Packed source, filters, PlanesBatchCoder holding its coded batch): computed once per key, shared, left unchanged"""
    datas = FBL.gen_items(esize, W_SIZES, 50 + esize)
    filters = FBL.assignments(len(datas), 9 + esize)[name]
    src, bc = coded_batch(torch, codec, esize, datas, filters=filters)
    return src, filters, bc


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    for name in NAMES:
        src, filters, bc = coded(torch, codec, esize, name)
        encode_contract_batch(torch, src, bc, codec, esize, FBL.virtual_filtered(src.datas, filters, esize, CHUNK),
                              "%s esize %d filters %s" % (trc.CODEC_NAMES[codec], esize, name))


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
    pc.encode(padded(torch, d), d.size)
    assert pc.guards_ok()
    assert_same_outputs(torch, bc, pc, codec, esize, "%s filter %d one item" % (trc.CODEC_NAMES[codec], filt))
    decodes_whole_batch(torch, src, bc, "%s filter %d one item" % (trc.CODEC_NAMES[codec], filt))


def raw_encode(bc, filters):
    st = bc.codec in trc.STATIC
    return trc.lib().trc_encode_fplanes_batch_dev(bc.codec, bc.items, filters, bc.count, bc.esize, bc.chunk, bc.cdf.data_ptr() if st else None,
                                                  bc.cdfnum, bc.status.data_ptr() if st else None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                                  bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes, bc._stream())


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
    for name in ("cycle", "random", "delta"):
        src, filters, bc = coded(torch, codec, esize, name)
        decode_items_batch(torch, src, bc, codec, esize, "%s esize %d filters %s" % (trc.CODEC_NAMES[codec], esize, name))


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_workspace_one_byte_short(torch_cuda, codec):
    torch = torch_cuda
    esize = 2
    src, filters, bc = coded(torch, codec, esize, "cycle")
    workspace_one_byte_short(torch, src, bc, trc.CODEC_NAMES[codec] + " filters cycle")


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
