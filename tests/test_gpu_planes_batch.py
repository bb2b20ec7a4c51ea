"""Batched byte planes on the MI355X: the gathering split and the scattering join at the edges of a thread's vector, a chunk, an
item and the grid-stride loop; the contract of the coded calls (a batch's outputs are those of trc_encode_planes_dev on the
virtual buffer, byte for byte); decode of item ranges; and the errors.  The items of a batch lie in ONE allocation with 16 to 48
bytes of 0xA5 between them and no slack of their own (planes_batch_lib), every other device buffer is followed by a 512-byte guard
of 0xA5, and every comparison is byte equality against numpy or against the unbatched calls.  The device calls and comparisons shared
with the other plane files are in gpu_planes.py."""
import numpy as np
import pytest

import planes_batch_lib as BL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (CHUNK, GUARD, PRM, Packed, assert_same_outputs, coded_batch, decode_items_batch, decodes_whole_batch, encode_contract_batch,
                        guarded, planes_reference, split_join_batch, workspace_one_byte_short)

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 2047, 2049, 4097, 65539]      # m[i], in elements
CHUNKS = (256, 320, 4096)                                       # 320: 40 vectors per chunk, not a power of two
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
LOOP_GRID = 3


def batch_data(esize, order, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, m * esize, dtype=np.uint8) for m in order]


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, chunk, order, partial=False):
    datas = batch_data(esize, order, 1000 * esize + chunk)
    split_join_batch(torch, datas, esize, chunk, BL.virtual(datas, esize, chunk), "esize %d, chunk %d" % (esize, chunk), partial=partial)


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
    for chunk in (256, 320):
        split_join_case(torch_cuda, esize, chunk, SIZES, partial=True)


# ---- the coded calls ---------------------------------------------------------------------------------------------------
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads


def weights_items(esize, sizes=W_SIZES):
    return [PL.weights(m, esize, seed=11 + i) for i, m in enumerate(sizes)]


def coded(torch, codec, esize):
    """-> (Packed source, PlanesBatchCoder holding its coded batch): computed once per (codec, esize), shared, left unchanged"""
    return coded_batch(torch, codec, esize, weights_items(esize))


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    src, bc = coded(torch, codec, esize)
    encode_contract_batch(torch, src, bc, codec, esize, BL.virtual(src.datas, esize, CHUNK), "%s esize %d" % (trc.CODEC_NAMES[codec], esize))


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
    decodes_whole_batch(torch, src, bc, trc.CODEC_NAMES[codec] + " one item")


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_items(torch_cuda, codec, esize):
    torch = torch_cuda
    src, bc = coded(torch, codec, esize)
    decode_items_batch(torch, src, bc, codec, esize, "%s esize %d" % (trc.CODEC_NAMES[codec], esize))


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
    decodes_whole_batch(torch, src, bc, "mixed")


# ---- errors ------------------------------------------------------------------------------------------------------------
def raw_encode(bc, codec, items, count):
    st = (codec & 0xff) in trc.STATIC
    return trc.lib().trc_encode_planes_batch_dev(codec, items, count, bc.esize, bc.chunk, bc.cdf.data_ptr() if st else None, bc.cdfnum,
                                                 bc.status.data_ptr() if st else None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                                 bc.total.data_ptr(), bc.work.data_ptr(), bc.work_bytes, bc._stream())


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
    E_ARG = -1
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
    workspace_one_byte_short(torch, src, bc, trc.CODEC_NAMES[codec])
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
