"""The batch advisor on the MI355X.  trc_planes_hist_batch_dev counts, so every comparison is exact equality with the numpy model
(abatch_lib: advise_lib's histograms item by item): at the edges of a thread's vector, a chunk, an item, a workgroup's run of
chunks and the grid; with runs that start inside an item and span several; across flushes of the 32-bit counters inside an item;
with every lane on one bin; into a dirty buffer; over an item range with every other pointer NULL.  As in test_gpu_planes_batch.py
the items lie in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of their own, every other device buffer is
followed by a 512-byte guard of 0xA5 that must survive, and the input image must be unchanged after every call.
trc_planes_advise_batch_dev must return what the pieces give by hand, whatever the slab; PlanesBatchCoder(filters="auto") must
code byte for byte what the chosen list codes.  The histogram call and its comparisons are in gpu_planes.py."""
import ctypes as C

import numpy as np
import pytest

import abatch_lib as ABL
import advise_lib as AL
import fplanes_lib as FL
import planes_batch_lib as BL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import E_ARG, E_WORK, GUARD, Packed, assert_hists, assert_same_outputs, decodes_whole_batch, device_hists, guarded

pytestmark = pytest.mark.gpu
ORDERS = (ABL.LENGTHS, ABL.LENGTHS[::-1])
M_BIG = 65539


_model = {}


def model(esize, chunk, lengths, kinds=ABL.KINDS, seed=None):
    """-> (items, histograms of all three filters [count, 3, esize, 256]): computed once per key, shared, left unchanged"""
    key = (esize, chunk, tuple(lengths), tuple(kinds), seed)
    if key not in _model:
        datas = ABL.gen_items(esize, lengths, 1000 * esize + chunk if seed is None else seed, kinds)
        h = ABL.hist(datas, esize, chunk, AL.ALL)
        for a in datas + [h]:
            a.setflags(write=False)
        _model[key] = (datas, h)
    return _model[key]


def hist_case(torch, esize, chunk, lengths, filters, fi=0, ic=None, null_outside=False, kinds=ABL.KINDS, seed=None):
    datas, h = model(esize, chunk, lengths, kinds, seed)
    src = Packed(torch, datas, seed=chunk + esize)
    ic = len(datas) - fi if ic is None else ic
    got, _ = device_hists(torch, esize, chunk, filters, src=src, fi=fi, ic=ic, null_outside=null_outside)
    assert_hists(got, h[fi:fi + ic], list(lengths[fi:fi + ic]), filters,
                 "esize %d chunk %d filters %d items [%d, %d) of %d" % (esize, chunk, filters, fi, fi + ic, len(datas)))


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", (1, 2, 4, 7, 6))
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_histograms_equal_the_model(torch_cuda, esize, filters):
    for chunk in ABL.CHUNKS:
        for lengths in ORDERS:
            hist_case(torch_cuda, esize, chunk, lengths, filters)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_item_range_with_every_other_pointer_null(torch_cuda, esize):
    """only the range's slices are written (the buffer is sized for the range and guarded), only its items are read"""
    count = len(ABL.LENGTHS)
    for chunk in ABL.CHUNKS:
        for fi, ic in ((4, 5), (0, 1), (count - 2, 2), (count - 1, 1)):
            hist_case(torch_cuda, esize, chunk, ORDERS[0], 7, fi, ic, null_outside=True)
        hist_case(torch_cuda, esize, chunk, ORDERS[1], 6, 0, 3, null_outside=True)      # behind the 65 539 elements: short items


def test_item_count_zero_launches_nothing(torch_cuda):
    torch = torch_cuda
    datas, _ = model(4, 256, ORDERS[0])
    src = Packed(torch, datas)
    got, d_hist = device_hists(torch, 4, 256, 7, src=src, fi=5, ic=0)
    assert got.size == 0 and (d_hist.whole.cpu().numpy() == 0xA5).all()
    # ... whatever the buffers are
    assert trc.lib().trc_planes_hist_batch_dev(7, src.items(), len(datas), len(datas), 0, 4, 256, None, None, 0, None) == 0


@pytest.mark.parametrize("grid", (3, 1))
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_runs_start_inside_an_item_and_span_several(torch_cuda, esize, grid, monkeypatch):
    """3 workgroups: the long item is cut twice and each run goes on over short items; 1 workgroup walks the whole batch"""
    monkeypatch.setenv("TRC_PLANES_GRID", str(grid))
    for chunk in ABL.CHUNKS:
        for lengths in ORDERS:
            hist_case(torch_cuda, esize, chunk, lengths, 7)
    hist_case(torch_cuda, esize, 320, ORDERS[0], 2, 3, 8, null_outside=True)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_counters_flush_inside_an_item(torch_cuda, esize, monkeypatch):
    """two workgroups, the long item 16 turns of each: a flush every 5 turns, then at every turn"""
    monkeypatch.setenv("TRC_PLANES_GRID", "2")
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "5")
    for lengths in ORDERS:
        hist_case(torch_cuda, esize, 256, lengths, 7)
    hist_case(torch_cuda, esize, 320, ORDERS[0], 4)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "1")
    for lengths in ORDERS:
        hist_case(torch_cuda, esize, 320, lengths, 7)
    hist_case(torch_cuda, esize, 256, ORDERS[1], 2)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_every_lane_on_one_bin(torch_cuda, esize):
    """constant items: every lane of every wave adds to the same bin of every plane, under every filter; and weights, whose sign /
    exponent plane has a handful of bins"""
    torch = torch_cuda
    const = [np.tile(np.arange(v, v + esize, dtype=np.uint8), M_BIG) for v in (0x81, 0x17)]
    exp = ABL.hist(const, esize, 256, AL.ALL)
    assert exp[0, 0, 0, 0x81] == M_BIG and exp[1, 2, 0, 0] == M_BIG - 257          # (257 chunks open with the element itself)
    src = Packed(torch, const)
    for filters in (1, 7):
        got, _ = device_hists(torch, esize, 256, filters, src=src)
        assert_hists(got, ABL.masked(exp, filters), [M_BIG] * 2, filters, "equal elements, esize %d, filters %d" % (esize, filters))
    for filters in (1, 7):
        hist_case(torch, esize, 256, (M_BIG, 4097, M_BIG), filters, kinds=("weights",), seed=7)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_short_items_next_to_a_long_one(torch_cuda, esize):
    for chunk in ABL.CHUNKS:
        for lengths in ((5, 300, M_BIG), (M_BIG, 9, 1), (2, M_BIG, 257), (1, 1)):
            hist_case(torch_cuda, esize, chunk, lengths, 7)


def test_the_call_zeroes_a_dirty_buffer(torch_cuda):
    torch = torch_cuda
    esize, chunk = 4, 256
    d1, h1 = model(esize, chunk, (4097, 513, 2049))
    d2, h2 = model(esize, chunk, (9, 255, 1), seed=5)
    got, d_hist = device_hists(torch, esize, chunk, 7, src=Packed(torch, d1))
    assert_hists(got, h1, [4097, 513, 2049], 7, "first call")
    got, _ = device_hists(torch, esize, chunk, 2, src=Packed(torch, d2), d_hist=d_hist)      # fewer elements, fewer filters, the same buffer
    assert_hists(got, ABL.masked(h2, 2), [9, 255, 1], 2, "second call into the first one's counts")


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_slices_are_the_unbatched_call_per_item(torch_cuda, esize):
    """the contract as it is written: slice j = trc_planes_hist_dev on item j alone (here: a copy with TRC_PAD behind it), seg = chunk"""
    torch = torch_cuda
    chunk = 320
    datas, _ = model(esize, chunk, ORDERS[0])
    got, _ = device_hists(torch, esize, chunk, 7, src=Packed(torch, datas, seed=3))
    hb = trc.planes_hist_bytes(esize)
    for i, d in enumerate(datas):
        d_in = guarded(torch, d.size + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
        d_one = guarded(torch, hb)
        trc.planes_hist(7, d_in, d.size, esize, chunk, d_one)
        torch.cuda.synchronize()
        assert np.array_equal(d_one.cpu().numpy()[:hb].view("<u8").reshape(3, esize, 256), got[i]), "item %d" % i


def test_argument_errors_write_nothing(torch_cuda):
    torch = torch_cuda
    esize, chunk = 2, 256
    datas, _ = model(esize, chunk, (300, 1000, 7, 256))
    src = Packed(torch, datas)
    count, L = 4, trc.lib()
    _, first = BL.plan(src.sizes, esize, chunk)
    tb, hb = L.trc_planes_batch_table_bytes(count, first[-1]), trc.planes_hist_batch_bytes(count, esize)
    d_hist, d_table = guarded(torch, hb), guarded(torch, tb)

    def call(filters=7, items=None, cnt=count, fi=0, ic=count, esize=esize, chunk=chunk, hist=0, table=0, tbytes=tb):
        return L.trc_planes_hist_batch_dev(filters, src.items() if items is None else items, cnt, fi, ic, esize, chunk,
                                           d_hist.data_ptr() + hist, d_table.data_ptr() + table, tbytes, None)

    def items_with(i, ptr=None, n=None):
        pairs = [(v.data_ptr(), s) for v, s in zip(src.views(), src.sizes)]
        pairs[i] = (pairs[i][0] if ptr is None else ptr, pairs[i][1] if n is None else n)
        return trc.planes_items(pairs)
    base2 = src.views()[2].data_ptr()
    for kw in (dict(esize=3), dict(esize=0), dict(chunk=100), dict(chunk=128), dict(chunk=65600), dict(filters=0), dict(filters=8),
               dict(items=items_with(2, n=src.sizes[2] + 1)), dict(items=items_with(3, n=0)), dict(cnt=0),
               dict(fi=0, ic=count + 1), dict(fi=count, ic=1), dict(fi=count + 1, ic=0), dict(fi=3, ic=2),
               dict(items=items_with(2, ptr=base2 + 8)), dict(items=items_with(2, ptr=base2 + 8), fi=2, ic=1),
               dict(hist=4), dict(table=16)):
        assert call(**kw) == E_ARG, kw
    assert L.trc_planes_hist_batch_dev(7, src.items(), count, 0, count, esize, chunk, None, d_table.data_ptr(), tb, None) == E_ARG
    assert L.trc_planes_hist_batch_dev(7, src.items(), count, 0, count, esize, chunk, d_hist.data_ptr(), None, tb, None) == E_ARG
    assert call(tbytes=tb - 1) == E_WORK
    one = L.trc_planes_batch_table_bytes(1, first[2] - first[1])
    assert call(fi=1, ic=1, tbytes=one - 1) == E_WORK
    torch.cuda.synchronize()
    assert (d_hist.cpu().numpy() == 0xA5).all() and (d_table.cpu().numpy() == 0xA5).all(), "a rejected call wrote to the histograms or the table"
    assert np.array_equal(src.buf.cpu().numpy(), src.img)
    # a misaligned pointer outside the requested range is not looked at
    assert call(items=items_with(2, ptr=base2 + 8), fi=0, ic=2) == 0
    torch.cuda.synchronize()
    assert (d_hist.cpu().numpy()[2 * trc.planes_hist_bytes(esize):] == 0xA5).all()


# ---- the choice --------------------------------------------------------------------------------------------------------------
A_KINDS = ("weights", "monotone", "bitflip", "random")
A_MS = (2049, 5220, 51300)
A_CHOICE = (FL.NONE, FL.ZDELTA, FL.XOR, FL.NONE)
_advice = {}


def advice_batch(esize, chunk):
    """24 items: the four kinds at every m, twice over -> (items, elements per item, the model's advice per item); computed once"""
    key = (esize, chunk)
    if key not in _advice:
        one = [(AL.gen(kind, esize, m, 0, 31 * esize + 7), m) for m in A_MS for kind in A_KINDS]
        datas, ms = [d for d, _ in one] * 2, [m for _, m in one] * 2
        want = ABL.advise(ABL.hist(datas[:12], esize, chunk, AL.ALL), AL.ALL, esize, ms[:12]) * 2
        _advice[key] = (datas, ms, want)
    return _advice[key]


def same_advice(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


@pytest.mark.parametrize("chunk", ABL.CHUNKS)
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_advise_batch_dev(torch_cuda, esize, chunk, monkeypatch):
    torch = torch_cuda
    monkeypatch.delenv("TRC_PLANES_ADVISE_SLAB_ITEMS", raising=False)
    datas, ms, want = advice_batch(esize, chunk)
    count = len(datas)
    assert [w[0] for w in want] == list(A_CHOICE) * 6, "the model itself"
    src = Packed(torch, datas, seed=esize)
    tag = "esize %d chunk %d" % (esize, chunk)
    got, advice = trc.planes_advise_batch_dev(src.views(), esize, chunk)
    ABL.assert_advice(got, advice, want, AL.ALL, esize, ms, tag)
    # the three pieces by hand on the whole batch
    h, _ = device_hists(torch, esize, chunk, AL.ALL, src=src)
    by_hand, by_hand_advice = trc.planes_advise_batch(h, AL.ALL, esize, src.items(), count)
    assert got == by_hand and same_advice(advice, by_hand_advice), tag + ": not what the pieces give"
    # five slabs of 5, 5, 5, 5 and 4 items; and through the item array
    monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", "5")
    small, small_advice = trc.planes_advise_batch_dev(src.items(), esize, chunk, count=count, device="cuda:0")
    assert small == got and same_advice(small_advice, advice), tag + ": the slabs changed the result"
    assert trc.planes_advise_batch_dev(src.views(), esize, chunk, advice=False) == (got, None)
    assert np.array_equal(src.buf.cpu().numpy(), src.img)


def test_advise_batch_dev_workspace(torch_cuda, monkeypatch):
    """the workspace is guarded and exactly as large as asked for; one byte less is TRC_E_WORK and writes nothing"""
    torch = torch_cuda
    esize, chunk = 4, 256
    monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", "7")
    datas, ms, want = advice_batch(esize, chunk)
    src = Packed(torch, datas, seed=esize)
    L, count = trc.lib(), len(datas)
    need = L.trc_planes_advise_batch_work_bytes(src.items(), count, esize, chunk)
    assert need > 8 << 20
    d_work = guarded(torch, need)
    out = (C.c_uint8 * count)(*([0xEE] * count))
    assert L.trc_planes_advise_batch_dev(7, src.items(), count, esize, chunk, out, None, d_work.data_ptr(), need - 1, None) == E_WORK
    assert L.trc_planes_advise_batch_dev(8, src.items(), count, esize, chunk, out, None, d_work.data_ptr(), need, None) == E_ARG
    torch.cuda.synchronize()
    assert list(out) == [0xEE] * count and (d_work.cpu().numpy() == 0xA5).all()
    assert L.trc_planes_advise_batch_dev(7, src.items(), count, esize, chunk, out, None, d_work.data_ptr(), need, None) == 0
    assert list(out) == [w[0] for w in want]
    assert (d_work.cpu().numpy()[need:] == 0xA5).all() and np.array_equal(src.buf.cpu().numpy(), src.img)


@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S))
def test_planes_batch_coder_auto(torch_cuda, codec):
    """filters="auto" codes byte for byte what the chosen list codes, and decodes with it"""
    torch = torch_cuda
    esize, chunk = 4, 256
    datas, ms, want = advice_batch(esize, chunk)
    datas, want = datas[:8], want[:8]                          # the four kinds at 2 049 and 5 220 elements
    src = Packed(torch, datas, seed=9)
    auto = trc.PlanesBatchCoder(codec, src.views(), chunk, guard=GUARD, esize=esize, filters="auto")
    assert auto.filters is None and auto.advice is None
    auto.encode()
    chosen = list(auto.filters)
    assert chosen == [w[0] for w in want] == list(A_CHOICE) * 2
    ABL.assert_advice(chosen, auto.advice, want, AL.ALL, esize, ms[:8], "PlanesBatchCoder")
    explicit = trc.PlanesBatchCoder(codec, src.views(), chunk, guard=GUARD, esize=esize, filters=chosen)
    explicit.encode()
    assert_same_outputs(torch, auto, explicit, codec, esize, trc.CODEC_NAMES[codec] + " auto")
    assert auto.stored_bytes() == explicit.stored_bytes()
    assert np.array_equal(src.buf.cpu().numpy(), src.img), "encode changed its input"
    decodes_whole_batch(torch, src, auto, trc.CODEC_NAMES[codec] + " auto")
    dst = Packed(torch, datas, seed=9, data=False)
    auto.decode(5, 1, out=dst.views(range(5, 6)))
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(5, 6))), "decode of one middle item"
    assert auto.guards_ok() and explicit.guards_ok()
