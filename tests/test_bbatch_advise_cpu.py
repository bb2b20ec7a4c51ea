"""The advisor of a batch against a base per item and the host-pointer calls of the TRCE container, the parts that need no GPU:
trc_planes_advise_bbatch against advise_lib on the histograms of bplanes_lib.hist (an item with no base included), the choices the
GPU tests rely on, and what the new entry points refuse before they look for a device."""
import ctypes as C

import numpy as np
import pytest

import advise_lib as AL
import bbatch_container_lib as EL
import bplanes_lib as BP
import trc

E_ARG = -1
FAKE = 1 << 20                                                 # an aligned address nobody dereferences: the calls refuse first


def err():
    return trc.lib().trc_last_error().decode()


def items_of(datas):
    return trc.planes_items([(None, d.size) for d in datas])


@pytest.mark.parametrize("esize", (2, 4, 8))
@pytest.mark.parametrize("filters", range(1, 8))
def test_advise_bbatch_is_advise_per_item(esize, filters):
    datas, bases = BP.gen_batch(esize, [300, 64, 1000, 7, 513, 2049, 1, 256], 40 + esize)
    bases[2] = bases[5] = None                                  # no base: the unfiltered row alone
    count = len(datas)
    ptrs = [None if b is None else FAKE + 16 * i for i, b in enumerate(bases)]
    if not filters & 1:                                         # an item without a base has nothing to be judged by
        _, hists = EL.advise(datas, [b if b is not None else d for b, d in zip(bases, datas)], esize, filters)
        with pytest.raises(trc.TrcError, match="item 2"):
            trc.planes_advise_batch(hists, filters, esize, items_of(datas), count, bases=ptrs)
        ptrs = [FAKE + 16 * i for i in range(count)]
        bases = [b if b is not None else d for b, d in zip(bases, datas)]
    want, hists = EL.advise(datas, bases, esize, filters)
    got, adv = trc.planes_advise_batch(hists, filters, esize, items_of(datas), count, bases=ptrs)
    assert got == want
    for i, (d, b) in enumerate(zip(datas, bases)):
        f = filters & (7 if b is not None else 1)
        one = trc.planes_advise(hists[i], f, esize, d.size // esize)
        assert all(np.array_equal(adv[i][k], one[k]) for k in one) and adv[i]["filter"] == want[i] and adv[i]["filters"] == f, "item %d" % i
        assert b is not None or got[i] == BP.NONE, "an item with no base was given a filter"
    if filters == 7:
        assert len(set(got)) > 1, "every item got the same filter: the batch decides nothing"


def test_advise_bbatch_refusals():
    datas, bases = BP.gen_batch(2, [300, 64], 1)
    _, hists = EL.advise(datas, bases, 2)
    L = trc.lib()
    out = (C.c_uint8 * 2)(9, 9)
    it, b = items_of(datas), trc.planes_bases([FAKE, FAKE], 2)
    assert L.trc_planes_advise_bbatch(hists.ctypes.data, 7, 2, it, b, 0, out, None) == E_ARG and "0 items" in err()
    assert L.trc_planes_advise_bbatch(hists.ctypes.data, 8, 2, it, b, 2, out, None) == E_ARG and "filters 0x8" in err()
    assert L.trc_planes_advise_bbatch(hists.ctypes.data, 7, 3, it, b, 2, out, None) == E_ARG and "esize 3" in err()
    assert L.trc_planes_advise_bbatch(None, 7, 2, it, b, 2, out, None) == E_ARG
    bad = hists.copy()
    bad[1, 1, 0, 0] += 1                                        # a row that does not sum to the item's elements
    assert L.trc_planes_advise_bbatch(bad.ctypes.data, 7, 2, it, b, 2, out, None) == E_ARG and "item 1" in err()
    assert list(out) == [9, 9], "a failing call wrote to filters_out"
    assert L.trc_planes_advise_bbatch(bad.ctypes.data, 7, 2, it, trc.planes_bases([FAKE, None], 2), 2, out, None) == 0      # (rows 1 and 2 of item 1 are not looked at)
    assert L.trc_planes_advise_bbatch(hists.ctypes.data, 7, 2, it, None, 2, out, None) == 0 and list(out) == [0, 0]         # no bases at all: no filter


@pytest.mark.parametrize("esize", (2, 4, 8))
def test_the_auto_batches_decide_what_the_gpu_tests_expect(esize):
    """with the seeds fixed in bbatch_container_lib: the "drift" / "same" pairs choose filters (the item without a base none), and
    the 1/64 rule leaves every "random" pair unfiltered, which makes that batch a TRCB container"""
    items, bases = EL.auto_batch("pairs", esize)
    choice, _ = EL.advise(items, bases, esize)
    assert choice[3] == BP.NONE and all(c != BP.NONE for i, c in enumerate(choice) if i != 3), choice
    items, bases = EL.auto_batch("random", esize)
    choice, hists = EL.advise(items, bases, esize)
    assert choice == [BP.NONE] * len(items), choice
    for h, d in zip(hists, items):                              # ... by the rule, not by a tie: the gain is below 1/64 of the plain estimate
        _, _, total = AL.advise(h, 7, esize, d.size // esize)
        assert total[0] - min(total[1], total[2]) < total[0] / 64


def test_hist_and_host_calls_refuse_before_any_device():
    L = trc.lib()
    items = trc.planes_items([(FAKE, 600), (FAKE + 4096, 512)])
    bases = trc.planes_bases([FAKE, FAKE + 4096], 2)
    tb = L.trc_planes_batch_table_bytes(2, 3)

    def hist(filters=7, count=2, fi=0, ic=2, esize=2, chunk=256, bases=bases, d_hist=FAKE, d_table=FAKE, table_bytes=tb, items=items):
        return L.trc_planes_hist_bbatch_dev(filters, items, bases, count, fi, ic, esize, chunk, d_hist, d_table, table_bytes, None)
    assert hist(count=0) == E_ARG and "0 items" in err()
    assert hist(esize=3) == E_ARG and hist(chunk=100) == E_ARG
    assert hist(filters=0) == E_ARG and "filters 0x0" in err()
    assert hist(filters=8) == E_ARG and "filters 0x8" in err()
    assert hist(fi=1, ic=2) == E_ARG and "items [1, 1 + 2) of 2" in err()
    assert hist(items=trc.planes_items([(FAKE + 8, 600), (FAKE, 512)])) == E_ARG and "item 0" in err()
    assert hist(bases=trc.planes_bases([FAKE, FAKE + 8], 2)) == E_ARG and "item 1: the base" in err()
    assert hist(d_hist=FAKE + 4) == E_ARG and "histograms" in err()
    assert hist(d_table=FAKE + 64) == E_ARG and "256-byte" in err()
    assert hist(table_bytes=tb - 1) == -3
    assert hist(ic=0, d_hist=None, d_table=None) == 0
    assert hist(filters=8, fi=1, ic=2) == E_ARG and "filters 0x8" in err()                     # the bit set before the range

    out = np.zeros(1 << 16, dtype=np.uint8)
    f = trc.planes_filters([1, 2], 2)

    def enc(codec=trc.RCA, filters=f, count=2, bases=bases, items_on=trc.ITEMS_DEV, chunk=256):
        return L.trc_encode_bplanes_batch_host(codec, items, bases, filters, count, 2, chunk, 0, items_on, out.ctypes.data, out.size)
    assert enc(codec=trc.RCA4) == 0 and "low four bits" in err()
    assert enc(codec=99) == 0
    assert enc(count=0) == 0 and "0 items" in err()
    assert enc(items_on=7) == 0
    assert enc(filters=trc.planes_filters([1, 3], 2)) == 0 and "item 1: filter 3" in err()
    assert enc(filters=trc.planes_filters([0, 0], 2)) == 0 and "trc_encode_planes_batch_host" in err()
    assert enc(filters=None) == 0 and "TRCB" in err()
    assert enc(bases=trc.planes_bases([FAKE, None], 2)) == 0 and "item 1: a filter against a base needs the base" in err()
    assert enc(bases=None) == 0 and "item 0" in err()
    assert enc(chunk=100) == 0
    assert L.trc_encode_abplanes_batch_host(trc.RCA4, items, bases, 2, 2, 256, 0, trc.ITEMS_DEV, out.ctypes.data, out.size, None) == 0 and "low four bits" in err()
    assert L.trc_encode_abplanes_batch_host(trc.RCA, items, bases, 0, 2, 256, 0, trc.ITEMS_DEV, out.ctypes.data, out.size, None) == 0 and "0 items" in err()
    assert not out.any()
    junk = np.arange(256, dtype=np.uint8)
    assert L.trc_decode_bplanes_batch_host(junk.ctypes.data, junk.size, items, bases, 2, 0, 2, trc.ITEMS_DEV) == 0 and "based batch container: bad magic" in err()
    assert L.trc_decode_bplanes_batch_host(junk.ctypes.data, 3, items, bases, 2, 0, 2, trc.ITEMS_DEV) == 0 and "based batch container:" in err()
    assert L.trc_decode_bplanes_batch_host(None, 0, items, bases, 2, 0, 2, trc.ITEMS_DEV) == 0
    assert L.trc_decode_bplanes_batch_host(junk.ctypes.data, junk.size, items, bases, 2, 0, 2, 5) == 0
