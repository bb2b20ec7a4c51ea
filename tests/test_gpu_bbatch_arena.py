"""The calls of a batch coded against bases in one piece, on the MI355X, at the minimum buffers include/trc_hip.h documents, out of
the audited arena of tests/gpu_arena.py (helpers: tests/gpu_planes_arena.py), as test_gpu_planes_arena.py does for their siblings:
bases with NO slack at 16 bytes and no better, d_fp and *d_bad at 8, tables of exactly trc_base_fingerprint_batch_table_bytes at
256, the pack's d_out of exactly trc_planes_bbatch_bound at 16, the container a decode reads at 8 (mod 16), workspaces of exactly
trc_planes_bbatch_range_work_bytes.  Every case runs under both poisons, the whole allocation is audited against its image after
every library call, expected values come from the numpy models and the oracle, and the two runs' outputs must be the same."""
import ctypes as C

import numpy as np
import pytest

import bbatch_container_lib as EL
import gpu_arena as GA
import gpu_planes_arena as P
import planes_container_lib as CL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def both(run, tag, *args):
    a = run(*args, "random", 7)
    b = run(*args, "ff", 0)
    GA.same_outputs(a, b, tag)


def run_fingerprint_batch(torch, esize, poison, seed):
    """trc_base_fingerprint_batch_dev for every range of ranges(count): d_fp of exactly 8 bytes per item, a table of exactly its
    bytes, NULL bases outside the range and at the unfiltered items; the poison behind a base must not reach its value"""
    b = P.Batch("bbatch", esize)
    count, L = b.count, trc.lib()
    specs = b.base_specs()
    for j, (fi, ic) in enumerate(P.ranges(count)):
        specs += [("r%d.fp" % j, 8 * ic), ("r%d.table" % j, L.trc_base_fingerprint_batch_table_bytes(ic))]
    A = P.arena(torch, specs, poison, seed)
    for i, d in enumerate(b.bases):
        A.put("b%d.base" % i, d)
    want = EL.fingerprints(b.bases, b.filters, b.sizes)
    items = trc.planes_items([(None, n) for n in b.sizes])
    fl = trc.planes_filters(b.filters, count)
    got = dict(out=[])
    for j, (fi, ic) in enumerate(P.ranges(count)):
        tag = "fingerprint_batch esize %d items (%d, %d), poison %s" % (esize, fi, ic, poison)
        tb = A.layout["r%d.table" % j].size
        bases = (C.c_void_p * count)(*[A.ptr("b%d.base" % i) if fi <= i < fi + ic and b.filters[i] else None for i in range(count)])
        P.ok(A.call(lambda: L.trc_base_fingerprint_batch_dev(items, bases, fl, count, fi, ic, A.ptr("r%d.fp" % j), A.ptr("r%d.table" % j), tb, None), tag,
                    [("r%d.fp" % j, 0, 8 * ic), ("r%d.table" % j, 0, tb)]), tag)
        fp = A.get("r%d.fp" % j, 8 * ic).view("<u8").copy()
        assert [int(x) for x in fp] == want[fi:fi + ic], "%s: %r, the model has %r" % (tag, [hex(int(x)) for x in fp], [hex(x) for x in want[fi:fi + ic]])
        got["out"].append(fp)
    return got


def run_bbatch_container(torch, codec, poison, seed):
    """the coded batch packed by trc_planes_bbatch_pack_dev into exactly the bound's bytes at 16 with a table of exactly its bytes:
    the prefix is the model's, the TRCB part passes its checker and has the model's front; trc_base_verify_batch_dev on it; the
    container copied to 8 (mod 16), every item range decoded from there in an exact-size workspace, item 3 onto its own base"""
    b, x, specs, cdfnum, wb = P._coded_batch("bbatch", codec, "payload4")
    e, count, static, L = b.esize, b.count, codec in trc.STATIC, trc.lib()
    null = trc.planes_items([(16, n) for n in b.sizes])
    bound = L.trc_planes_bbatch_bound(codec, null, count, e, b.chunk, cdfnum)
    rwb = [L.trc_planes_bbatch_range_work_bytes(codec, null, count, e, b.chunk, fi, ic) for fi, ic in P.ranges(count)]
    tb = L.trc_base_fingerprint_batch_table_bytes(count)
    assert bound and all(rwb) and tb
    A = P.arena(torch, specs + [("packed.out", bound), ("size", 8), ("bad.size", 8), ("table", tb), ("cont", bound)] +
                [("r%d.range_work" % j, w) for j, w in enumerate(rwb)], poison, seed)
    b.put(A)
    name = trc.CODEC_NAMES[codec]
    kw = dict(coder="bbatch:" + name, allow=GA.PLANES_ALLOW)
    tag = "bbatch %s container, poison %s" % (name, poison)
    got = P._encode_batch(A, b, codec, cdfnum, wb, tag, kw, x, "payload4")
    totals = [int(p["payload"].size) for p in x]
    lay = trc.planes_batch_layout(codec, b.sizes, e, b.chunk, cdfnum, totals)
    prefix = EL.prefix_bytes(count)
    size = prefix + lay["size"]
    assert size <= bound - P.PAD
    fam_args = b.fam_args(A)
    P.ok(A.call(lambda: L.trc_planes_bbatch_pack_dev(codec, b.items(A), *fam_args, count, e, b.chunk, A.ptr("cdf") if static else None, cdfnum,
                                                     A.ptr("status") if static else None, A.ptr("clen"), A.ptr("payload4"), A.ptr("total"),
                                                     A.ptr("packed.out"), bound, A.ptr("size"), A.ptr("table"), tb, None),
                tag + ": pack", [("packed.out", 0, size), ("size", 0, 8), ("table", 0, tb)]), tag + ": pack")
    assert int(A.get("size", 8).view("<u8")[0]) == size, tag + ": *d_size is %d, the layout gives %d" % (int(A.get("size", 8).view("<u8")[0]), size)
    cont = A.get("packed.out", size)
    trc.planes_bbatch_check(cont, count)
    want = EL.prefix(EL.fingerprints(b.bases, b.filters, b.sizes))
    assert np.array_equal(cont[:prefix], want), tag + ": the prefix: " + P.PM.first_difference("prefix", cont[:prefix], want)
    body = cont[prefix:]
    trc.planes_batch_check(body, count)
    front = CL.front(b.sizes, b.filters, e, b.chunk, lay["size"])
    assert np.array_equal(body[:lay["inner"]], front), tag + ": header, n[] or filters"
    for k in range(e):
        o = lay["off"][k] + (CL.up8(2 * (cdfnum + 1)) if static else 0) + 32
        assert np.array_equal(body[o:o + 4 * b.NC].view("<u4"), x[k]["clen"]), tag + ": the directory of section %d" % k
        assert np.array_equal(body[o + 4 * b.NC:o + 4 * b.NC + totals[k]], x[k]["payload"]), tag + ": the payload of section %d" % k
    got["container"] = cont
    A.put("cont", cont)                                        # at 8 (mod 16); TRC_PAD readable bytes behind `size`: poison
    assert A.ptr("cont") % 16 == 8
    # verify: the right bases, then a longer item's base in the place of item 4's
    for what, onto, expect in (("the right bases", None, -1), ("another base for item 4", (4, "b6.base"), 4)):
        assert b.filters[4] and b.sizes[6] >= b.sizes[4]
        ptrs = b.base_ptrs(A, onto=onto)
        P.ok(A.call(lambda: L.trc_base_verify_batch_dev(A.ptr("cont"), b.items(A), ptrs, fam_args[1], count, 0, count, A.ptr("bad.size"), A.ptr("table"), tb, None),
                    "%s: verify, %s" % (tag, what), [("bad.size", 0, 8), ("table", 0, tb)]), tag + ": verify")
        bad = int(A.get("bad.size", 8).view("<i8")[0])
        assert bad == expect, "%s: verify, %s: *d_bad is %d" % (tag, what, bad)
    tot = (C.c_uint64 * 8)(*totals)

    def decode(what, fi, ic, work, onto=None):
        only = range(fi, fi + ic)
        for i in range(count):
            A.poison("o%d.item" % i)
        items = b.items(A, "o", only)
        dst = {i: "o%d.item" % i for i in only}
        if onto is not None:                                   # in place: the item's pointer is its base's
            items[onto].d_ptr = A.ptr("b%d.base" % onto)
            dst[onto] = "b%d.base" % onto
        wsize = A.layout[work].size
        w = [(dst[i], 0, b.sizes[i]) for i in only] + [(work, 0, wsize)]
        P.ok(A.call(lambda: L.trc_decode_bplanes_batch_packed_dev(codec, A.ptr("cont"), bound, items, *b.fam_args(A, only), count, fi, ic, e, b.chunk, cdfnum, tot,
                                                                  A.ptr(work), wsize, None), "%s: %s" % (tag, what), w, [GA.slack(A, work)], **kw), "%s: %s" % (tag, what))
        for i in only:
            o = A.get(dst[i], b.sizes[i])
            assert np.array_equal(o, b.datas[i]), "%s: %s: item %d: %s" % (tag, what, i, P.PM.first_difference("bytes", o, b.datas[i], chunk=b.chunk * e))
            got["out"].append(o)
        if onto is not None:
            A.put("b%d.base" % onto, b.bases[onto])

    for j, (fi, ic) in enumerate(P.ranges(count)):
        decode("packed decode of items (%d, %d)" % (fi, ic), fi, ic, "r%d.range_work" % j)
    assert b.filters[3] != 0 and P.ranges(count)[1] == (3, 1)
    decode("packed decode of item 3 onto its own base", 3, 1, "r1.range_work", onto=3)
    return got


NO_BASE = (5, 8)                                               # the items the advisor's cases leave without a base


def run_bbatch_hist(torch, esize, poison, seed):
    """trc_planes_hist_bbatch_dev, all three filters, for every range of ranges(count): histograms and table of exactly their bytes,
    NULL items and bases outside the range, two items without a base"""
    b = P.Batch("bbatch", esize)
    count, L = b.count, trc.lib()
    specs = b.item_specs() + b.base_specs()
    for j, (fi, ic) in enumerate(P.ranges(count)):
        specs += [("r%d.hist" % j, L.trc_planes_hist_batch_bytes(ic, esize)), ("r%d.table" % j, L.trc_planes_batch_table_bytes(ic, b.first[fi + ic] - b.first[fi]))]
    A = P.arena(torch, specs, poison, seed)
    b.put(A)
    got = dict(out=[])
    for j, (fi, ic) in enumerate(P.ranges(count)):
        tag = "hist bbatch esize %d items (%d, %d), poison %s" % (esize, fi, ic, poison)
        hb, tb = A.layout["r%d.hist" % j].size, A.layout["r%d.table" % j].size
        only = range(fi, fi + ic)
        items = b.items(A, only=only)
        bases = (C.c_void_p * count)(*[A.ptr("b%d.base" % i) if i in only and i not in NO_BASE else None for i in range(count)])
        P.ok(A.call(lambda: L.trc_planes_hist_bbatch_dev(7, items, bases, count, fi, ic, esize, b.chunk, A.ptr("r%d.hist" % j), A.ptr("r%d.table" % j), tb, None), tag,
                    [("r%d.hist" % j, 0, hb), ("r%d.table" % j, 0, tb)]), tag)
        h = A.get("r%d.hist" % j, hb).view("<u8").reshape(ic, 3, esize, 256).copy()
        for i in only:
            exp = P.BPL.hist(b.datas[i], b.bases[i], esize, 1 if i in NO_BASE else 7)
            assert np.array_equal(h[i - fi], exp), "%s: item %d: %s" % (tag, i, P.PM.first_difference("counters", h[i - fi], exp))
        got["out"].append(h)
    return got


def run_bbatch_advise(torch, esize, poison, seed):
    """trc_planes_advise_bbatch_dev in a workspace of exactly trc_planes_advise_batch_work_bytes: the model's choice per item"""
    b = P.Batch("bbatch", esize)
    count, L = b.count, trc.lib()
    null = trc.planes_items([(16, n) for n in b.sizes])
    wb = L.trc_planes_advise_batch_work_bytes(null, count, esize, b.chunk)
    assert wb
    A = P.arena(torch, b.item_specs() + b.base_specs() + [("work", wb)], poison, seed)
    b.put(A)
    tag = "advise_bbatch_dev esize %d, poison %s" % (esize, poison)
    out = (C.c_uint8 * count)()
    bases = (C.c_void_p * count)(*[A.ptr("b%d.base" % i) if i not in NO_BASE else None for i in range(count)])
    P.ok(A.call(lambda: L.trc_planes_advise_bbatch_dev(7, b.items(A), bases, count, esize, b.chunk, out, None, A.ptr("work"), wb, None), tag,
                [("work", 0, wb)]), tag)
    want = EL.advise(b.datas, [x if i not in NO_BASE else None for i, x in enumerate(b.bases)], esize)[0]
    assert [int(v) for v in out] == want, "%s: choices %r, the model has %r" % (tag, [int(v) for v in out], want)
    return dict(choice=np.array(list(out)))


@pytest.mark.parametrize("esize", P.ESIZES)
def test_bbatch_hist_and_advice(torch_cuda, esize):
    both(run_bbatch_hist, "hist bbatch esize %d" % esize, torch_cuda, esize)
    both(run_bbatch_advise, "advise_bbatch_dev esize %d" % esize, torch_cuda, esize)


@pytest.mark.parametrize("esize", P.ESIZES)
def test_fingerprint_batch(torch_cuda, esize):
    both(run_fingerprint_batch, "fingerprint_batch esize %d" % esize, torch_cuda, esize)


@pytest.mark.parametrize("codec", P.BATCH_CODERS, ids=lambda c: trc.CODEC_NAMES[c])
def test_bbatch_container(torch_cuda, codec):
    both(run_bbatch_container, "bbatch %s container" % trc.CODEC_NAMES[codec], torch_cuda, codec)
