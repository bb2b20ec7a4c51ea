"""The advisor of a batch against a base per item and the host-pointer calls of the TRCE container, on the MI355X:
trc_planes_hist_bbatch_dev against bplanes_lib.hist per item (bit sets 1 .. 7, an item without a base, item ranges),
trc_planes_advise_bbatch_dev against its three pieces called by hand, trc_encode_bplanes_batch_host / trc_decode_bplanes_batch_host
with items on the device and on the host (the bases verified before anything is decoded), trc_encode_abplanes_batch_host against the
explicit call for the chosen list, and BasePlanesBatchCoder(filters="auto").  Every comparison is byte equality against the numpy
models; device buffers are followed by a 512-byte guard of 0xA5."""
import numpy as np
import pytest

import bbatch_container_lib as EL
import bplanes_lib as BP
import planes_batch_lib as BL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, GUARD, PRM, Guarded, Packed, assert_hists, guarded, ranges

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 2049, 4097, 65539]      # elements per item
NO_BASE = (3, 11)                                              # the items without a base


def hist_case(torch, esize, chunk=CHUNK, sets=range(1, 8)):
    datas, bases = BP.gen_batch(esize, SIZES, 300 + esize)
    count = len(datas)
    src, bsrc = Packed(torch, datas, seed=esize), Packed(torch, bases, seed=esize + 1)
    ms = [d.size // esize for d in datas]
    _, first = BL.plan(src.sizes, esize, chunk)
    for filters in sets:
        exp = [BP.hist(d, b, esize, filters & (1 if i in NO_BASE else 7)) for i, (d, b) in enumerate(zip(datas, bases))]
        for fi, ic in ranges(count) if filters in (5, 7) else [(0, count)]:
            only = range(fi, fi + ic)
            bv = [v if i in only and i not in NO_BASE else None for i, v in enumerate(bsrc.views())]
            tb = trc.lib().trc_planes_batch_table_bytes(ic, first[fi + ic] - first[fi])
            hb = trc.planes_hist_batch_bytes(ic, esize)
            d_hist, d_table = Guarded(torch, hb), guarded(torch, tb)
            trc.planes_hist_bbatch(filters, src.items(only), bv, count, fi, ic, esize, chunk, d_hist.t, d_table, tb)
            torch.cuda.synchronize()
            raw, intact = d_hist.get()
            tag = "esize %d chunk %d filters %d items (%d, %d)" % (esize, chunk, filters, fi, ic)
            assert intact, tag + ": the call wrote outside the histograms of its range"
            assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": the call wrote behind its table"
            got = raw.view("<u8").reshape(ic, 3, esize, 256)
            for j, i in enumerate(only):                        # (assert_hists wants one bit set for all items: item by item)
                assert_hists(got[j:j + 1], exp[i][None], ms[i:i + 1], filters & (1 if i in NO_BASE else 7), tag + " item %d" % i)
    assert src.unchanged() and bsrc.unchanged(), "the call changed an item, a base, a gap or the guard"


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_hist_bbatch(torch_cuda, esize):
    hist_case(torch_cuda, esize)


def test_hist_bbatch_grid_and_flush_edges(torch_cuda, monkeypatch):
    hist_case(torch_cuda, 4, chunk=4096, sets=(7,))
    monkeypatch.setenv("TRC_PLANES_GRID", "3")                  # the long item spans workgroups, the short ones share one
    hist_case(torch_cuda, 2, sets=(7, 6))
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "3")       # a flush every three vectors: the long item's rows arrive by atomics
    hist_case(torch_cuda, 8, sets=(7,))


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_advise_bbatch_dev_is_its_three_pieces(torch_cuda, esize, monkeypatch):
    torch = torch_cuda
    datas, bases = EL.auto_batch("pairs", esize)
    more, mb = BP.gen_batch(esize, [300, 64, 2049], 7 + esize)
    datas, bases = datas + more, bases + mb
    count = len(datas)
    src = Packed(torch, datas, seed=esize)
    bsrc = Packed(torch, [b if b is not None else np.zeros(16, np.uint8) for b in bases], seed=esize + 1)
    bv = [v if b is not None else None for v, b in zip(bsrc.views(), bases)]
    want, hists = EL.advise(datas, bases, esize)
    # by hand: the histograms, their copy, the host's choice
    _, first = BL.plan(src.sizes, esize, CHUNK)
    tb = trc.lib().trc_planes_batch_table_bytes(count, first[count])
    d_hist, d_table = guarded(torch, trc.planes_hist_batch_bytes(count, esize)), guarded(torch, tb)
    trc.planes_hist_bbatch(7, src.items(), bv, count, 0, count, esize, CHUNK, d_hist, d_table, tb)
    h = d_hist.cpu().numpy()[:trc.planes_hist_batch_bytes(count, esize)].view("<u8").reshape(count, 3, esize, 256)
    assert np.array_equal(h, hists)
    by_hand, adv_hand = trc.planes_advise_batch(h, 7, esize, src.items(), count, bases=bv)
    assert by_hand == want and len(set(want)) > 1
    for slab in (None, "2"):
        if slab:
            monkeypatch.setenv("TRC_PLANES_ADVISE_SLAB_ITEMS", slab)
        got, adv = trc.planes_advise_batch_dev(src.items(), esize, CHUNK, 7, count, "cuda:0", bases=bv)
        assert got == by_hand, "slab items %s" % slab
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(adv, adv_hand) for k in a)
    assert src.unchanged() and bsrc.unchanged()


# ---- host pointers ---------------------------------------------------------------------------------------------------------------
def model_container(codec, datas, bases, filters, esize, chunk):
    b = [x if x is not None else np.zeros(0, np.uint8) for x in bases]
    virtual = BP.virtual_batch(datas, b, filters, esize, chunk)
    return EL.expected(datas, b, filters, esize, chunk, trc.host_encode_planes(codec, virtual, esize, chunk, cdfnum=256, prm=PRM))


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA, trc.RCSS))
def test_host_encode_and_decode_both_ways(torch_cuda, codec, esize):
    torch = torch_cuda
    datas, bases = BP.gen_batch(esize, [1000, 256, 3000, 77, 513, 4097, 5, 2048], 50 + esize)
    count = len(datas)
    filters = [i % 3 for i in range(count)]
    hb = [b if f else None for b, f in zip(bases, filters)]
    want = model_container(codec, datas, bases, filters, esize, CHUNK)
    comp = trc.host_encode_bplanes_batch(codec, datas, hb, esize, CHUNK, filters, prm=PRM)
    assert np.array_equal(comp, want), "items on the host: the container differs from the model's"
    src, bsrc = Packed(torch, datas, seed=esize), Packed(torch, bases, seed=esize + 1)
    db = [v if f else None for v, f in zip(bsrc.views(), filters)]
    comp_dev = trc.host_encode_bplanes_batch(codec, src.views(), db, esize, CHUNK, filters, prm=PRM)
    assert np.array_equal(comp_dev, want), "items on the device: the container differs from the model's"
    assert src.unchanged() and bsrc.unchanged()
    trc.planes_bbatch_check(comp, count)
    # decode: whole and by range, host items
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        got = trc.host_decode_bplanes_batch(comp, [b if i in only else None for i, b in enumerate(hb)], fi, ic)
        assert all(np.array_equal(g, datas[i]) for g, i in zip(got, only)), "host items (%d, %d)" % (fi, ic)
    # device items, in a blank copy; then in place onto the bases
    for fi, ic in ((0, count), (2, 5)):
        only = range(fi, fi + ic)
        dst = src.blank()
        n = trc.host_decode_bplanes_batch(comp, [v if i in only else None for i, v in enumerate(db)], fi, ic, out=dst.views(only))
        assert n == sum(src.sizes[i] for i in only) and np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), "device items (%d, %d)" % (fi, ic)
    inp = Packed(torch, bases, seed=esize + 1)
    trc.host_decode_bplanes_batch(comp, inp.views(), out=inp.views())
    assert np.array_equal(inp.buf.cpu().numpy(), BL.image(datas, inp.offs, inp.total)), "the decode in place"
    assert bsrc.unchanged()


def test_host_decode_verifies_the_bases_of_the_range_only(torch_cuda):
    torch = torch_cuda
    esize, codec = 4, trc.RCA
    datas, bases = BP.gen_batch(esize, [1000, 256, 3000, 77, 513], 9)
    filters = [1, 2, 1, 0, 2]
    comp = trc.host_encode_bplanes_batch(codec, datas, bases, esize, CHUNK, filters)
    wrong = [b.copy() for b in bases]
    wrong[2][100] ^= 1
    # a wrong base outside the range is not looked at
    got = trc.host_decode_bplanes_batch(comp, wrong, 0, 2)
    assert np.array_equal(got[0], datas[0]) and np.array_equal(got[1], datas[1])
    got = trc.host_decode_bplanes_batch(comp, [None, None, None, None, bases[4]], 3, 2)
    assert np.array_equal(got[0], datas[3]) and np.array_equal(got[1], datas[4])
    # inside the range: 0, "base fingerprint", the item and both values; the outputs untouched
    with pytest.raises(trc.TrcError, match="item 2: base fingerprint 0x%016x, the container was coded against 0x%016x" % (BP.fingerprint(wrong[2]), BP.fingerprint(bases[2]))):
        trc.host_decode_bplanes_batch(comp, wrong, 1, 3)
    src = Packed(torch, datas, seed=1)
    dst, bsrc = src.blank(), Packed(torch, wrong, seed=2)
    with pytest.raises(trc.TrcError, match="item 2: base fingerprint"):
        trc.host_decode_bplanes_batch(comp, bsrc.views(), 0, 5, out=dst.views())
    assert dst.unchanged() and bsrc.unchanged(), "a refused decode wrote"
    outs = [np.full(d.size, 0x77, np.uint8) for d in datas]
    items = trc.planes_items([(o.ctypes.data, o.size) for o in outs])
    b = trc.planes_bases([x.ctypes.data for x in wrong], 5)
    assert trc.lib().trc_decode_bplanes_batch_host(comp.ctypes.data, comp.size, items, b, 5, 0, 5, trc.ITEMS_HOST) == 0
    assert all((o == 0x77).all() for o in outs), "a refused decode wrote to a host item"
    with pytest.raises(trc.TrcError, match="item 0"):           # a filtered item of the range without a base
        trc.host_decode_bplanes_batch(comp, [None] * 5, 0, 1)
    # the decoder reads a TRCB container; bases are ignored
    plain = trc.host_encode_planes_batch(codec, datas, esize, CHUNK, filters=[1, 0, 2, 0, 1])
    got = trc.host_decode_bplanes_batch(plain, None)
    assert all(np.array_equal(g, d) for g, d in zip(got, datas))
    got = trc.host_decode_bplanes_batch(plain, wrong, 1, 2)
    assert np.array_equal(got[0], datas[1]) and np.array_equal(got[1], datas[2])


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_host_encode_auto_is_the_explicit_call(torch_cuda, esize):
    torch = torch_cuda
    codec = trc.RCA
    datas, bases = EL.auto_batch("pairs", esize)
    want_filters, _ = EL.advise(datas, bases, esize)
    comp, chosen = trc.host_encode_bplanes_batch(codec, datas, bases, esize, CHUNK, "auto")
    assert chosen == want_filters and any(chosen) and chosen[3] == BP.NONE
    explicit = trc.host_encode_bplanes_batch(codec, datas, [b if f else None for b, f in zip(bases, chosen)], esize, CHUNK, chosen)
    assert np.array_equal(comp, explicit) and np.array_equal(comp, model_container(codec, datas, bases, chosen, esize, CHUNK))
    src = Packed(torch, datas, seed=esize)
    bsrc = Packed(torch, [b if b is not None else np.zeros(16, np.uint8) for b in bases], seed=esize + 1)
    comp_dev, chosen_dev = trc.host_encode_bplanes_batch(codec, src.views(), [v if b is not None else None for v, b in zip(bsrc.views(), bases)], esize, CHUNK, "auto")
    assert chosen_dev == chosen and np.array_equal(comp_dev, comp)
    got = trc.host_decode_bplanes_batch(comp, bases)
    assert all(np.array_equal(g, d) for g, d in zip(got, datas))
    # unrelated pairs: no filter anywhere, a TRCB container -- the one the plain call writes
    datas, bases = EL.auto_batch("random", esize)
    comp, chosen = trc.host_encode_bplanes_batch(codec, datas, bases, esize, CHUNK, "auto")
    assert chosen == [BP.NONE] * len(datas) and comp[:4].tobytes() == b"TRCB"
    assert np.array_equal(comp, trc.host_encode_planes_batch(codec, datas, esize, CHUNK))
    got = trc.host_decode_bplanes_batch(comp, bases)
    assert all(np.array_equal(g, d) for g, d in zip(got, datas))


def test_base_planes_batch_coder_auto(torch_cuda):
    torch = torch_cuda
    g = torch.Generator(device="cpu").manual_seed(1)
    base = [torch.randn(n, generator=g).to(torch.bfloat16).to("cuda:0") for n in (5000, 77, 4097)]
    new = [(b.float() + 1e-4 * torch.randn(b.numel(), generator=g).to("cuda:0")).to(torch.bfloat16) for b in base]
    new[1] = torch.randn(77, generator=g).to(torch.bfloat16).to("cuda:0")       # re-initialised: its base does not help
    keep = [t.clone() for t in new]
    bc = trc.BasePlanesBatchCoder(trc.RCA, new, chunk=512, guard=GUARD, filters="auto", bases=[base[0], base[1], None])
    bc.encode()
    chosen = list(bc.filters[:3])
    host = [t.view(torch.uint8).cpu().numpy() for t in new]
    hbase = [base[0].view(torch.uint8).cpu().numpy(), base[1].view(torch.uint8).cpu().numpy(), None]
    assert chosen == EL.advise(host, hbase, 2)[0] and chosen[0] != 0 and chosen[2] == 0 and len(bc.advice) == 3
    d_cont, size = bc.pack(guard=GUARD)
    info = trc.parse_planes_bbatch(d_cont.cpu().numpy())
    assert info["filters"] == chosen and bc.verify(d_cont) == -1
    for t in new:
        t.zero_()
    bc.decode_packed(d_cont, info["total"])
    torch.cuda.synchronize()
    assert all(torch.equal(t.view(torch.uint8), k.view(torch.uint8)) for t, k in zip(new, keep)) and bc.guards_ok()


# ---- the file tool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ("z", "a"))
def test_trcfile_based_batch(torch_cuda, tmp_path, letter):
    """trcfile e writes the library's container from pairs of files, E reads one item back against its base file and refuses
    another base, l lists the fingerprints"""
    from gpu_planes import trcfile
    esize = 2
    datas, bases = EL.auto_batch("pairs", esize)
    args, files = [], []
    for i, (d, b) in enumerate(zip(datas, bases)):
        fd, fb = str(tmp_path / ("item%d.bin" % i)), str(tmp_path / ("base%d.bin" % i))
        d.tofile(fd)
        if b is not None:
            b.tofile(fb)
        files.append((fd, fb if b is not None else "-"))
        args += [fd, fb if b is not None else "-"]
    comp = str(tmp_path / "batch.trce")
    r = trcfile("e", 46, esize, CHUNK, letter, comp, *args)
    filters = EL.advise(datas, bases, esize)[0] if letter == "a" else [BP.ZDELTA if b is not None else BP.NONE for b in bases]
    want = model_container(trc.RCA, datas, bases, filters, esize, CHUNK)
    got = np.fromfile(comp, dtype=np.uint8)
    assert np.array_equal(got, want), r.stdout
    if letter == "a":
        assert all("item %d: %d bytes, choice %s" % (i, d.size, "nzx"[f]) in r.stdout for i, (d, f) in enumerate(zip(datas, filters)))
    listing = trcfile("l", comp).stdout
    fps = EL.fingerprints([b if b is not None else d for b, d in zip(bases, datas)], filters, [d.size for d in datas])
    for i, (d, f) in enumerate(zip(datas, filters)):
        line = "item %d: %d bytes, filter %s" % (i, d.size, "nzx"[f]) + (", base %016x" % fps[i] if f else "")
        assert line + "\n" in listing, (line, listing)
    for i in (0, 3, 5):
        out = str(tmp_path / ("out%d.bin" % i))
        trcfile("E", comp, i, files[i][1], out)
        assert np.array_equal(np.fromfile(out, dtype=np.uint8), datas[i]), "item %d" % i
    r = trcfile("E", comp, 0, files[2][1], str(tmp_path / "no.bin"), rc=1)      # (a longer item's base: another fingerprint)
    assert "base fingerprint" in r.stderr and "item 0" in r.stderr
    trcfile("E", comp, len(datas), "-", str(tmp_path / "no.bin"), rc=2)
