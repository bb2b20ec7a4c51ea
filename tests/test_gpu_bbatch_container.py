"""A batch coded against a base per item in one piece, on the MI355X: the fingerprints of a batch's bases from one launch
(trc_base_fingerprint_batch_dev) against the numpy fingerprint, exactly; the TRCE container packed on the device against the model
container (bbatch_container_lib) byte for byte; its decode by item range and in place onto the bases; trc_base_verify_batch_dev;
the BasePlanesBatchCoder class.  Items and bases each lie in ONE allocation with 16 to 48 bytes of 0xA5 between them and no slack of
their own; every other device buffer is followed by a 512-byte guard of 0xA5."""
import numpy as np
import pytest

import bbatch_container_lib as EL
import bplanes_lib as BP
import fplanes_batch_lib as FBL
import planes_batch_lib as BL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, GUARD, PRM, Guarded, Packed, first_diff, guarded, ranges

pytestmark = pytest.mark.gpu
E_ARG, E_WORK = -1, -3
FP_SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 2049, 4097, 65539] + [2, 4, 5, 6]      # elements per item; the last four complete the n % 16 classes
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
CHUNKS = (256, 320, 4096)
W_SIZES = [1000, 256, 3000, 77, 513, 4097, 5, 2048]             # elements; 52 chunks of 256 with the pads


def base_views(bsrc, filters, only=None):
    """the bases of the filtered items of `only` (default: all); None for an unfiltered item and outside the range"""
    return [v if f != BP.NONE and (only is None or i in only) else None for i, (v, f) in enumerate(zip(bsrc.views(), filters))]


def cdfnum_of(codec):
    return 256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0


# ---- the batched fingerprint -----------------------------------------------------------------------------------------------------
def fingerprint_case(torch, esize, name):
    """"random" bases (the weighted sum wraps), mixed filters with NULL bases at the unfiltered items, every range of ranges(count):
    d_fp between guards, a table of exactly the required size with a guard behind it, the bases unchanged"""
    bases = [BP.gen_pair("random", esize, m, 0, 31 * esize + i)[1] for i, m in enumerate(FP_SIZES)]
    count = len(bases)
    assert min(b.size for b in bases) < 16 and {b.size % 16 for b in bases} == {esize * k % 16 for k in range(8)}, "a base below one 16-byte word, every rest"
    filters = FBL.assignments(count, 5 + esize)[name]
    assert name != "cycle" or (BP.NONE in filters and BP.ZDELTA in filters and BP.XOR in filters)
    bsrc = Packed(torch, bases, seed=esize + 1)
    items = trc.planes_items([(None, b.size) for b in bases])   # no d_ptr is looked at
    want = [0 if f == BP.NONE else BP.fingerprint(b) for b, f in zip(bases, filters)]
    assert any(w >> 63 for w in want), "no fingerprint with the top bit set"
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        tb = trc.lib().trc_base_fingerprint_batch_table_bytes(ic)
        d_fp, d_table = Guarded(torch, 8 * ic), guarded(torch, tb)
        trc.base_fingerprint_batch(items, base_views(bsrc, filters, only), filters, count, fi, ic, d_fp.t, d_table, tb)
        torch.cuda.synchronize()
        got, intact = d_fp.get()
        tag = "esize %d filters %s items (%d, %d)" % (esize, name, fi, ic)
        assert [int(x) for x in got.view("<u8")] == want[fi:fi + ic], tag
        assert intact, tag + ": the call wrote outside d_fp"
        assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": the call wrote behind its table"
    assert bsrc.unchanged(), "the call changed a base, a gap or the guard"


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_fingerprint_batch(torch_cuda, esize):
    for name in ("cycle", "delta"):
        fingerprint_case(torch_cuda, esize, name)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_fingerprint_batch_grid_stride_loop(torch_cuda, esize, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", "3")                  # three workgroups: the long item spans them, the short ones share one
    fingerprint_case(torch_cuda, esize, "cycle")


def test_fingerprint_batch_is_the_single_call_and_the_host_call(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    bases = [rng.integers(0, 256, n, dtype=np.uint8) for n in (1 << 20, 4096, 100, 3 * 4096 + 24, 16, 15)]
    bsrc = Packed(torch, bases, seed=2)
    count = len(bases)
    tb = trc.lib().trc_base_fingerprint_batch_table_bytes(count)
    d_fp, d_table = guarded(torch, 8 * count), guarded(torch, tb)
    trc.base_fingerprint_batch(trc.planes_items([(None, b.size) for b in bases]), bsrc.views(), 2, count, 0, count, d_fp, d_table, tb)
    got = [int(x) for x in d_fp.cpu().numpy()[:8 * count].view("<u8")]
    assert got == [trc.base_fingerprint_host(b) for b in bases] == [BP.fingerprint(b) for b in bases]
    single = []
    for v in bsrc.views():
        d1 = guarded(torch, 8)
        trc.base_fingerprint_enqueue(v, v.numel(), d1)
        single.append(int(d1.cpu().numpy()[:8].view("<u8")[0]))
    assert got == single
    # all NONE / no filters: zeros, no base looked at
    d_fp2 = guarded(torch, 8 * count)
    trc.base_fingerprint_batch(trc.planes_items([(None, b.size) for b in bases]), None, None, count, 0, count, d_fp2, d_table, tb)
    assert not d_fp2.cpu().numpy()[:8 * count].any() and (d_fp2.cpu().numpy()[8 * count:] == 0xA5).all()


# ---- the coded batch and its container ---------------------------------------------------------------------------------------------
_cache = {}


def coded(torch, codec, esize, name, chunk=CHUNK):
    """-> dict(src, bsrc, filters, bc holding the coded batch, cont: the packed container on the host, want: the model's): once per key"""
    key = (codec, esize, name, chunk)
    if key not in _cache:
        datas, bases = BP.gen_batch(esize, W_SIZES, 50 + esize)
        filters = FBL.assignments(len(datas), 9 + esize)[name]
        src, bsrc = Packed(torch, datas, seed=esize), Packed(torch, bases, seed=esize + 1)
        bc = trc.BasePlanesBatchCoder(codec, src.views(), chunk, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters, bases=base_views(bsrc, filters))
        bc.encode()
        d_cont, size = bc.pack(guard=GUARD)
        torch.cuda.synchronize()
        tag = "%s esize %d chunk %d filters %s" % (trc.CODEC_NAMES[codec], esize, chunk, name)
        assert bc.guards_ok(), tag + ": encode or pack wrote behind one of the coder's buffers"
        assert src.unchanged() and bsrc.unchanged(), tag + ": encode or pack changed an item or a base"
        virtual = BP.virtual_batch(datas, bases, filters, esize, chunk)
        want = EL.expected(datas, bases, filters, esize, chunk, trc.host_encode_planes(codec, virtual, esize, chunk, cdfnum=256, prm=PRM))
        _cache[key] = dict(src=src, bsrc=bsrc, filters=filters, bc=bc, size=size, cont=d_cont.cpu().numpy().copy(), tag=tag,
                           guard=bc.pack_guard.cpu().numpy().copy(), want=want, datas=datas, bases=bases)
    return _cache[key]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("codec", CODECS)
def test_pack_is_the_model_container(torch_cuda, codec, chunk):
    for esize, name in ((2, "cycle"), (4, "delta"), (8, "cycle")) if chunk != CHUNK else [(e, n) for e in PL.ESIZES for n in ("cycle", "delta", "random")]:
        p = coded(torch_cuda, codec, esize, name, chunk)
        sizes, count = p["src"].sizes, len(p["datas"])
        bound = trc.planes_bbatch_bound(codec, sizes, esize, chunk, cdfnum_of(codec))
        assert p["size"] == p["want"].size <= bound - trc.PAD, p["tag"] + ": *d_size is %d, the model has %d bytes" % (p["size"], p["want"].size)
        assert np.array_equal(p["cont"], p["want"]), p["tag"] + ": the container differs at byte %d" % first_diff(p["cont"], p["want"])
        assert p["guard"].size == bound + GUARD - p["size"] and (p["guard"] == 0xA5).all(), p["tag"] + ": a byte at or behind d_out + size was written"
        trc.planes_bbatch_check(p["cont"], count)
        prefix = EL.prefix_bytes(count)
        trc.planes_batch_check(p["cont"][prefix:], count)       # the TRCB part as it stands
        info = trc.parse_planes_bbatch(p["cont"])
        assert info["n"] == sizes and info["filters"] == list(p["filters"]) and info["codec"] == codec and info["prefix"] == prefix
        assert info["base_fp"] == EL.fingerprints(p["bases"], p["filters"], sizes)


def test_pack_refusals_and_failed_status(torch_cuda):
    torch = torch_cuda
    L = trc.lib()
    p = coded(torch, trc.ANS4S, 4, "cycle")
    bc = p["bc"]
    bound = trc.planes_bbatch_bound(bc.codec, p["src"].sizes, 4, CHUNK, 256)
    out = guarded(torch, bound)
    d_size = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda:0")
    tb = bc.table_bytes
    table = guarded(torch, tb)

    def call(filters=bc.filters, bases=bc.bases, out_bytes=bound, d_out=out.data_ptr(), table_bytes=tb, status=bc.status):
        return L.trc_planes_bbatch_pack_dev(bc.codec, bc.items, bases, filters, bc.count, 4, CHUNK, bc.cdf.data_ptr(), 256, status.data_ptr(), bc.clen.data_ptr(),
                                            bc.payload.data_ptr(), bc.total.data_ptr(), d_out, out_bytes, d_size.data_ptr(), table.data_ptr(), table_bytes, bc._stream())
    assert call(filters=trc.planes_filters(0, bc.count)) == E_ARG and "trc_planes_batch_pack_dev" in L.trc_last_error().decode()
    assert call(filters=None) == E_ARG and "TRCB" in L.trc_last_error().decode()
    assert call(out_bytes=bound - 1) == E_WORK
    assert call(table_bytes=tb - 1) == E_WORK
    assert call(d_out=out.data_ptr() + 8) == E_ARG and "16-byte" in L.trc_last_error().decode()
    assert call(bases=None) == E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and (table.cpu().numpy() == 0xA5).all() and int(d_size.item()) == 0x5A5A, "a rejected call wrote"
    # a failing static status: *d_size == 0, nothing behind the bound
    bad = bc.status.clone()
    bad[:4] = torch.from_numpy(np.array([-1], dtype="<i4").view(np.uint8)).to("cuda:0")
    assert call(status=bad) == 0
    torch.cuda.synchronize()
    assert int(d_size.item()) == 0 and (out.cpu().numpy()[bound:] == 0xA5).all() and (table.cpu().numpy()[tb:] == 0xA5).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(d_size.item()) == p["size"] and np.array_equal(out.cpu().numpy()[:p["size"]], p["want"])
    assert (out.cpu().numpy()[p["size"]:] == 0xA5).all(), "a byte at or behind d_out + size was written"


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_packed(torch_cuda, codec, esize):
    torch = torch_cuda
    L = trc.lib()
    for name in ("cycle", "delta"):
        p = coded(torch, codec, esize, name)
        bc, src, bsrc, filters = p["bc"], p["src"], p["bsrc"], p["filters"]
        total = trc.parse_planes_bbatch(p["cont"])["total"]
        d_cont = bc.packed                                      # the container with what is left of the bound behind it
        for fi, ic in ranges(bc.count):
            only = range(fi, fi + ic)
            dst = src.blank()
            need = L.trc_planes_bbatch_range_work_bytes(codec, dst.items(only), bc.count, esize, bc.chunk, fi, ic)
            bc.range_work, bc.range_work_bytes = None, 0        # a workspace of exactly the required size, guarded, for every range
            bc.decode_packed(d_cont, total, fi, ic, out=dst.views(only), cont_bytes=p["size"], bases=base_views(bsrc, filters, only))
            assert bc.range_work_bytes == need > 0
            torch.cuda.synchronize()
            tag = p["tag"] + " items (%d, %d)" % (fi, ic)
            assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag
            assert bc.guards_ok(), tag
        # in place: the bases' own allocation becomes the items
        inp = Packed(torch, bsrc.datas, seed=esize + 1)
        bc.decode_packed(d_cont, total, out=inp.views(), bases=inp.views())
        torch.cuda.synchronize()
        assert np.array_equal(inp.buf.cpu().numpy(), BL.image(src.datas, inp.offs, inp.total)), p["tag"] + ": the decode in place"
        assert np.array_equal(d_cont[:p["size"]].cpu().numpy(), p["want"]) and src.unchanged() and bsrc.unchanged(), p["tag"] + ": decode changed the container, an item or a base"
    with pytest.raises(trc.TrcError, match="rc=-3"):
        bc.decode_packed(d_cont, total, work_bytes=need - 1)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        bc.decode_packed(d_cont, total, cont_bytes=p["size"] - 1)


# ---- verify ----------------------------------------------------------------------------------------------------------------------
def test_verify(torch_cuda):
    torch = torch_cuda
    esize = 4
    datas, bases = BP.gen_batch(esize, [300, 64, 300, 1000, 7, 300, 64], 11)
    bases[5] = (bases[2] ^ np.uint8(1)).copy()                  # (equal lengths, different bytes: items 2 and 5, items 1 and 6)
    filters = [1, 2, 1, 0, 2, 2, 1]
    src, bsrc = Packed(torch, datas, seed=1), Packed(torch, bases, seed=2)
    bc = trc.BasePlanesBatchCoder(trc.RCA, src.views(), CHUNK, guard=GUARD, esize=esize, filters=filters, bases=base_views(bsrc, filters))
    bc.encode()
    d_cont, _ = bc.pack(guard=GUARD)
    assert bc.verify(d_cont) == -1
    assert all(bc.verify(d_cont, first_item=fi, item_count=ic) == -1 for fi, ic in ranges(bc.count))
    assert bc.verify(d_cont, first_item=3, item_count=0) == -1

    def flipped(*which):
        b = [x.copy() for x in bases]
        for i in which:
            b[i][b[i].size // 2] ^= 0x10
        return base_views(Packed(torch, b, seed=2), filters)
    assert bc.verify(d_cont, bases=flipped(4)) == 4
    assert bc.verify(d_cont, bases=flipped(5, 2)) == 2
    assert bc.verify(d_cont, bases=flipped(3)) == -1            # an unfiltered item's base is not looked at
    assert bc.verify(d_cont, bases=flipped(2, 5), first_item=3, item_count=4) == 5
    assert bc.verify(d_cont, bases=flipped(2), first_item=3, item_count=4) == -1      # a wrong base outside the range
    v = base_views(bsrc, filters)
    v[2], v[5] = v[5], v[2]                                     # two bases of equal length swapped
    assert bc.verify(d_cont, bases=v) == 2
    v = base_views(bsrc, filters)
    v[1], v[6] = v[6], v[1]
    assert bc.verify(d_cont, bases=v) == 1
    assert bc.guards_ok() and src.unchanged() and bsrc.unchanged() and (bc.pack_guard == 0xA5).all().item()


# ---- the class -------------------------------------------------------------------------------------------------------------------
def test_base_planes_batch_coder_round_trip(torch_cuda):
    torch = torch_cuda
    g = torch.Generator(device="cpu").manual_seed(1)
    base = [torch.randn(n, generator=g).to(torch.bfloat16).to("cuda:0") for n in (5000, 77, 4097)]
    new = [(b.float() + 1e-4 * torch.randn(b.numel(), generator=g).to("cuda:0")).to(torch.bfloat16) for b in base]
    keep = [t.clone() for t in new]
    with pytest.raises(ValueError):
        trc.BasePlanesBatchCoder(trc.RCA, new, chunk=512)
    bc = trc.BasePlanesBatchCoder(trc.RCA, new, chunk=512, guard=GUARD, filters=[1, 0, 2], bases=[base[0], None, base[2]])
    bc.encode()
    d_cont, size = bc.pack(guard=GUARD)
    host = d_cont.cpu().numpy()
    trc.planes_bbatch_check(host, 3)
    info = trc.parse_planes_bbatch(host)
    assert info["size"] + info["prefix"] == size and info["filters"] == [1, 0, 2]
    assert info["base_fp"] == [trc.base_fingerprint(base[0].view(torch.uint8)), 0, trc.base_fingerprint(base[2].view(torch.uint8))]
    assert bc.verify(d_cont) == -1 and bc.verify(d_cont, bases=[base[0], None, new[2]]) == 2
    for t in new:
        t.zero_()
    bc.decode_packed(d_cont, info["total"])
    torch.cuda.synchronize()
    assert all(torch.equal(t.view(torch.uint8), k.view(torch.uint8)) for t, k in zip(new, keep)) and bc.guards_ok()
    assert (bc.pack_guard == 0xA5).all().item()
