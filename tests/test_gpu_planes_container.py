"""The TRCB container of a coded batch on the MI355X: the pack kernel (the whole container byte for byte against the numpy front
followed by the parent's trc_encode_planes_host on the materialised virtual buffer, the size, the guards), the decode of a packed
container where it lies, the host-pointer calls with host and device items, and `trcfile b / B / l`.  As in the other batch tests
the items lie in ONE allocation with 16 to 48 bytes of 0xA5 between them, and every comparison is byte equality."""
import numpy as np
import pytest

import fplanes_lib as FL
import planes_batch_lib as BL
import planes_container_lib as CL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, E_ARG, E_WORK, GUARD, PRM, Packed, guarded, item_ranges, trcfile

pytestmark = pytest.mark.gpu
CODECS = (trc.RCA, trc.ANS4S, trc.RCSS)
ESIZES = (2, 4, 8)
LENGTHS = [1, 255, 256, 257, 8 * 37 + 3, 2 * 256]              # elements per item: 9 chunks of 256, an odd NC
ORDERS = {"odd": LENGTHS, "even": LENGTHS + [256], "one": [8 * 37 + 3], "nc1": [255]}
FILTERS = ("none", "mixed", "zigzag")


def gen_items(esize, order, seed, turn=0):
    """uniform bytes (chunks stored raw: total == m), zeros (tiny totals) and sorted ids (zero high planes), by turns from `turn` on"""
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(order, turn):
        if i % 3 == 0:
            out.append(rng.integers(0, 256, m * esize, dtype=np.uint8))
        elif i % 3 == 1:
            out.append(np.zeros(m * esize, dtype=np.uint8))
        else:
            ids = np.cumsum(rng.integers(1, 200, m)).astype("<u%d" % esize)
            out.append(ids.view(np.uint8).copy())
    return out


def filters_of(name, count):
    return {"none": None, "mixed": [(i + 1) % 3 for i in range(count)], "zigzag": [FL.ZDELTA] * count}[name]


def cdfnum_of(codec):
    return 256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0


def expected_container(codec, datas, filters, esize, chunk):
    vf = CL.virtual_filtered(datas, filters, esize, chunk)
    return CL.expected(datas, filters, esize, chunk, trc.host_encode_planes(codec, vf, esize, chunk, cdfnum=256, prm=PRM))


_cache = {}


def packed(torch, codec, esize, fname, oname):
    """-> dict(src, filters, bc, cont: the packed container on the host, want: the expected one): once per key, shared, left unchanged"""
    key = (codec, esize, fname, oname)
    if key not in _cache:
        datas = gen_items(esize, ORDERS[oname], 7 * esize + len(oname), 2 if len(ORDERS[oname]) == 1 else 0)      # one item: sorted ids
        filters = filters_of(fname, len(datas))
        src = Packed(torch, datas, seed=esize)
        bc = trc.PlanesBatchCoder(codec, src.views(), CHUNK, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters)
        bc.encode()
        d_cont, size = bc.pack(guard=GUARD)
        torch.cuda.synchronize()
        tag = "%s esize %d filters %s items %s" % (trc.CODEC_NAMES[codec], esize, fname, oname)
        assert bc.guards_ok(), tag + ": pack wrote behind one of the coded buffers"
        assert np.array_equal(src.buf.cpu().numpy(), src.img), tag + ": the items changed"
        _cache[key] = dict(src=src, filters=filters, bc=bc, size=size, cont=d_cont.cpu().numpy().copy(), tag=tag,
                           guard=bc.pack_guard.cpu().numpy().copy(), want=expected_container(codec, datas, filters, esize, CHUNK))
    return _cache[key]


def all_cases():
    return [(c, e, f, o) for c in CODECS for e in ESIZES for f in FILTERS for o in ("odd", "even")] + \
           [(c, e, "mixed", o) for c in CODECS for e in ESIZES for o in ("one", "nc1")]


# ---- pack ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_pack_is_the_host_container(torch_cuda, codec, esize):
    for c, e, fname, oname in all_cases():
        if (c, e) != (codec, esize):
            continue
        p = packed(torch_cuda, codec, esize, fname, oname)
        bound = trc.planes_batch_bound(codec, p["src"].sizes, esize, CHUNK, cdfnum_of(codec))
        assert p["size"] == p["want"].size <= bound - trc.PAD, p["tag"] + ": *d_size"
        assert np.array_equal(p["cont"], p["want"]), p["tag"] + ": the container differs at byte %d" % \
            int(np.flatnonzero(p["cont"] != p["want"][:p["cont"].size])[0] if p["cont"].size == p["want"].size else -1)
        assert p["guard"].size == bound + GUARD - p["size"] and (p["guard"] == 0xA5).all(), p["tag"] + ": a byte at or behind d_out + size was written"
        trc.planes_batch_check(p["cont"], len(p["src"].sizes))
        info = trc.parse_planes_batch(p["cont"])
        assert info["n"] == p["src"].sizes and info["filters"] == (p["filters"] or [0] * len(info["n"])) and info["codec"] == codec
        lay = trc.planes_batch_layout(codec, info["n"], esize, CHUNK, cdfnum_of(codec), info["total"])
        assert (lay["inner"], lay["off"], lay["size"]) == (info["inner"], info["off"], info["size"])


def test_case_list_covers_the_alignments(torch_cuda):
    """the data must keep providing what the kernel's head / body / tail logic can get wrong: payload sizes that are no multiple of
    8 and of 4, a payload destination that is only 4-byte aligned (odd NC) and one that is 8-byte aligned (even NC), one item, one chunk"""
    totals, ncs, counts = [], set(), set()
    for key in all_cases():
        p = packed(torch_cuda, *key)
        info = trc.parse_planes_batch(p["cont"])
        totals += info["total"]
        ncs.add(p["bc"].nch)
        counts.add(p["bc"].count)
        pl, _ = BL.plan(p["src"].sizes, key[1], CHUNK)
        assert p["bc"].nch == pl["chunks"]
    assert any(t % 8 for t in totals) and any(t % 4 for t in totals)
    assert any(nc % 2 for nc in ncs) and any(nc % 2 == 0 for nc in ncs) and 1 in ncs and 1 in counts
    raw = [p for key in all_cases() for p in [packed(torch_cuda, *key)] if key[2] == "none" and key[3] == "odd"]
    assert any(max(trc.parse_planes_batch(p["cont"])["total"]) >= sum(LENGTHS[::3]) for p in raw), "no plane with chunks stored raw"
    assert any(0 < t < 64 for t in totals), "no plane with a tiny payload"


def test_pack_grid_stride_loop_and_argument_errors(torch_cuda, monkeypatch):
    torch = torch_cuda
    L = trc.lib()
    p = packed(torch, trc.RCA, 4, "mixed", "even")
    bc = p["bc"]
    monkeypatch.setenv("TRC_PLANES_GRID", "1")                  # one workgroup takes every tile
    d_cont, size = bc.pack(guard=GUARD)
    assert size == p["size"] and np.array_equal(d_cont.cpu().numpy(), p["want"]) and (bc.pack_guard == 0xA5).all().item()
    monkeypatch.delenv("TRC_PLANES_GRID")
    bound = trc.planes_batch_bound(bc.codec, p["src"].sizes, 4, CHUNK, 0)
    out = guarded(torch, bound)
    d_size = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda:0")

    def call(codec=bc.codec, filters=bc.filters, out_bytes=bound, d_out=out.data_ptr(), chunk=CHUNK):
        return L.trc_planes_batch_pack_dev(codec, bc.items, filters, bc.count, 4, chunk, None, 0, None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                           bc.total.data_ptr(), d_out, out_bytes, d_size.data_ptr(), bc._stream())
    assert call(out_bytes=bound - 1) == E_WORK
    assert call(d_out=out.data_ptr() + 8) == E_ARG and "16-byte" in L.trc_last_error().decode()
    assert call(codec=trc.RCA4) == E_ARG and "low four bits" in L.trc_last_error().decode()
    assert call(chunk=100) == E_ARG
    assert call(filters=trc.planes_filters([0, 3] + [0] * (bc.count - 2), bc.count)) == E_ARG and "item 1: filter 3" in L.trc_last_error().decode()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and int(d_size.item()) == 0x5A5A, "a rejected call wrote"
    # a total no encoder writes: *d_size = 0, and no fault
    bad_total = bc.total.clone()
    bad_total[:8] = torch.from_numpy(np.array([bc.plan["m_total"] + 1], dtype="<u8").view(np.uint8)).to("cuda:0")
    assert L.trc_planes_batch_pack_dev(bc.codec, bc.items, bc.filters, bc.count, 4, CHUNK, None, 0, None, bc.clen.data_ptr(), bc.payload.data_ptr(),
                                       bad_total.data_ptr(), out.data_ptr(), bound, d_size.data_ptr(), bc._stream()) == 0
    torch.cuda.synchronize()
    assert int(d_size.item()) == 0 and (out.cpu().numpy()[bound:] == 0xA5).all()


# ---- decode_packed_dev -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_decode_packed(torch_cuda, codec, esize):
    torch = torch_cuda
    for fname, oname in (("mixed", "odd"), ("none", "even"), ("zigzag", "odd"), ("mixed", "one")):
        p = packed(torch, codec, esize, fname, oname)
        bc, src = p["bc"], p["src"]
        total = trc.parse_planes_batch(p["cont"])["total"]
        d_cont = bc.packed                                      # the container with what is left of the bound behind it
        for fi, ic in item_ranges(bc.count, [(i, 2) for i in range(bc.count - 1)]):
            only = range(fi, fi + ic)
            dst = Packed(torch, src.datas, seed=esize, data=False)
            bc.range_work, bc.range_work_bytes = None, 0        # a workspace of exactly the required size, guarded, for every range
            bc.decode_packed(d_cont, total, fi, ic, out=dst.views(only), cont_bytes=p["size"])
            torch.cuda.synchronize()
            tag = p["tag"] + " items (%d, %d)" % (fi, ic)
            assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag
            assert bc.guards_ok(), tag
        assert np.array_equal(d_cont[:p["size"]].cpu().numpy(), p["want"]), p["tag"] + ": decode changed the container"


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_decode_packed_argument_errors(torch_cuda, codec):
    torch = torch_cuda
    p = packed(torch, codec, 2, "mixed", "odd")
    bc, src = p["bc"], p["src"]
    total = trc.parse_planes_batch(p["cont"])["total"]
    dst = Packed(torch, src.datas, seed=2, data=False)
    need = trc.lib().trc_planes_batch_range_work_bytes(codec, dst.items(), bc.count, 2, CHUNK, 0, bc.count)
    with pytest.raises(trc.TrcError, match="rc=%d" % E_WORK):
        bc.decode_packed(bc.packed, total, out=dst.views(), cont_bytes=p["size"], work_bytes=need - 1)
    with pytest.raises(trc.TrcError, match="rc=%d" % E_ARG):
        bc.decode_packed(bc.packed, total, out=dst.views(), cont_bytes=p["size"] - 1)
    with pytest.raises(trc.TrcError, match="payload bytes"):
        bc.decode_packed(bc.packed, [bc.plan["m_total"] + 1] * 2, out=dst.views(), cont_bytes=p["size"])
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(0))), "a rejected call wrote to an item, a gap or the guard"


# ---- the host-pointer calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_host_encode_both_ways(torch_cuda, codec, esize):
    torch = torch_cuda
    for fname, oname in (("mixed", "odd"), ("none", "even"), ("mixed", "nc1")):
        p = packed(torch, codec, esize, fname, oname)
        src = p["src"]
        got = trc.host_encode_planes_batch(codec, src.datas, esize, CHUNK, filters=p["filters"], prm=PRM)
        assert np.array_equal(got, p["want"]), p["tag"] + ": host items"
        got = trc.host_encode_planes_batch(codec, src.views(), esize, CHUNK, filters=p["filters"], prm=PRM)
        assert np.array_equal(got, p["want"]), p["tag"] + ": device items"
        assert np.array_equal(src.buf.cpu().numpy(), src.img)


@pytest.mark.parametrize("esize", ESIZES)
def test_host_encode_auto_is_the_explicit_call(torch_cuda, esize):
    torch = torch_cuda
    datas = gen_items(esize, LENGTHS + [4097, 3000, 2048], 90 + esize)
    src = Packed(torch, datas, seed=esize)
    chosen, _ = trc.planes_advise_batch_dev(src.items(), esize, CHUNK, 7, len(datas), "cuda:0")
    assert len(set(chosen)) > 1, "the advisor is meant to tell ids from noise here"
    want = trc.host_encode_planes_batch(trc.RCA, src.views(), esize, CHUNK, filters=chosen)
    for arrays in (src.views(), datas):
        got, filters = trc.host_encode_planes_batch(trc.RCA, arrays, esize, CHUNK, filters="auto")
        assert filters == chosen and np.array_equal(got, want)
    assert np.array_equal(want, expected_container(trc.RCA, datas, chosen, esize, CHUNK))
    assert trc.parse_planes_batch(want)["filters"] == chosen


@pytest.mark.parametrize("esize", ESIZES)
@pytest.mark.parametrize("codec", CODECS)
def test_host_decode_ranges(torch_cuda, codec, esize):
    torch = torch_cuda
    p = packed(torch, codec, esize, "mixed", "odd")
    src, count = p["src"], p["bc"].count
    for fi, ic in ((0, 1), (1, 2), (3, 1), (count - 1, 1), (2, 3), (0, count)):
        only = range(fi, fi + ic)
        got = trc.host_decode_planes_batch(p["want"], fi, ic)                        # to host arrays, NULL outside the range
        assert len(got) == ic and all(np.array_equal(g, src.datas[i]) for g, i in zip(got, only)), p["tag"] + " host items (%d, %d)" % (fi, ic)
        dst = Packed(torch, src.datas, seed=esize, data=False)
        assert trc.host_decode_planes_batch(p["want"], fi, ic, out=dst.views(only)) == sum(src.sizes[i] for i in only)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), p["tag"] + " device items (%d, %d)" % (fi, ic)
    sizes = list(src.sizes)
    sizes[count - 1] += esize                                   # an item outside the range that does not match is refused all the same
    with pytest.raises(trc.TrcError, match="item %d" % (count - 1)):
        trc.host_decode_planes_batch(p["want"], 0, 1, sizes=sizes)


def test_host_calls_at_chunk_4096_with_64_columns(torch_cuda, monkeypatch):
    """payloads of several 16 KiB tiles each: the pack kernel's search for a tile's region, also with three workgroups for all of them"""
    torch = torch_cuda
    rng = np.random.default_rng(4096)
    datas = [(np.cumsum(rng.integers(0, 50, 1024)).astype("<u4") if i % 2 else rng.standard_normal(1024).astype("<f4")).view(np.uint8).copy()
             for i in range(64)]
    filters = [i % 2 for i in range(64)]
    want = expected_container(trc.RCA, datas, filters, 4, 4096)
    got = trc.host_encode_planes_batch(trc.RCA, datas, 4, 4096, filters=filters)
    assert np.array_equal(got, want)
    src = Packed(torch, datas, seed=1)
    assert np.array_equal(trc.host_encode_planes_batch(trc.RCA, src.views(), 4, 4096, filters=filters), want)
    assert max(trc.parse_planes_batch(want)["total"]) > 3 * 16384
    monkeypatch.setenv("TRC_PLANES_GRID", "3")
    assert np.array_equal(trc.host_encode_planes_batch(trc.RCA, src.views(), 4, 4096, filters=filters), want)
    monkeypatch.delenv("TRC_PLANES_GRID")
    back = trc.host_decode_planes_batch(got, 17, 30)
    assert all(np.array_equal(b, datas[17 + i]) for i, b in enumerate(back))
    back = trc.host_decode_planes_batch(got)
    assert len(back) == 64 and all(np.array_equal(b, d) for b, d in zip(back, datas))


# ---- the harness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ("z", "a"))
def test_trcfile_batch(torch_cuda, tmp_path, letter):
    datas = gen_items(4, [1000, 299, 5000], 5)
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / ("item%d.bin" % i)))
        d.tofile(paths[-1])
    comp = str(tmp_path / "batch.trcb")
    r = trcfile("b", "46", "4", "256", letter, comp, *paths)
    cont = np.fromfile(comp, dtype=np.uint8)
    info = trc.parse_planes_batch(cont)
    assert info["n"] == [d.size for d in datas] and info["codec"] == trc.RCA and info["chunk"] == 256
    if letter == "z":
        assert np.array_equal(cont, expected_container(trc.RCA, datas, [FL.ZDELTA] * 3, 4, 256))
    else:
        assert [l.split("choice ")[1][0] for l in r.stdout.splitlines() if l.startswith("item ")] == ["nzx"[f] for f in info["filters"]]
        assert info["filters"][2] == FL.ZDELTA, "sorted ids are meant to take the zigzag delta"
    l = trcfile("l", comp)
    assert l.stdout.startswith("3 items, esize 4, chunk 256")
    assert [x.split(":")[0] for x in l.stdout.splitlines()[1:]] == ["item 0", "item 1", "item 2"]
    for first, cnt in ((0, 3), (1, 2), (2, 1)):
        out = str(tmp_path / "out.bin")
        trcfile("B", comp, first, cnt, out)
        assert np.array_equal(np.fromfile(out, dtype=np.uint8), np.concatenate(datas[first:first + cnt]))
