"""Byte planes against a base buffer on the MI355X.  The whole contract is bplanes(filter, ..., in, base) == planes(..., D(filter, esize,
in, base)) with D the numpy model of bplanes_lib, so every comparison is byte equality: the two kernels alone against the model at
the edges of a vector, a workgroup and the grid, in place, and with TRC_FILTER_NONE; the fingerprint against the host function and
the model; the coded calls against the unfiltered calls on the model-filtered input, whole, by chunk range and in place; the
advisor's histograms against a base; the TRCD container through host pointers and `trcfile r / R`.  Every kernel buffer has a
512-byte guard of 0xA5 on both sides that must survive, and the base is uploaded with NO slack behind it."""
import numpy as np
import pytest

import advise_lib as AL
import bplanes_lib as BP
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, GUARD, PRM, Guarded, decodes_flat, decodes_ranges_flat, first_diff, guarded, padded, trcfile, up256
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
M6 = 5 * CHUNK + 3                                              # 6 chunks per plane, the last one of 3 elements
SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 5)            # a thread's vector, one workgroup's 2048 elements, a ragged end
NAMES = {BP.ZDELTA: "z", BP.XOR: "x"}


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, filt, m, t, kind):
    """split against the base at the smallest pitch the call takes, join again.  Compared: the planes with the pitch gaps behind
    them, the tail, the guards on both sides of all five buffers, join(split(x)) == x, the unchanged input and base"""
    d, b = BP.gen_pair(kind, esize, m, t, 100 * m + 10 * esize + t)
    planes, tail = PL.split(BP.forward(d, b, esize, filt), esize)
    tag = "esize %d, filter %s, m %d, t %d, %s" % (esize, NAMES[filt], m, t, kind)
    n, pitch = d.size, up256(m)
    d_in, d_base, d_planes, d_tail, d_out = (Guarded(torch, n, d), Guarded(torch, m * esize, b), Guarded(torch, esize * pitch), Guarded(torch, 8),
                                             Guarded(torch, n))
    trc.planes_split_base(filt, d_in.t, d_base.t, n, esize, d_planes.t, pitch, d_tail.t if t else None)
    trc.planes_join_base(filt, d_planes.t, pitch, d_tail.t if t else None, d_base.t, n, esize, d_out.t)
    torch.cuda.synchronize()
    exp = np.full(esize * pitch, 0xA5, dtype=np.uint8)          # (the pitch gap behind m stays as it was)
    for k in range(esize):
        exp[k * pitch:k * pitch + m] = planes[k]
    got, intact = d_planes.get()
    assert np.array_equal(got, exp), tag + ": planes or the gaps behind them (first difference at %d)" % first_diff(got, exp)
    assert intact, tag + ": split wrote outside its planes"
    exp_tail = np.full(8, 0xA5, dtype=np.uint8)
    exp_tail[:t] = tail
    got, intact = d_tail.get()
    assert np.array_equal(got, exp_tail) and intact, tag + ": tail or the bytes around it"
    got, intact = d_out.get()
    assert np.array_equal(got, d), tag + ": join(split(x)) != x (first difference at byte %d)" % first_diff(got, d)
    assert intact, tag + ": join wrote outside its output"
    for buf, src, what in ((d_in, d, "input"), (d_base, b, "base")):
        got, intact = buf.get()
        assert np.array_equal(got, src) and intact, tag + ": the %s changed" % what


@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("esize", BP.ESIZES)
def test_split_join(torch_cuda, esize, filt):
    for i, m in enumerate(SIZES):
        for t in (0, esize - 1):
            split_join_case(torch_cuda, esize, filt, m, t, BP.KINDS[(i + (t > 0)) % 4])


@pytest.mark.parametrize("esize", BP.ESIZES)
def test_split_join_grid_capped(torch_cuda, esize, monkeypatch):
    """one workgroup: the loops of split and join turn 10 times"""
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    for filt, kind in ((BP.ZDELTA, "wrap"), (BP.XOR, "drift")):
        split_join_case(torch_cuda, esize, filt, 9 * 2048 + 5, esize - 1, kind)


@pytest.mark.parametrize("esize", BP.ESIZES)
def test_largest_input(torch_cuda, esize):
    split_join_case(torch_cuda, esize, BP.ZDELTA if esize != 4 else BP.XOR, 1 << 20, 0, "drift")


@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("esize", BP.ESIZES)
def test_join_in_place(torch_cuda, esize, filt):
    """out == base applies the delta to the resident base; out == base + 16 is refused and nothing is written"""
    torch = torch_cuda
    for m, t in ((3 * 2048 + 5, esize - 1), (7, 0), (40000, 0)):
        d, b = BP.gen_pair("drift", esize, m, t, m + esize)
        n, pitch = d.size, up256(m)
        planes, tail = PL.split(BP.forward(d, b, esize, filt), esize)
        img = np.full(esize * pitch, 0xA5, dtype=np.uint8)
        for k in range(esize):
            img[k * pitch:k * pitch + m] = planes[k]
        d_planes, d_tail = Guarded(torch, esize * pitch, img), Guarded(torch, 8, np.concatenate([tail, np.full(8 - t, 0xA5, np.uint8)]))
        d_base = Guarded(torch, n + 32, np.concatenate([b, np.full(t + 32, 0xA5, np.uint8)]))      # (room for the tail and the shifted output)
        if m * esize > 64:
            with pytest.raises(trc.TrcError, match="rc=-1"):
                trc.planes_join_base(filt, d_planes.t, pitch, d_tail.t, d_base.t, n, esize, d_base.t[16:])
            assert "overlaps the base" in trc.lib().trc_last_error().decode()
            with pytest.raises(trc.TrcError, match="rc=-1"):        # ... and a base that starts inside the output
                trc.planes_join_base(filt, d_planes.t, pitch, d_tail.t, d_base.t[16:], n - 16, esize, d_base.t)
        torch.cuda.synchronize()
        got, intact = d_base.get()
        assert np.array_equal(got[:m * esize], b) and (got[m * esize:] == 0xA5).all() and intact, "a refused join wrote"
        trc.planes_join_base(filt, d_planes.t, pitch, d_tail.t if t else None, d_base.t, n, esize, d_base.t)
        torch.cuda.synchronize()
        got, intact = d_base.get()
        assert np.array_equal(got[:n], d), "esize %d filter %s m %d: in place (first difference at byte %d)" % (esize, NAMES[filt], m, first_diff(got[:n], d))
        assert (got[n:] == 0xA5).all() and intact, "the in-place join wrote behind its n bytes"
        assert np.array_equal(d_planes.get()[0], img) and d_planes.get()[1]


def test_filter_none_is_the_unfiltered_kernel(torch_cuda):
    torch = torch_cuda
    esize, m, t = 4, 1000, 3
    n = m * esize + t
    d = BP.gen_pair("random", esize, m, t, 1)[0]
    planes, tail = PL.split(d, esize)
    d_in, d_planes, d_tail, d_out = guarded(torch, n, d), guarded(torch, esize * 1024), guarded(torch, 8), guarded(torch, n)
    trc.planes_split_base(trc.FILTER_NONE, d_in, None, n, esize, d_planes, 1024, d_tail)
    trc.planes_join_base(trc.FILTER_NONE, d_planes, 1024, d_tail, None, n, esize, d_out)
    torch.cuda.synchronize()
    got = d_planes.cpu().numpy()
    for k in range(esize):
        assert np.array_equal(got[k * 1024:k * 1024 + m], planes[k]) and (got[k * 1024 + m:(k + 1) * 1024] == 0xA5).all()
    assert np.array_equal(d_tail.cpu().numpy()[:t], tail)
    assert np.array_equal(d_out.cpu().numpy()[:n], d) and (d_out.cpu().numpy()[n:] == 0xA5).all()


def test_split_join_argument_errors(torch_cuda):
    torch = torch_cuda
    d_in, d_base, d_planes, d_tail = guarded(torch, 4096), guarded(torch, 4096), guarded(torch, 8 * 1024), guarded(torch, 8)
    bad = [(f, 4096, 2, 2048, None) for f in (-1, 3)]                                     # the filter
    bad += [(1, 4096, 3, 2048, None), (2, 1, 2, 256, d_tail), (1, 3, 4, 256, d_tail)]     # esize 3, no whole element
    bad += [(1, 4096, 2, 2000, None), (1, 4096, 2, 1792, None), (2, 4097, 2, 2048, None)]  # pitch, a tail without a buffer
    for filt, n, esize, pitch, tail in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_base(filt, d_in, d_base, n, esize, d_planes, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_base(filt, d_planes, pitch, tail, d_base, n, esize, d_in)
    for filt in BP.FILTERS:
        for src, base in ((d_in[8:], d_base), (d_in, d_base[8:]), (d_in, None)):          # an input / a base off 16 bytes, no base
            with pytest.raises(trc.TrcError, match="rc=-1"):
                trc.planes_split_base(filt, src, base, 1024, 2, d_planes, 1024, None)
            with pytest.raises(trc.TrcError, match="rc=-1"):
                trc.planes_join_base(filt, d_planes, 1024, None, base, 1024, 2, src)
    torch.cuda.synchronize()
    for x in (d_in, d_base, d_planes, d_tail):
        assert (x.cpu().numpy() == 0xA5).all(), "a rejected call wrote"


# ---- the fingerprint -------------------------------------------------------------------------------------------------------
def fingerprint_case(torch, nbytes, seed):
    a = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    d = Guarded(torch, nbytes, a)                               # no slack: the guard starts at the last byte's neighbour
    d_fp = Guarded(torch, 8, fill=0x77)                         # a dirty word: the call overwrites it
    trc.base_fingerprint_enqueue(d.t, nbytes, d_fp.t)
    torch.cuda.synchronize()
    got, intact = d_fp.get()
    exp = BP.fingerprint(a)
    assert int(got.view("<u8")[0]) == exp == trc.base_fingerprint_host(a) and intact, "nbytes %d: device %016x, model %016x" % (nbytes, int(got.view("<u8")[0]), exp)
    assert trc.base_fingerprint(d.t[:nbytes]) == exp
    assert np.array_equal(d.get()[0], a) and d.get()[1]


def test_fingerprint(torch_cuda, monkeypatch):
    for i, nbytes in enumerate((1, 7, 8, 9, 15, 16, 17, 2047, 4096 * 16, 65536 + 3)):
        fingerprint_case(torch_cuda, nbytes, i)
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    fingerprint_case(torch_cuda, 1 << 20, 99)
    fingerprint_case(torch_cuda, (1 << 20) + 13, 98)
    d = guarded(torch_cuda, 64)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.base_fingerprint(d[8:], 16)


# ---- the coded calls ---------------------------------------------------------------------------------------------------
_cache = {}


def coded(torch, codec, esize, filt, chunk=CHUNK, m=M6, kind="drift"):
    """-> (input bytes, base bytes, the base on the device without slack, BasePlanesCoder holding the container, PlanesCoder holding
    the container of the model-filtered input): computed once per key, shared, left unchanged"""
    key = (codec, esize, filt, chunk, m, kind)
    if key not in _cache:
        d, b = BP.gen_pair(kind, esize, m, esize - 1, 17 * esize + filt)
        n = d.size
        d_base = Guarded(torch, m * esize, b)
        bc = trc.BasePlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, filter=filt)
        pc = trc.PlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD)
        d_in = padded(torch, d)
        img = d_in.cpu().numpy()
        for c in (bc, pc):
            c.payload[:esize * c.pitch] = 0x5A
        bc.encode(d_in, d_base.t, n)
        pc.encode(padded(torch, BP.forward(d, b, esize, filt)), n)
        assert bc.guards_ok() and pc.guards_ok(), "encode wrote behind one of its buffers"
        assert np.array_equal(d_in.cpu().numpy(), img), "encode changed its input, the pad or the guard behind it"
        got, intact = d_base.get()
        assert np.array_equal(got, b) and intact, "encode changed the base or the bytes around it"
        _cache[key] = (d, b, d_base, bc, pc)
    return _cache[key]


class WithBase:
    """a BasePlanesCoder with its base bound, so that the decode checks of gpu_planes serve unchanged"""

    def __init__(self, bc, d_base):
        self.bc, self.d_base = bc, d_base

    def decode(self, d_out, n=None, flags=0):
        self.bc.decode(d_out, self.d_base, n, flags)

    def decode_range(self, d_out, first, count, n=None, flags=0):
        self.bc.decode_range(d_out, self.d_base, first, count, n, flags)

    def guards_ok(self):
        return self.bc.guards_ok()


@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract_and_every_range(torch_cuda, codec, filt):
    torch = torch_cuda
    esize = 4
    d, b, d_base, bc, pc = coded(torch, codec, esize, filt)
    tag = "%s filter %s" % (trc.CODEC_NAMES[codec], NAMES[filt])
    assert bc.nch == 6
    assert_same_container(bc, pc, esize, codec, tag)
    wb = WithBase(bc, d_base.t)
    decodes_flat(torch, wb, d, tag)
    decodes_ranges_flat(torch, wb, d, esize, CHUNK, [(first, count) for first in range(6) for count in range(1, 6 - first + 1)], tag)
    got, intact = d_base.get()
    assert np.array_equal(got, b) and intact, tag + ": a decode changed the base"


@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("esize,codec", [(2, trc.RCA), (8, trc.ANS4S)])
def test_encode_contract_other_widths(torch_cuda, esize, codec, filt):
    torch = torch_cuda
    chunk, m = 4096, 2 * 4096 + 77
    d, b, d_base, bc, pc = coded(torch, codec, esize, filt, chunk, m)
    tag = "%s esize %d filter %s" % (trc.CODEC_NAMES[codec], esize, NAMES[filt])
    assert_same_container(bc, pc, esize, codec, tag)
    wb = WithBase(bc, d_base.t)
    decodes_flat(torch, wb, d, tag)
    decodes_ranges_flat(torch, wb, d, esize, chunk, [(1, 2)], tag)


@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_decode_in_place(torch_cuda, codec, filt):
    """the whole decode and a chunk range onto the base they read; any other overlap is refused before anything is enqueued"""
    torch = torch_cuda
    esize = 4
    d, b, _, bc, _ = coded(torch, codec, esize, filt)
    n, m = d.size, d.size // esize
    room = np.concatenate([b, np.full(n - m * esize + trc.PAD, 0xA5, np.uint8)])
    d_base = Guarded(torch, room.size, room)
    for shifted in (d_base.t[16:], d_base.t[m * esize // 16 * 16 - 16:]):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            bc.decode(shifted, d_base.t, n)
        assert "overlaps the base" in trc.lib().trc_last_error().decode()
    with pytest.raises(trc.TrcError, match="rc=-1"):                # a range in place starts at ITS elements of the base
        bc.decode_range(d_base.t, d_base.t, 1, 2, n)
    torch.cuda.synchronize()
    assert np.array_equal(d_base.get()[0], room) and d_base.get()[1], "a refused decode wrote"
    first, count = 2, 3
    off, size = first * CHUNK * esize, count * CHUNK * esize
    bc.decode_range(d_base.t[off:], d_base.t, first, count, n)
    torch.cuda.synchronize()
    got, intact = d_base.get()
    exp = room.copy()
    exp[off:off + size] = d[off:off + size]
    assert np.array_equal(got, exp) and intact, "the range in place: chunks [2, 5) become the input's, everything else stays the base"
    d_base = Guarded(torch, room.size, room)
    bc.decode(d_base.t, d_base.t, n)
    torch.cuda.synchronize()
    got, intact = d_base.get()
    assert np.array_equal(got[:n], d) and (got[n:] == 0xA5).all() and intact, "the whole decode in place"
    assert bc.guards_ok()


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_filter_none_is_the_unfiltered_call(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d = BP.gen_pair("drift", esize, M6, esize - 1, 3)[0]
    n = d.size
    bc = trc.BasePlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    assert bc.filter == trc.FILTER_NONE
    pc = trc.PlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    d_in = padded(torch, d)
    for c in (bc, pc):
        c.payload[:esize * c.pitch] = 0x5A
    bc.encode(d_in, None, n)
    pc.encode(d_in, n)
    assert_same_container(bc, pc, esize, codec, trc.CODEC_NAMES[codec] + " filter none")
    for name in ("clen", "total", "tail", "cdf", "status"):
        assert torch.equal(getattr(bc, name), getattr(pc, name)), name
    wb = WithBase(bc, None)
    decodes_flat(torch, wb, d, "filter none")
    decodes_ranges_flat(torch, wb, d, esize, CHUNK, [(2, 2)], "filter none")


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d, b, d_base, bc, _ = coded(torch, codec, esize, BP.ZDELTA)
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    d_in = padded(torch, d)
    names = ("clen", "payload", "total", "tail", "cdf", "work")
    before = [getattr(bc, x).clone() for x in names]

    def rejected(base=d_base.t, nbytes=n, flags=0, **attrs):
        saved = {k: getattr(bc, k) for k in attrs}
        for k, v in attrs.items():
            setattr(bc, k, v)
        try:
            with pytest.raises(trc.TrcError, match="rc=-1"):
                bc.encode(d_in, base, nbytes, flags=flags)
            with pytest.raises(trc.TrcError, match="rc=-1"):
                bc.decode(d_out, base, nbytes, flags=flags)
            with pytest.raises(trc.TrcError, match="rc=-1"):
                bc.decode_range(d_out, base, 0, 1, nbytes, flags=flags)
        finally:
            for k, v in saved.items():
                setattr(bc, k, v)

    for filt in (-1, 3):
        rejected(filter=filt)
        assert "filter %d" % filt in trc.lib().trc_last_error().decode()
    rejected(base=None)
    rejected(base=d_base.t[8:])
    for chunk in (100, 128, 65600):
        rejected(chunk=chunk)
    for flag in (trc.TABLES_READY, trc.DIR_READY):
        rejected(flags=flag)
    rejected(esize=3)
    rejected(nbytes=esize - 1)                                  # m == 0
    for first, count in ((6, 1), (0, 7), (3, 4)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            bc.decode_range(d_out, d_base.t, first, count, n)
    bc.decode_range(d_out, d_base.t, 2, 0, n)                   # count 0: TRC_OK, nothing launched
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its output"
    for x, bef in zip(names, before):
        assert torch.equal(getattr(bc, x), bef), "a rejected call changed the container or the workspace"
    assert bc.guards_ok()


# ---- the advisor's histograms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", BP.ESIZES)
def test_hist_base(torch_cuda, esize, monkeypatch):
    torch = torch_cuda
    hb = trc.planes_hist_bytes(esize)
    for i, (m, filters) in enumerate(((9, 7), (3 * 2048 + 5, 7), (2049, 2), (4100, 4), (2048, 6), (777, 5), (100, 1))):
        kind = BP.KINDS[i % 4]
        d, b = BP.gen_pair(kind, esize, m, esize - 1, m + filters)
        d_in, d_base, d_hist = Guarded(torch, d.size, d), Guarded(torch, m * esize, b), Guarded(torch, hb, fill=0x33)
        trc.planes_hist_base(filters, d_in.t, d_base.t if filters != 1 else None, d.size, esize, d_hist.t)
        torch.cuda.synchronize()
        got, intact = d_hist.get()
        got = got.view("<u8").reshape(3, esize, 256)
        exp = BP.hist(d, b, esize, filters)
        assert np.array_equal(got, exp) and intact, "esize %d m %d filters %d %s" % (esize, m, filters, kind)
        for buf, src in ((d_in, d), (d_base, b)):
            assert np.array_equal(buf.get()[0], src) and buf.get()[1]
    # more than one turn of a workgroup's loop and more than one flush
    monkeypatch.setenv("TRC_PLANES_GRID", "2")
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "2")
    m = 9 * 2048 + 5
    d, b = BP.gen_pair("drift", esize, m, 0, 5)
    d_in, d_base, d_hist = Guarded(torch, d.size, d), Guarded(torch, m * esize, b), Guarded(torch, hb, fill=0x33)
    trc.planes_hist_base(7, d_in.t, d_base.t, d.size, esize, d_hist.t)
    torch.cuda.synchronize()
    got, intact = d_hist.get()
    assert np.array_equal(got.view("<u8").reshape(3, esize, 256), BP.hist(d, b, esize, 7)) and intact
    a = trc.planes_advise(got.view("<u8"), 7, esize, m)
    assert a["filter"] == AL.advise(BP.hist(d, b, esize, 7), 7, esize, m)[0] != BP.NONE
    for filters, base in ((0, d_base.t), (8, d_base.t), (7, None), (2, d_base.t[8:])):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_hist_base(filters, d_in.t, base, d.size, esize, d_hist.t)


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (256, 0))
@pytest.mark.parametrize("filt", BP.FILTERS)
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S))
def test_host_container(torch_cuda, codec, filt, chunk):
    esize, m = 4, 9 * 256 + 3
    d, b = BP.gen_pair("drift", esize, m, esize - 1, 23)
    n, t = d.size, esize - 1
    tag = "%s TRCD filter %s chunk %d" % (trc.CODEC_NAMES[codec], NAMES[filt], chunk)
    base = np.concatenate([b, np.full(5, 0xEE, np.uint8)])         # a base longer than the elements: the rest is not looked at
    comp = trc.host_encode_bplanes(codec, filt, d, base, esize, chunk)
    trc.bplanes_check(comp, n)
    assert comp[:4].tobytes() == b"TRCD" and tuple(comp[4:8]) == (filt, 1, 0, 0), tag + ": prefix"
    size, base_bytes, fp = (int(x) for x in comp[8:32].view("<u8"))
    assert (size, base_bytes, fp) == (comp.size, m * esize, BP.fingerprint(b)), tag + ": size, base_bytes, base_fp"
    hdr, _, tail = trc.parse_planes(comp[32:])
    assert hdr["chunk"] == (chunk or trc.lib().trc_auto_chunk_codec(codec, m)) and hdr["n"] == n, tag
    assert np.array_equal(comp[32:], trc.host_encode_planes(codec, BP.forward(d, b, esize, filt), esize, chunk)), tag + ": bytes [32:]"
    assert np.array_equal(tail, d[n - t:])
    assert np.array_equal(trc.host_decode_bplanes(comp, base, n), d), tag + ": the whole decode"
    assert np.array_equal(trc.host_decode_bplanes(comp, b, n), d), tag + ": the whole decode from a base of exactly base_bytes"
    c = hdr["chunk"] * esize
    for offset, length in [(0, 1), (c - 1, 3), (c // 2, 2 * c), (5, n - 5), (n - t - 1, t + 1), (n - t, t), (n - 1, 1), (0, n)]:
        if offset + length <= n:
            assert np.array_equal(trc.host_decode_bplanes_range(comp, base, offset, length), d[offset:offset + length]), tag + ": bytes [%d, +%d)" % (offset, length)
    with pytest.raises(trc.TrcError):
        trc.host_decode_bplanes_range(comp, base, n - 1, 2)
    with pytest.raises(trc.TrcError, match="container"):
        trc.host_decode_bplanes(comp[:-1], base, n)
    # another base: refused by its fingerprint before anything is decoded, both values named; the range decoder does not look
    other = base.copy()
    other[1025] ^= 0x10
    with pytest.raises(trc.TrcError, match="base fingerprint") as e:
        trc.host_decode_bplanes(comp, other, n)
    assert "%016x" % fp in str(e.value) and "%016x" % BP.fingerprint(other[:m * esize]) in str(e.value)
    assert np.array_equal(trc.host_decode_bplanes_range(comp, other, 0, 16), d[:16])
    with pytest.raises(trc.TrcError, match="the base holds"):
        trc.host_decode_bplanes(comp, b[:-1], n)
    with pytest.raises(trc.TrcError, match="filter 0"):
        trc.host_encode_bplanes(codec, trc.FILTER_NONE, d, base, esize, chunk)
    with pytest.raises(trc.TrcError, match="trc_decode_bplanes_host"):
        trc.host_decode_xplanes(comp, n)


def test_fine_tune_stores_fewer_bytes_against_its_base(torch_cuda):
    """2^20 bf16 weights against the same weights plus N(0, (1e-4)^2) noise through rccdf at the automatic chunk: the order-0 model
    says 0.339 of the size against the base and 0.67 as plain planes"""
    base, data = BP.pair(1 << 20, 2, 7, 1e-4)
    plain = trc.host_encode_planes(trc.RCA, data, 2, 0)
    delta = trc.host_encode_bplanes(trc.RCA, trc.FILTER_ZDELTA, data, base, 2, 0)
    xored = trc.host_encode_bplanes(trc.RCA, trc.FILTER_XOR, data, base, 2, 0)
    print("bf16 fine-tune, %d bytes: planes %d, zigzag delta against the base %d, xor against the base %d" % (data.size, plain.size, delta.size, xored.size))
    assert delta.size <= 0.6 * plain.size and xored.size < plain.size       # (the model's ratio of the two is 0.51)
    assert np.array_equal(trc.host_decode_bplanes(delta, base, data.size), data)


def test_trcfile_bplanes(torch_cuda, tmp_path):
    d, b = BP.gen_pair("drift", 4, 40000, 3, 9)
    src, base, comp, back = (str(tmp_path / f) for f in ("in.bin", "base.bin", "in.trcd", "out.bin"))
    d.tofile(src)
    b.tofile(base)
    for letter, filt in (("z", 1), ("x", 2)):
        trcfile("r", "46", "4", letter, base, src, comp)
        head = np.fromfile(comp, dtype=np.uint8)
        assert head[:4].tobytes() == b"TRCD" and head[4] == filt and head[32:36].tobytes() == b"TRCP"
        trcfile("R", comp, base, back)
        assert np.array_equal(np.fromfile(back, dtype=np.uint8), d)
        assert "trcfile R" in trcfile("d", comp, back, rc=2).stderr
        assert "trcfile R" in trcfile("x", comp, 0, 16, back, rc=2).stderr
        assert "base fingerprint" in trcfile("R", comp, src, back, rc=1).stderr       # the wrong base
    assert "filter" in trcfile("r", "46", "4", "q", base, src, comp, rc=2).stderr
