"""Byte planes behind a predictor of order 2 or 3 on the MI355X.  The whole contract is oplanes(K, S, ..., in) == planes(..., O(K, S,
chunk, esize, in)) with O the numpy model of oplanes_lib, so every comparison is byte equality: the two kernels alone against the
model where the reach of ORDER * S elements crosses one, two and three vectors, a tile, a restart segment, a span and the grid;
orders 0 and 1 against the existing calls; the coded calls against the unfiltered calls on the model-filtered input; chunk ranges;
the histograms of trc_planes_hist_order_dev against numpy bincounts; the TRCO container and the order advisor through host
pointers and `trcfile o / O / d / x`; and what it is for: a smooth series stores fewer bytes at order 2, an integer column more.
The kernel tests put 512 guard bytes of 0xA5 on both sides of every device buffer.  The buffers and the check layers shared with
the other plane files are in gpu_planes.py."""
import numpy as np
import pytest

import fplanes_lib as FL
import oplanes_lib as OL
import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import (GUARD, Guarded, assert_order_hists, coded_flat, decodes_flat, decodes_ranges_flat, device_order_hists, first_diff,
                        host_container_filtered, padded, trcfile, trcfile_round_trip, up256)
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu

# (seg, m): a span of 8 segments per wave with a partial last vector; below a tile, no power of two, S does not divide it; one tile
# per segment; eight tiles per segment, so that every level's carry crosses tiles; fewer elements than ORDER * S, than two vectors
SHAPES = ((256, 2049 + 5), (320, 3 * 320 + 9), (512, 1024 + 1), (4096, 9 * 4096 + 5), (256, 5), (256, 9))


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_order(torch, d, esize, order, stride, seg, m, t, tag):
    """split d at the smallest pitch the call takes, join the planes again (split_join_flat of gpu_planes.py for the order calls).
    Compared with the model: the planes with the pitch gaps behind them (bytes of a plane past m are unwritten), the tail, the guards
    on both sides of all four buffers, join(split(x)) == x, the unchanged input"""
    n = d.size
    assert n == m * esize + t, tag
    planes, tail = PL.split(OL.forward(d, esize, order, seg, stride), esize)
    pitch = up256(m)
    d_in, d_planes, d_tail, d_out = Guarded(torch, n, d), Guarded(torch, esize * pitch), Guarded(torch, 8), Guarded(torch, n)
    trc.planes_split_ofilter(order, stride, d_in.t, n, esize, seg, d_planes.t, pitch, d_tail.t if t else None)
    trc.planes_join_ofilter(order, stride, d_planes.t, pitch, d_tail.t if t else None, n, esize, seg, d_out.t)
    torch.cuda.synchronize()
    exp = np.full(esize * pitch, 0xA5, dtype=np.uint8)
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
    got, intact = d_in.get()
    assert np.array_equal(got, d) and intact, tag + ": the input changed"


def split_join_case(torch, esize, order, stride, seg, m, kind):
    t = esize - 1
    d = OL.gen(kind, esize, m, t, 100 * m + 10 * esize + order + stride, stride)
    split_join_order(torch, d, esize, order, stride, seg, m, t, "esize %d, order %d, stride %d, seg %d, m %d, %s" % (esize, order, stride, seg, m, kind))


@pytest.mark.parametrize("stride", OL.ALL_STRIDES)
@pytest.mark.parametrize("order", OL.ORDERS)
@pytest.mark.parametrize("esize", OL.ESIZES)
def test_split_join(torch_cuda, esize, order, stride):
    """every (esize, order, stride) entry of the split and join tables: among them the join's rotating even stride 6 and, at 16 bits,
    the half-filled last pair of stride 7"""
    for seg, m in SHAPES:
        for kind in ("random", "smooth"):
            split_join_case(torch_cuda, esize, order, stride, seg, m, kind)
    for seg, m in ((256, 2049 + 5), (4096, 9 * 4096 + 5)):      # every byte 0xff: the sums wrap at every level
        split_join_case(torch_cuda, esize, order, stride, seg, m, "ones")
    split_join_case(torch_cuda, esize, order, stride, 320, 3 * 320 + 9, "wrap")


@pytest.mark.parametrize("esize", OL.ESIZES)
def test_split_join_grid_capped(torch_cuda, esize, monkeypatch):
    """one workgroup = 4 waves: the split's loop turns 9 and 19 times; the join's waves take 2 or 3 of the 9 spans of 8 segments of
    256 (4 tiles each), 3 or 4 of the 13 spans of 5 segments of 320, and 2 or 3 of the 10 segments of 4096 (8 tiles each), the
    prefetch crossing from one span into the next"""
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    for order, strides in ((2, (3, 8)), (3, (1, 5))):
        for stride in strides:
            split_join_case(torch_cuda, esize, order, stride, 256, 64 * 256 + 8, "wrap")
            split_join_case(torch_cuda, esize, order, stride, 320, 100 * 320 + 5, "smooth")
            split_join_case(torch_cuda, esize, order, stride, 4096, 9 * 4096 + 5, "random")


def test_orders_zero_and_one_are_the_existing_kernels(torch_cuda):
    torch = torch_cuda
    for esize in OL.ESIZES:
        m, t, seg = 3 * 256 + 5, esize - 1, 256
        n, pitch = m * esize + t, up256(m)
        d = FL.gen("random", esize, m, t, esize)
        for order, stride in ((0, 1), (0, 5), (1, 1), (1, 3), (1, 8)):
            bufs = []
            for ordered in (True, False):
                d_in, d_planes, d_tail, d_out = Guarded(torch, n, d), Guarded(torch, esize * pitch), Guarded(torch, 8), Guarded(torch, n)
                if ordered:
                    trc.planes_split_ofilter(order, stride, d_in.t, n, esize, seg, d_planes.t, pitch, d_tail.t)
                    trc.planes_join_ofilter(order, stride, d_planes.t, pitch, d_tail.t, n, esize, seg, d_out.t)
                elif order == 0:
                    trc.planes_split(d_in.t, n, esize, d_planes.t, pitch, d_tail.t)
                    trc.planes_join(d_planes.t, pitch, d_tail.t, n, esize, d_out.t)
                else:
                    trc.planes_split_sfilter(FL.ZDELTA, stride, d_in.t, n, esize, seg, d_planes.t, pitch, d_tail.t)
                    trc.planes_join_sfilter(FL.ZDELTA, stride, d_planes.t, pitch, d_tail.t, n, esize, seg, d_out.t)
                torch.cuda.synchronize()
                bufs.append([b.whole.cpu().numpy() for b in (d_planes, d_tail, d_out)])
            for a, b, what in zip(bufs[0], bufs[1], ("planes", "tail", "output")):
                assert np.array_equal(a, b), (esize, order, stride, what)
            assert np.array_equal(bufs[0][2][GUARD:GUARD + n], d)


def test_split_join_argument_errors_launch_nothing(torch_cuda):
    torch = torch_cuda
    d_in, d_planes, d_tail = Guarded(torch, 4096), Guarded(torch, 8 * 1024), Guarded(torch, 8)
    bad = [(k, s, 4096, 2, 256, 2048, None) for k in (-1, 4) for s in (1, 0, 9)]                          # the order
    bad += [(k, s, 4096, 2, 256, 2048, None) for k in (0, 1, 2, 3) for s in (0, 9, -1)]                   # the stride
    bad += [(k, 3, 4096, 2, seg, 2048, None) for k in (2, 3) for seg in (100, 128, 65600, 0)]             # the restart length
    bad += [(2, 2, 4096, 3, 256, 2048, None), (3, 8, 1, 2, 256, 256, d_tail.t), (2, 4, 3, 4, 256, 256, d_tail.t)]      # esize 3, no whole element
    bad += [(2, 5, 4096, 2, 256, 2000, None), (3, 6, 4096, 2, 256, 1792, None), (2, 7, 4097, 2, 256, 2048, None)]      # pitch, a tail without a buffer
    for order, stride, n, esize, seg, pitch, tail in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_ofilter(order, stride, d_in.t, n, esize, seg, d_planes.t, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_ofilter(order, stride, d_planes.t, pitch, tail, n, esize, seg, d_in.t)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_split_ofilter(2, 3, d_in.t[8:], 1024, 2, 256, d_planes.t, 1024, None)               # an input that is not 16-byte aligned
    d_hist = Guarded(torch, trc.planes_hist_order_bytes(4))
    for orders, stride, esize, seg in ((15, 0, 4, 256), (15, 9, 4, 256), (0, 3, 4, 256), (16, 3, 4, 256), (12, 3, 3, 256), (12, 3, 4, 100)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_hist_order(orders, stride, d_in.t, 4096, esize, seg, d_hist.t)
    torch.cuda.synchronize()
    for b in (d_in, d_planes, d_tail, d_hist):
        assert (b.whole.cpu().numpy() == 0xA5).all(), "a rejected call wrote something"


# ---- the histograms -----------------------------------------------------------------------------------------------------
def hist_case(torch, esize, stride, seg, m, orders, kind="smooth"):
    tag = "esize %d, stride %d, seg %d, m %d, orders %d, %s" % (esize, stride, seg, m, orders, kind)
    d = OL.gen(kind, esize, m, esize - 1, 31 * m + esize, stride)
    got = device_order_hists(torch, d, esize, stride, seg, orders).reshape(4, esize, 256)
    assert_order_hists(got, OL.hist4(d, esize, seg, stride, orders).reshape(4, esize, 256), m, orders, tag)
    return d, got


@pytest.mark.parametrize("orders", (15, 4, 9))
@pytest.mark.parametrize("esize,stride", [(2, 3), (4, 4), (8, 7)])
def test_hist_order(torch_cuda, esize, stride, orders, monkeypatch):
    torch = torch_cuda
    for m in (1, stride, 7, 8, 9, 3 * stride + 1, 255, 257, 3 * 256 + 5, 40 * 256 + 3):
        hist_case(torch, esize, stride, 256, m, orders)
    hist_case(torch, esize, stride, 4096, 2 * 4096 + 77, orders, "random")
    hist_case(torch, esize, stride, 320, 3 * 320 + 5, orders, "wrap")
    d, got = hist_case(torch, esize, stride, 320, 3 * 320 + 5, orders, "ones")
    if orders == 15:                                            # rows 0 and 1 are those of trc_planes_hist_stride_dev
        n = d.size
        d_in, d_hist = Guarded(torch, n, d), Guarded(torch, trc.planes_hist_bytes(esize))
        trc.planes_hist_stride(3, stride, d_in.t, n, esize, 320, d_hist.t)
        torch.cuda.synchronize()
        assert np.array_equal(d_hist.get()[0].view("<u8").reshape(3, esize, 256)[:2], got[:2])
    # one workgroup whose loop turns 11 times, flushing its counters every second turn
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    hist_case(torch, esize, stride, 256, 10 * 2048 + 13, orders)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "2")
    hist_case(torch, esize, stride, 256, 10 * 2048 + 13, orders)
    hist_case(torch, esize, stride, 4096, 10 * 2048 + 13, orders, "random")


@pytest.mark.parametrize("esize", OL.ESIZES)
def test_hist_order_every_stride_and_order_set(torch_cuda, esize):
    """every (esize, stride) entry of the histogram table under every order set 1 .. 15 (the reach the kernel loads follows the
    highest order requested): a span of 8 segments with a partial last vector, and fewer elements than the reach.  The model's four
    rows are computed once per input; a set that leaves an order out must leave that order's rows zero"""
    for stride in OL.ALL_STRIDES:
        for seg, m in ((256, 2049 + 5), (256, 9)):
            d = OL.gen("smooth", esize, m, esize - 1, 31 * m + esize, stride)
            full = OL.hist4(d, esize, seg, stride).reshape(4, esize, 256)
            for orders in range(1, 16):
                exp = full.copy()
                exp[[k for k in range(4) if not orders >> k & 1]] = 0
                got = device_order_hists(torch_cuda, d, esize, stride, seg, orders).reshape(4, esize, 256)
                assert_order_hists(got, exp, m, orders, "esize %d, stride %d, seg %d, m %d, orders %d" % (esize, stride, seg, m, orders))


# ---- the coded calls ---------------------------------------------------------------------------------------------------
def coded(torch, codec, esize, order, stride, chunk, m):
    """-> (input bytes, OrderPlanesCoder holding their container, PlanesCoder holding the container of the model-filtered input):
    computed once per key, shared, left unchanged"""
    d = OL.gen("smooth", esize, m, esize - 1, 17 * esize + order + stride, stride)
    return (d,) + coded_flat(torch, codec, esize, chunk, d, trc.OrderPlanesCoder, lambda: OL.forward(d, esize, order, chunk, stride),
                             order=order, stride=stride)


CODED = [(4, c, chunk) for c in (trc.ANS4S, trc.RCA, trc.RCB) for chunk in (256, 4096)] + [(2, trc.RCA, 256), (8, trc.ANS4S, 256)]


@pytest.mark.parametrize("order,stride", [(2, 1), (3, 2), (2, 8), (3, 3)])
@pytest.mark.parametrize("esize,codec,chunk", CODED, ids=["%d-%s-%d" % (e, trc.CODEC_NAMES[c], ch) for e, c, ch in CODED])
def test_encode_contract_decode_and_ranges(torch_cuda, esize, codec, chunk, order, stride):
    torch = torch_cuda
    m = 5 * chunk + 3 if chunk == 256 else 2 * chunk + 77
    d, oc, pc = coded(torch, codec, esize, order, stride, chunk, m)
    tag = "%s esize %d chunk %d order %d stride %d" % (trc.CODEC_NAMES[codec], esize, chunk, order, stride)
    nch = oc.nch
    assert nch == (m + chunk - 1) // chunk
    assert_same_container(oc, pc, esize, codec, tag)
    assert torch.equal(oc.total, pc.total) and torch.equal(oc.clen, pc.clen), tag + ": totals or directory"
    decodes_flat(torch, oc, d, tag)
    decodes_ranges_flat(torch, oc, d, esize, chunk, ((0, 1), (1, 1), (nch - 1, 1), (1, nch - 1)), tag)


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_orders_zero_and_one_are_the_existing_calls(torch_cuda, codec):
    torch = torch_cuda
    esize, chunk, m = 4, 256, 5 * 256 + 3
    d = FL.gen("monotone", esize, m, esize - 1, 3)
    n = d.size
    d_in = padded(torch, d)
    for order, stride in ((0, 1), (0, 6), (1, 1), (1, 3)):
        oc = trc.OrderPlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, guard=GUARD, order=order, stride=stride)
        sc = trc.StridedPlanesCoder(codec, n, esize, chunk, "cuda:0", cdfnum=256, guard=GUARD, filter=FL.ZDELTA if order else FL.NONE, stride=stride)
        for c in (oc, sc):
            c.payload[:esize * c.pitch] = 0x5A
            c.encode(d_in, n)
        tag = "%s order %d stride %d" % (trc.CODEC_NAMES[codec], order, stride)
        assert_same_container(oc, sc, esize, codec, tag)
        for name in ("clen", "total", "tail", "cdf", "status"):
            assert torch.equal(getattr(oc, name), getattr(sc, name)), tag + ": " + name
        decodes_flat(torch, oc, d, tag)
        decodes_ranges_flat(torch, oc, d, esize, chunk, [(2, 2)], tag)


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (256, 0))
@pytest.mark.parametrize("order,stride", [(2, 1), (3, 2), (2, 7)])
def test_host_container(torch_cuda, order, stride, chunk):
    codec, esize, m = trc.RCA, 4, 9 * 256 + 3
    d = OL.gen("smooth", esize, m, esize - 1, 23, stride)
    n = d.size
    comp, _ = host_container_filtered(codec, d, esize, m, chunk, b"TRCO", (order, 1, stride, 0),
                                      lambda x, ch: trc.host_encode_oplanes(codec, order, stride, x, esize, ch), trc.oplanes_check,
                                      trc.host_decode_oplanes, trc.host_decode_oplanes_range, lambda seg: OL.forward(d, esize, order, seg, stride),
                                      more_ranges=lambda c: [(c + 5, 3 * c + 1)])
    assert np.array_equal(trc.host_decode_xplanes(comp, n), d)
    with pytest.raises(trc.TrcError, match="magic"):
        trc.host_decode_splanes(comp, n)                        # a TRCO container is not a TRCS container
    with pytest.raises(trc.TrcError, match="trc_encode_splanes_host" if stride > 1 else "trc_encode_fplanes_host"):
        trc.host_encode_oplanes(codec, 1, stride, d, esize, chunk)


@pytest.fixture(scope="module")
def table():
    """the inputs of the advisor and savings tests, 64 Ki elements each: name -> (esize, stride, bytes)"""
    t = {name: (esize, stride, d) for name, esize, stride, d in OL.table_inputs(1 << 16)}
    t["uniform bytes"] = (4, 1, np.random.default_rng(9).integers(0, 256, 4 << 16, dtype=np.uint8))
    return t


def explicit(codec, order, stride, d, esize):
    """what the explicit host call writes for that order at the automatic chunk"""
    if order == 0:
        return trc.host_encode_planes(codec, d, esize, 0)
    if order == 1:
        return trc.host_encode_fplanes(codec, trc.FILTER_ZDELTA, d, esize, 0) if stride == 1 else trc.host_encode_splanes(codec, trc.FILTER_ZDELTA, stride, d, esize, 0)
    return trc.host_encode_oplanes(codec, order, stride, d, esize, 0)


@pytest.mark.parametrize("name", ("uniform bytes", "u32 timestamps, step 1000 +- 2", "u32 sensor series", "the same as interleaved stereo"))
def test_the_advisor_chooses_the_models_order_and_writes_the_explicit_calls_bytes(torch_cuda, table, name):
    codec = trc.RCA
    esize, stride, d = table[name]
    m = d.size // esize
    comp, a = trc.host_encode_aoplanes(codec, stride, d, esize, 0)
    inner = comp if comp[:4].tobytes() == b"TRCP" else comp[16:]
    seg = trc.parse_planes(inner)[0]["chunk"]                   # the resolved chunk is the advisor's restart length
    h = OL.hist4(d, esize, seg, stride)
    est = OL.estimates(h, esize, m)
    print("%s: order-0 estimates of orders 0 .. 3 in bytes %s, choice %d, %d -> %d bytes" % (name, [int(x / 8) for x in est], a["order"], d.size, comp.size))
    assert a["order"] == OL.advise(h, 15, esize, m), name
    assert np.allclose(a["total_bits"], est, rtol=1e-9, atol=0) and (a["esize"], a["orders"], a["m"]) == (esize, 15, m)
    magic = {0: b"TRCP", 1: b"TRCF" if stride == 1 else b"TRCS"}.get(a["order"], b"TRCO")
    assert comp[:4].tobytes() == magic, name
    assert np.array_equal(comp, explicit(codec, a["order"], stride, d, esize)), name + ": not the bytes of the explicit call"
    assert np.array_equal(trc.host_decode_xplanes(comp, d.size), d), name


def test_a_smooth_series_stores_fewer_bytes_at_order_two_and_timestamps_more(torch_cuda, table):
    """256 KiB each through rccdf at the automatic chunk: the sensor series behind the zigzag delta (order 1) and behind the second
    difference; the timestamps, which the first difference already flattens, the same way"""
    sizes = {}
    for name in ("u32 sensor series", "u32 timestamps, step 1000 +- 2"):
        esize, stride, d = table[name]
        one, two = explicit(trc.RCA, 1, stride, d, esize), explicit(trc.RCA, 2, stride, d, esize)
        print("%s, %d bytes: order 1 %d, order 2 %d" % (name, d.size, one.size, two.size))
        sizes[name] = (one.size, two.size)
        assert np.array_equal(trc.host_decode_oplanes(two, d.size), d)
    assert sizes["u32 sensor series"][1] < sizes["u32 sensor series"][0]
    assert sizes["u32 timestamps, step 1000 +- 2"][1] > sizes["u32 timestamps, step 1000 +- 2"][0]


def test_trcfile_oplanes(torch_cuda, tmp_path, table):
    esize, stride, d = table["the same as interleaved stereo"]
    d = np.concatenate([d[:60001 * 2], np.array([7], dtype=np.uint8)])
    for order in (2, 3):
        head = trcfile_round_trip(tmp_path, d, "trco", ["o", "46", "2", order, stride], 70001, 3000)
        assert head[:4].tobytes() == b"TRCO" and head[4] == order and head[5] == 1 and head[6] == stride and head[16:20].tobytes() == b"TRCP"
    src, comp, back = (str(tmp_path / f) for f in ("in.bin", "adv.trc", "adv.bin"))
    r = trcfile("O", "46", "2", stride, src, comp)
    choice = int(r.stdout.rsplit("choice order", 1)[1].split()[0])
    got = np.fromfile(comp, dtype=np.uint8)
    assert np.array_equal(got, explicit(trc.RCA, choice, stride, d, 2)) and choice >= 2, r.stdout
    trcfile("d", comp, back)
    assert np.array_equal(np.fromfile(back, dtype=np.uint8), d)
    r = trcfile("o", "46", "2", "4", "2", src, comp, rc=2)
    assert "order" in r.stderr
