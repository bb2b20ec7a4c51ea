"""Byte planes behind a predictor of order 2 or 3, the parts that need no GPU: the declarations and exports, the header structs
through a C compiler, the two models of oplanes_lib against each other and against the pinned fixture
tests/golden/oplanes_vectors.npz, the inverse where every level wraps, the order's and the stride's argument errors from every new
call, trc_oplanes_check on containers assembled by hand, trc_planes_advise_order against the numpy rule, and what the orders are
for: the order-0 estimates of smooth series and of integer columns."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fplanes_lib as FL
import oplanes_lib as OL
import splanes_lib as SL
import trc
from test_fplanes_cpu import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 2**64 - 1
SYMBOLS = ("trc_planes_split_ofilter_dev", "trc_planes_join_ofilter_dev", "trc_encode_oplanes_dev", "trc_decode_oplanes_dev",
           "trc_decode_oplanes_range_dev", "trc_planes_hist_order_bytes", "trc_planes_hist_order_dev", "trc_planes_advise_order",
           "trc_oplanes_bound", "trc_encode_oplanes_host", "trc_decode_oplanes_host", "trc_decode_oplanes_range_host", "trc_oplanes_check",
           "trc_encode_aoplanes_host")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trc_hip.h")).read(), flags=re.S)


def err():
    return trc.lib().trc_last_error().decode()


def test_symbols_declared_and_exported():
    txt = header_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s + " is not declared in include/trc_hip.h"
        assert hasattr(trc.lib(), s), s + " is not exported"
    for name in ("ORDER_MAX", "planes_split_ofilter", "planes_join_ofilter", "OrderPlanesCoder", "planes_hist_order", "planes_advise_order",
                 "host_encode_oplanes", "host_decode_oplanes", "host_decode_oplanes_range", "oplanes_check", "host_encode_aoplanes", "OPLANES_MAGIC"):
        assert hasattr(trc, name), name
    assert issubclass(trc.OrderPlanesCoder, trc.PlanesCoder)
    assert trc.OrderPlanesCoder(trc.RCA, 4096, 4, 256, "cpu", order=3, stride=5)._lead() == (3, 5)
    # the filter enum is not touched: the order is an argument, not a filter
    assert re.search(r"enum\s*\{\s*TRC_FILTER_NONE\s*=\s*0\s*,\s*TRC_FILTER_ZDELTA\s*=\s*1\s*,\s*TRC_FILTER_XOR\s*=\s*2\s*\}", txt)


def test_header_structs(tmp_path):
    """sizeof(trc_oplanes_hdr) == 16 with the fields where the TRCS prefix has them and the order in the filter's place; the advice
    struct as ctypes lays it out: read from the header by a C compiler"""
    txt = header_text()
    assert re.search(r"#define\s+TRC_OPLANES_MAGIC\s+0x4f435254u", txt) and re.search(r"#define\s+TRC_ORDER_MAX\s+3\b", txt)
    assert (trc.OPLANES_MAGIC, trc.ORDER_MAX, trc.OPLANES_HDR) == (0x4f435254, 3, 16) and OL.ORDER_MAX == 3
    assert struct.pack("<I", trc.OPLANES_MAGIC) == b"TRCO"
    body = re.search(r"typedef struct trc_oplanes_hdr \{(.*?)\} trc_oplanes_hdr;", txt, flags=re.S).group(1)
    fields = re.findall(r"(uint\d+_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "magic"), ("uint8_t", "order"), ("uint8_t", "version"), ("uint16_t", "stride"), ("uint64_t", "size")]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(trc_oplanes_hdr), offsetof(trc_oplanes_hdr, order), offsetof(trc_oplanes_hdr, stride), offsetof(trc_oplanes_hdr, size), '
                   'sizeof(trc_planes_order_advice), offsetof(trc_planes_order_advice, m), offsetof(trc_planes_order_advice, bits), '
                   'offsetof(trc_planes_order_advice, total_bits), TRC_ORDER_MAX); return 0; }\n')
    exe = tmp_path / "sz"
    r = subprocess.run([os.environ.get("CC", "cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    A = trc.PlanesOrderAdvice
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == \
        ["16", "4", "6", "8", str(C.sizeof(A)), str(A.m.offset), str(A.bits.offset), str(A.total_bits.offset), "3"]


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_the_two_models_agree_on_the_golden_cases():
    golden = OL.load_golden()
    assert [g[0] for g in golden] == OL.golden_cases() and len(golden) >= 30
    assert {(g[0][0], g[0][1], g[0][2]) for g in golden} >= {(e, k, s) for e in OL.ESIZES for k in OL.ORDERS for s in OL.STRIDES}
    assert {g[0][6] for g in golden} == set(OL.KINDS)
    stored = 0
    for case, in_sha, out_sha, out in golden:
        esize, order, stride, seg, m, t, kind = case
        d = OL.golden_input(case)
        assert OL.sha(d) == in_sha, ("the input generator changed", case)
        f, g = OL.forward(d, esize, order, seg, stride), OL.scalar_forward(d, esize, order, seg, stride)
        assert np.array_equal(f, g), case
        assert OL.sha(f) == out_sha, case
        if out is not None:
            stored += 1
            assert np.array_equal(f, out), case
        else:
            assert f.size > OL.GOLDEN_STORE_MAX
        assert np.array_equal(f[m * esize:], d[m * esize:]), "the tail bytes are not filtered"
        assert np.array_equal(OL.inverse(f, esize, order, seg, stride), d), case
    assert stored >= 20
    assert os.path.getsize(OL.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("esize", OL.ESIZES)
def test_orders_zero_and_one_are_no_filter_and_the_strided_zigzag_delta(esize):
    for stride in (1, 3, 8):
        for seg, m, t in ((256, 700, esize - 1), (320, 961, 0)):
            d = OL.gen("smooth", esize, m, t, m + stride, stride)
            assert np.array_equal(OL.forward(d, esize, 0, seg, stride), d)
            assert np.array_equal(OL.forward(d, esize, 1, seg, stride), SL.forward(d, esize, FL.ZDELTA, seg, stride))
            assert np.array_equal(OL.scalar_forward(d, esize, 1, seg, stride), SL.scalar_forward(d, esize, FL.ZDELTA, seg, stride))


@pytest.mark.parametrize("esize", OL.ESIZES)
@pytest.mark.parametrize("order", OL.ORDERS)
def test_model_is_the_closed_form_at_every_stride_and_restart_length_of_the_gpu_matrix(esize, order):
    """the points the GPU tests add to the fixture's: strides 4, 6 and 7 (OL.ALL_STRIDES beyond OL.STRIDES) at 256 and every length of
    FL.RESTARTS, over two restarts and a ragged end -- the model is a sound yardstick there too"""
    assert set(OL.ALL_STRIDES) - set(OL.STRIDES) == {4, 6, 7}
    for stride in (4, 6, 7):
        for i, seg in enumerate((256,) + FL.RESTARTS):
            m, t = 2 * seg + 3 * stride + 2, (0, esize - 1)[i & 1]
            d = OL.gen(OL.KINDS[(i + stride) % 4], esize, m, t, 13 * m + esize, stride)
            f = OL.forward(d, esize, order, seg, stride)
            assert np.array_equal(f, OL.scalar_forward(d, esize, order, seg, stride)), (stride, seg)
            assert np.array_equal(OL.inverse(f, esize, order, seg, stride), d), (stride, seg)


@pytest.mark.parametrize("esize", OL.ESIZES)
@pytest.mark.parametrize("order", (1, 2, 3))
def test_inverse_round_trips_where_every_level_wraps(esize, order):
    """values next to 0 and next to 2^w - 1 in turn: the differences and the sums overflow at every level"""
    w = 8 * esize
    rng = np.random.default_rng(esize + order)
    for stride in (1, 3, 8):
        for seg, m, t in ((256, 5, 0), (256, 700, esize - 1), (320, 961, 1)):
            near = rng.integers(0, 4, m).astype(np.uint64)
            x = np.where(rng.integers(0, 2, m) == 1, near, np.uint64((1 << w) - 1) - near).astype(OL.DT[esize])
            d = np.concatenate([x.view(np.uint8), rng.integers(0, 256, t, dtype=np.uint8)])
            f = OL.forward(d, esize, order, seg, stride)
            assert np.array_equal(f, OL.scalar_forward(d, esize, order, seg, stride)), (stride, seg, m)
            assert np.array_equal(OL.inverse(f, esize, order, seg, stride), d), (stride, seg, m)
            for kind in ("wrap", "ones"):
                e = OL.gen(kind, esize, m, t, 3)
                assert np.array_equal(OL.inverse(OL.forward(e, esize, order, seg, stride), esize, order, seg, stride), e), (kind, stride, seg, m)


def test_a_segment_decodes_from_its_own_values():
    for esize in OL.ESIZES:
        for order in OL.ORDERS:
            seg, stride = 256, 3
            d = OL.gen("smooth", esize, 4 * seg + 17, 0, 5, stride)
            f = OL.forward(d, esize, order, seg, stride)
            part = slice(2 * seg * esize, 3 * seg * esize)
            assert np.array_equal(OL.inverse(f[part], esize, order, seg, stride), d[part])
            assert np.array_equal(OL.forward(d[part], esize, order, seg, stride), f[part])


# ---- the argument errors ----------------------------------------------------------------------------------------------------
def new_calls(order, stride):
    """every new device and host call that takes an order, with NULL pointers and sizes of zero behind it -> [(name, call -> failed)]"""
    L = trc.lib()
    return [("split", lambda: L.trc_planes_split_ofilter_dev(order, stride, None, 0, 4, 256, None, 0, None, None) == -1),
            ("join", lambda: L.trc_planes_join_ofilter_dev(order, stride, None, 0, None, 0, 4, 256, None, None) == -1),
            ("encode", lambda: L.trc_encode_oplanes_dev(trc.RCA, order, stride, None, 0, 4, 256, None, 0, None, None, None, None, None, None, 0, None) == -1),
            ("decode", lambda: L.trc_decode_oplanes_dev(trc.RCA, order, stride, None, None, None, 0, 4, 256, None, 0, None, None, 0, None) == -1),
            ("range", lambda: L.trc_decode_oplanes_range_dev(trc.RCA, order, stride, None, None, 0, 4, 256, 0, 1, None, 0, None, None, 0, None) == -1),
            ("host", lambda: L.trc_encode_oplanes_host(trc.RCA, order, stride, None, 0, 4, 256, None, 0, 0) == 0)]


@pytest.mark.parametrize("order", (-1, 4))
def test_a_bad_order_is_the_first_error_of_every_new_call(order):
    """TRC_E_ARG naming the order, ahead of a bad stride, NULL pointers and sizes of zero, and without a device"""
    for stride in (3, 0, 9):
        for name, call in new_calls(order, stride):
            assert call() and "order %d" % order in err() and "stride" not in err(), (name, err())


@pytest.mark.parametrize("stride", (0, 9))
def test_a_bad_stride_is_the_next_error(stride):
    L = trc.lib()
    for order in range(0, 4):
        for name, call in new_calls(order, stride):
            assert call() and "stride %d" % stride in err(), (name, order, err())
    for orders in (1, 4, 15):
        assert L.trc_planes_hist_order_dev(orders, stride, None, 0, 4, 256, None, None) == -1 and "stride %d" % stride in err()
    for orders in (0, 16):                                      # the bit set comes first
        assert L.trc_planes_hist_order_dev(orders, stride, None, 0, 4, 256, None, None) == -1 and "orders 0x%x" % orders in err()
    out = np.full(4096, 0xA5, dtype=np.uint8)
    d = np.zeros(1024, dtype=np.uint8)
    assert L.trc_encode_aoplanes_host(trc.RCA, stride, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0, None) == 0 and "stride %d" % stride in err()
    assert (out == 0xA5).all()


def test_good_orders_and_strides_reach_the_next_check():
    """still without a device: the next complaint is about something else"""
    L = trc.lib()
    for order in (2, 3):
        for stride in range(1, 9):
            assert L.trc_planes_split_ofilter_dev(order, stride, None, 0, 4, 100, None, 0, None, None) == -1 and "restart length 100" in err()
            assert L.trc_planes_join_ofilter_dev(order, stride, None, 4096, None, 0, 3, 256, None, None) == -1 and "esize 3" in err()
            assert L.trc_planes_split_ofilter_dev(order, stride, None, 4096, 4, 256, None, 1024, None, None) == -1 and "aligned" in err()
            assert L.trc_encode_oplanes_dev(trc.RCA | trc.TABLES_READY, order, stride, None, 0, 4, 256, None, 0, None, None, None, None, None, None, 0, None) == -1
            assert "TRC_TABLES_READY" in err()
            assert L.trc_planes_hist_order_dev(15, stride, None, 4096, 3, 256, None, None) == -1 and "esize 3" in err()
    # orders 0 and 1 are the existing calls and complain as those do
    assert L.trc_planes_split_ofilter_dev(1, 3, None, 0, 4, 100, None, 0, None, None) == -1 and "planes_split_sfilter" in err()
    assert L.trc_planes_split_ofilter_dev(1, 1, None, 4096, 4, 256, None, 1024, None, None) == -1 and "planes_split_filter" in err()


def test_host_encode_takes_order_2_or_3():
    L = trc.lib()
    d = FL.gen("monotone", 4, 5000, 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    for order, stride, other in ((0, 1, "trc_encode_planes_host"), (0, 5, "trc_encode_planes_host"), (1, 1, "trc_encode_fplanes_host"), (1, 4, "trc_encode_splanes_host")):
        assert L.trc_encode_oplanes_host(trc.RCA, order, stride, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
        assert other in err() and "order %d" % order in err()
        with pytest.raises(trc.TrcError, match=other):
            trc.host_encode_oplanes(trc.RCA, order, stride, d, 4, 256)
    with pytest.raises(trc.TrcError, match="order 4"):
        trc.host_encode_oplanes(trc.RCA, 4, 1, d, 4, 256)
    assert (out == 0xA5).all()
    # the seven low-nibble coders are refused as everywhere in the planes family, before a device is looked for
    assert L.trc_encode_oplanes_host(trc.RC4, 2, 2, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0) == 0
    assert "low four bits" in err()
    assert L.trc_encode_aoplanes_host(trc.RC4, 2, d.ctypes.data, d.size, 4, 256, out.ctypes.data, out.size, 0, None) == 0
    assert "low four bits" in err()


def test_bounds():
    L = trc.lib()
    for esize in OL.ESIZES:
        for n in (esize, 1000 * esize + esize - 1, 10**6 + 1):
            for chunk in (0, 256, 4096):
                for cdfnum in (0, 256):
                    assert L.trc_oplanes_bound(n, esize, chunk, cdfnum) == L.trc_planes_bound(n, esize, chunk, cdfnum) + 16 > 16
        assert L.trc_oplanes_bound(esize - 1, esize, 256, 0) == 0
        assert L.trc_planes_hist_order_bytes(esize) == 4 * esize * 256 * 8 == trc.planes_hist_order_bytes(esize)
    assert L.trc_oplanes_bound(4096, 3, 256, 0) == 0 and L.trc_planes_hist_order_bytes(3) == 0


# ---- trc_oplanes_check on hand-made containers ------------------------------------------------------------------------------
def wrap(inner, magic=trc.OPLANES_MAGIC, order=2, version=1, stride=3, size=None):
    b = struct.pack("<IBBHQ", magic, order, version, stride, 16 + len(inner) if size is None else size) + inner
    return np.frombuffer(b, dtype=np.uint8).copy()


def check(buf, buflen=None, outlen=ANY):
    return trc.lib().trc_oplanes_check(buf.ctypes.data, buf.size if buflen is None else buflen, outlen)


@pytest.mark.parametrize("esize,t", [(2, 1), (4, 0), (8, 7)])
def test_check_accepts(esize, t):
    inner, n = make(esize, t)
    for order in OL.ORDERS:
        for stride in range(1, 9):
            buf = wrap(inner, order=order, stride=stride)
            assert check(buf) == 0 and check(buf, outlen=n) == 0, err()
            trc.oplanes_check(buf, n)
            assert check(np.concatenate([buf, np.zeros(100, np.uint8)])) == 0         # slack behind the container is fine
            assert trc.lib().trc_planes_check(buf[16:].ctypes.data, buf.size - 16, n) == 0        # the inner part is a TRCP container as it stands


def test_check_rejects_each_defect():
    inner, n = make(4, 1)
    good = wrap(inner)
    assert check(good) == 0
    for magic in (trc.SPLANES_MAGIC, trc.FPLANES_MAGIC, trc.PLANES_MAGIC):
        assert check(wrap(inner, magic=magic)) != 0 and "magic" in err()
    assert check(np.frombuffer(inner, dtype=np.uint8).copy()) != 0 and "magic" in err()  # a bare TRCP container
    assert check(wrap(inner, version=2)) != 0 and "version" in err()
    for order in (0, 1, 4, 255):
        assert check(wrap(inner, order=order)) != 0 and "order %d" % order in err()
    for stride in (0, 9, 256, 65535):
        assert check(wrap(inner, stride=stride)) != 0 and "stride %d" % stride in err()
    assert check(wrap(inner, order=4, stride=9)) != 0 and "order 4" in err()             # the order is looked at first
    assert check(wrap(inner, size=16)) != 0 and "size 16" in err()                       # size <= 16: no room for an inner container
    assert check(wrap(inner, size=15)) != 0 and "size 15" in err()
    assert check(wrap(inner, size=16 + len(inner) + 8)) != 0 and "buffer holds" in err()      # size > buflen
    assert check(good, buflen=good.size - 1) != 0 and "buffer holds" in err()
    assert check(good, buflen=15) != 0 and "shorter than the header" in err()
    assert check(wrap(inner[:-9])) != 0 and "planes container" in err()                  # a broken inner container
    assert check(wrap(inner, size=16 + len(inner) - 9)) != 0 and "planes container" in err()
    assert check(wrap(make(4, 1, version=2)[0])) != 0 and "planes container" in err()
    assert check(good, outlen=n - 1) != 0 and "caller expects" in err()
    with pytest.raises(trc.TrcError, match="stride 9"):
        trc.oplanes_check(wrap(inner, stride=9))
    # the decoders check first, before a device is looked for, and write nothing
    L = trc.lib()
    out = np.full(n + 64, 0xA5, dtype=np.uint8)
    bad = wrap(inner, order=4)
    for name in ("trc_decode_oplanes_host", "trc_decode_xplanes_host"):
        assert getattr(L, name)(bad.ctypes.data, bad.size, out.ctypes.data, n) == 0 and "order 4" in err(), name
    assert L.trc_decode_oplanes_range_host(bad.ctypes.data, bad.size, 0, 8, out.ctypes.data) == 0 and "order 4" in err()
    assert L.trc_decode_oplanes_host(good.ctypes.data, good.size, out.ctypes.data, n - 1) == 0 and "caller expects" in err()
    assert L.trc_decode_splanes_host(good.ctypes.data, good.size, out.ctypes.data, n) == 0 and "magic" in err()      # a TRCO container is not a TRCS container
    assert (out == 0xA5).all()


# ---- trc_planes_advise_order -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return OL.table_inputs(1 << 16)


def test_advise_order_is_the_numpy_rule_on_the_table(table):
    """the estimates are the model's to 1e-9 relative; the choice is the model's; smooth series choose an order above 1 and store
    less at order 2 than at order 1, integer columns choose order 1 and store more at order 2"""
    seg = 4096
    for name, esize, stride, d in table:
        m = d.size // esize
        h = OL.hist4(d, esize, seg, stride)
        a = trc.planes_advise_order(h, 15, esize, m)
        est = OL.estimates(h, esize, m)
        print("%s: order-0 estimates of orders 0 .. 3 in bytes: %s, choice %d" % (name, [int(x / 8) for x in est], a["order"]))
        assert np.allclose(a["total_bits"], est, rtol=1e-9, atol=0) and np.allclose(a["bits"].sum(axis=1), est, rtol=1e-9, atol=0)
        assert (a["esize"], a["orders"], a["m"]) == (esize, 15, m)
        assert a["order"] == OL.advise(h, 15, esize, m), name
        for orders in (1, 2, 6, 9, 12, 13):
            b = trc.planes_advise_order(h, orders, esize, m)
            assert b["order"] == OL.advise(h, orders, esize, m) and orders >> b["order"] & 1, (name, orders)
            assert all(b["total_bits"][k] == (a["total_bits"][k] if orders >> k & 1 else 0) for k in range(4))
        smooth = "PCM" in name or "stereo" in name or "sensor" in name
        assert (est[2] < est[1]) == smooth and (a["order"] >= 2) == smooth, name
        # rows 0 and 1 are the rows of the stride histograms
        assert np.array_equal(h[:2 * esize * 256], SL.hist3(d, esize, seg, stride)[:2 * esize * 256])


def shaped(m, delta):
    """uint64 [2, 256]: plane 0 uniform, plane 1 uniform with `delta` moved from each of the upper 128 bins to the lower 128"""
    flat = np.full(256, m // 256, dtype=np.uint64)
    tilt = flat.copy()
    tilt[:128] += np.uint64(delta)
    tilt[128:] -= np.uint64(delta)
    return np.stack([flat, tilt])


def test_advise_order_one_64th_rule_and_ties():
    esize, m = 2, 1 << 16
    flat = shaped(m, 0)

    def hist(r0, r1, r2, r3):
        return np.concatenate([r.reshape(-1) for r in (r0, r1, r2, r3)])
    # the smallest tilt whose saving reaches 1/64 of the unfiltered total, by the model
    tot0 = OL.estimates(hist(flat, flat, flat, flat), esize, m)[0]
    delta = next(dl for dl in range(1, 256) if tot0 - OL.estimates(hist(flat, flat, shaped(m, dl), flat), esize, m)[2] >= tot0 / 64)
    assert delta > 2
    below, at = hist(flat, flat, shaped(m, delta - 1), flat), hist(flat, flat, shaped(m, delta), flat)
    assert trc.planes_advise_order(below, 15, esize, m)["order"] == 0 == OL.advise(below, 15, esize, m)
    assert trc.planes_advise_order(at, 15, esize, m)["order"] == 2 == OL.advise(at, 15, esize, m)
    assert trc.planes_advise_order(below, 14, esize, m)["order"] == 2          # order 0 not requested: the argmin stands
    # ties go to the lower order
    t = shaped(m, 200)
    assert trc.planes_advise_order(hist(flat, t, t, t), 15, esize, m)["order"] == 1
    assert trc.planes_advise_order(hist(flat, flat, t, t), 15, esize, m)["order"] == 2
    assert trc.planes_advise_order(hist(flat, flat, t, t), 8, esize, m)["order"] == 3
    assert trc.planes_advise_order(hist(flat, flat, flat, flat), 15, esize, m)["order"] == 0


def test_advise_order_argument_errors():
    L = trc.lib()
    esize, m = 2, 1 << 16
    flat = shaped(m, 0)
    h = np.concatenate([flat.reshape(-1)] * 4)
    a = trc.PlanesOrderAdvice()
    assert L.trc_planes_advise_order(h.ctypes.data, 15, esize, m, C.byref(a)) == 0
    for k in range(4):                                          # a requested row that does not sum to m
        for step in (1, -1):
            bad = h.copy()
            bad[(k * esize + 1) * 256 + 7] = int(h[(k * esize + 1) * 256 + 7]) + step
            assert L.trc_planes_advise_order(bad.ctypes.data, 15, esize, m, C.byref(a)) == -1 and "order %d plane 1" % k in err()
            assert L.trc_planes_advise_order(bad.ctypes.data, 15 & ~(1 << k), esize, m, C.byref(a)) == 0      # ... is not read where not requested
    for orders in (0, 16):
        assert L.trc_planes_advise_order(h.ctypes.data, orders, esize, m, C.byref(a)) == -1 and "orders" in err()
    assert L.trc_planes_advise_order(h.ctypes.data, 15, 3, m, C.byref(a)) == -1 and "esize 3" in err()
    assert L.trc_planes_advise_order(h.ctypes.data, 15, esize, 0, C.byref(a)) == -1
    assert L.trc_planes_advise_order(None, 15, esize, m, C.byref(a)) == -1 and L.trc_planes_advise_order(h.ctypes.data, 15, esize, m, None) == -1
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_advise_order(h, 15, esize, m + 1)


# ---- the harness --------------------------------------------------------------------------------------------------------------
def test_trcfile_compiles_against_headers_and_knows_the_modes(tmp_path):
    lib = os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    assert os.path.exists(lib), "libturborc_hip.so is not built"
    exe = tmp_path / "trcfile"
    libdir = os.path.dirname(lib)
    r = subprocess.run([os.environ.get("CC", "cc"), "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "harness", "trcfile.c"),
                        "-o", str(exe), "-L" + libdir, "-lturborc_hip", "-lm", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 2 and "trcfile o <id> <esize> <order> <stride> <in> <out>" in u.stderr and "trcfile O <id> <esize> <stride> <in> <out>" in u.stderr
    d = tmp_path / "in.bin"
    OL.gen("smooth", 2, 1000, 0, 1).tofile(str(d))
    for order, stride, word in (("1", "2", "order"), ("4", "2", "order"), ("2", "0", "stride"), ("3", "9", "stride")):      # refused before the library is asked
        r = subprocess.run([str(exe), "o", "46", "2", order, stride, str(d), str(tmp_path / "o")], capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr
    r = subprocess.run([str(exe), "O", "46", "2", "9", str(d), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 2 and "stride" in r.stderr
