"""The planes advisor on the MI355X.  trc_planes_hist_dev counts, so every comparison is exact equality with the numpy model of
advise_lib: at the edges of a thread's vector, a restart segment, a workgroup and the grid; with every lane on one bin; across
flushes of the 32-bit counters; into a dirty buffer.  trc_encode_aplanes_host must write byte for byte what the explicit call for
its choice writes, and `trcfile a / d` must round-trip.  Every device buffer is followed by a 512-byte guard of 0xA5 that must
survive (the histogram call's have one on both sides); that call and its comparisons are in gpu_planes.py."""
import numpy as np
import pytest

import advise_lib as AL
import fplanes_lib as FL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, assert_hists, device_hists, guarded, trcfile

pytestmark = pytest.mark.gpu
MS = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4097, 65539)
SEGS = (256, 320)
M_BIG = 65539
M_AUTO = 200 * CHUNK + 100


_model = {}


def model(kind, esize, m, t, seg, seed=None):
    """-> (input bytes, histograms of all three filters): computed once per key, shared, left unchanged"""
    key = (kind, esize, m, t, seg, seed)
    if key not in _model:
        d = AL.gen(kind, esize, m, t, 100 * m + 10 * esize + t if seed is None else seed)
        h = AL.hist(d, esize, seg, AL.ALL)
        d.setflags(write=False)
        h.setflags(write=False)
        _model[key] = (d, h)
    return _model[key]


def hist_case(torch, kind, esize, m, t, seg, filters, seed=None):
    d, exp = model(kind, esize, m, t, seg, seed)
    got, _ = device_hists(torch, esize, seg, filters, d=d)
    assert_hists(got, exp, [m], filters, "%s esize %d m %d t %d seg %d filters %d" % (kind, esize, m, t, seg, filters))


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", (1, 2, 4, 7))
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_histograms_equal_the_model(torch_cuda, esize, filters):
    for m in MS:
        for t in (0, esize - 1):
            for seg in SEGS:
                for kind in ("random", "wrap"):
                    hist_case(torch_cuda, kind, esize, m, t, seg, filters)


@pytest.mark.parametrize("filters", (3, 5, 6))
def test_pairs_of_filters(torch_cuda, filters):
    for esize in FL.ESIZES:
        hist_case(torch_cuda, "wrap", esize, 4097, esize - 1, 320, filters)
        hist_case(torch_cuda, "monotone", esize, M_BIG, 0, 256, filters)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_every_lane_on_one_bin(torch_cuda, esize):
    """all elements equal: every lane of every wave adds to the same bin of every plane, under every filter (the filtered planes are
    zero but for each segment's first element); and weights, whose sign / exponent plane has a handful of bins"""
    torch = torch_cuda
    d = np.tile(np.arange(0x81, 0x81 + esize, dtype=np.uint8), M_BIG)
    exp = AL.hist(d, esize, 256, AL.ALL)
    for filters in (1, 7):
        got, _ = device_hists(torch, esize, 256, filters, d=d)
        assert_hists(got, exp, [M_BIG], filters, "equal elements, esize %d, filters %d" % (esize, filters))
    assert exp[0, 0, 0x81] == M_BIG and exp[2, 0, 0] == M_BIG - 257           # (257 segments open with the element itself)
    for filters in (1, 7):
        hist_case(torch, "weights", esize, M_BIG, esize - 1, 256, filters, seed=7)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_grid_stride_loop(torch_cuda, esize, monkeypatch):
    """three workgroups for 8192 vectors: the loop turns 10 or 11 times, the last turn with idle threads"""
    monkeypatch.setenv("TRC_PLANES_GRID", "3")
    for kind, seg in (("random", 256), ("wrap", 320), ("walk", 256)):
        hist_case(torch_cuda, kind, esize, M_BIG, esize - 1, seg, 7)
    hist_case(torch_cuda, "monotone", esize, M_BIG, 0, 320, 2)


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_counters_flush_in_between(torch_cuda, esize, monkeypatch):
    """two workgroups, 16 turns each, a flush every 5: three flushes inside the loop and the one at the end; then a flush at
    every turn"""
    monkeypatch.setenv("TRC_PLANES_GRID", "2")
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "5")
    hist_case(torch_cuda, "random", esize, M_BIG, 0, 256, 7)
    hist_case(torch_cuda, "walk", esize, M_BIG, esize - 1, 320, 7)
    monkeypatch.setenv("TRC_PLANES_HIST_ROUND_VECS", "1")
    hist_case(torch_cuda, "wrap", esize, M_BIG, esize - 1, 256, 7)
    hist_case(torch_cuda, "wrap", esize, M_BIG, esize - 1, 256, 4)


def test_the_call_zeroes_a_dirty_buffer(torch_cuda):
    torch = torch_cuda
    esize = 4
    d1, h1 = model("random", esize, 4097, 0, 256)
    d2, h2 = model("wrap", esize, 513, 3, 256)
    got, d_hist = device_hists(torch, esize, 256, 7, d=d1)
    assert_hists(got, h1, [4097], 7, "first call")
    got, _ = device_hists(torch, esize, 256, 2, d=d2, d_hist=d_hist)          # fewer elements, fewer filters, the same buffer
    assert_hists(got, h2, [513], 2, "second call into the first one's counts")


def test_argument_errors_write_nothing(torch_cuda):
    torch = torch_cuda
    d_in, d_hist = guarded(torch, 4096), guarded(torch, trc.planes_hist_bytes(8))
    bad = [(7, d_in, 4096, 3, 256, d_hist), (7, d_in, 1, 2, 256, d_hist), (7, d_in, 7, 8, 256, d_hist),          # esize 3, no whole element
           (7, d_in, 4096, 2, 100, d_hist), (7, d_in, 4096, 2, 128, d_hist), (7, d_in, 4096, 2, 65600, d_hist),  # the restart length
           (7, d_in[8:], 1024, 2, 256, d_hist), (7, d_in, 4096, 4, 256, d_hist[4:]),                             # alignment of either buffer
           (0, d_in, 4096, 2, 256, d_hist), (8, d_in, 4096, 2, 256, d_hist)]                                     # the bit set
    for filters, inp, n, esize, seg, hist in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_hist(filters, inp, n, esize, seg, hist)
    torch.cuda.synchronize()
    assert (d_hist.cpu().numpy() == 0xA5).all() and (d_in.cpu().numpy() == 0xA5).all()


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", (2, 4))
@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_auto_container(torch_cuda, codec, esize):
    """byte identity with the explicit call for the choice, the advice, the round trip; and, on the two inputs where a filter wins
    by 18 % of the order-0 estimate or more, the auto container is no larger than either other explicit container (at chunk 256
    the CPU oracle orders the coded sizes of both coders the same way)"""
    t = esize - 1
    for kind, want in (("weights", FL.NONE), ("monotone", FL.ZDELTA), ("bitflip", FL.XOR)):
        d = AL.gen(kind, esize, M_AUTO, t, 31 * esize + 7)
        n = d.size
        tag = "%s esize %d %s" % (trc.CODEC_NAMES[codec], esize, kind)
        auto, adv = trc.encode_aplanes_host(codec, d, esize, CHUNK)
        explicit = {FL.NONE: trc.host_encode_planes(codec, d, esize, CHUNK)}
        for f in FL.FILTERS:
            explicit[f] = trc.host_encode_fplanes(codec, f, d, esize, CHUNK)
        assert adv["filter"] == want, tag + ": chose %d, totals %s" % (adv["filter"], adv["total_bits"])
        assert np.array_equal(auto, explicit[want]), tag + ": not the explicit call's bytes"
        assert auto[:4].tobytes() == (b"TRCF" if want else b"TRCP")
        choice, bits, total = AL.advise(AL.hist(d, esize, CHUNK, AL.ALL), AL.ALL, esize, M_AUTO)
        assert choice == want and (adv["esize"], adv["filters"], adv["m"]) == (esize, AL.ALL, M_AUTO)
        assert np.allclose(adv["bits"], bits, rtol=1e-9, atol=0) and np.allclose(adv["total_bits"], total, rtol=1e-9, atol=0), tag
        assert np.array_equal(trc.host_decode_xplanes(auto, n), d), tag + ": round trip"
        if want:
            assert all(auto.size <= explicit[f].size for f in explicit), tag + ": sizes %s" % {f: explicit[f].size for f in explicit}
    with pytest.raises(trc.TrcError, match="neither a planes"):
        trc.host_decode_xplanes(trc.encode_host_container(trc.RCA, d[:4096], 1024), 4096)


def test_auto_container_automatic_chunk(torch_cuda):
    """chunk 0 resolves as in the explicit calls, and the histograms restart where the coded call will"""
    esize = 4
    d = AL.gen("monotone", esize, 9 * 4096 + 3, esize - 1, 23)
    auto, adv = trc.encode_aplanes_host(trc.RCA, d, esize, 0)
    assert adv["filter"] == FL.ZDELTA
    assert np.array_equal(auto, trc.host_encode_fplanes(trc.RCA, FL.ZDELTA, d, esize, 0))
    hdr, _, _ = trc.parse_planes(auto[16:])
    _, _, total = AL.advise(AL.hist(d, esize, hdr["chunk"], AL.ALL), AL.ALL, esize, d.size // esize)
    assert np.allclose(adv["total_bits"], total, rtol=1e-9, atol=0)
    assert np.array_equal(trc.host_decode_xplanes(auto, d.size), d)


def test_trcfile_auto(torch_cuda, tmp_path):
    d = FL.gen("monotone", 4, 40000, 3, 9)
    src, comp, back, ref = (str(tmp_path / f) for f in ("in.bin", "in.trca", "out.bin", "in.trcf"))
    d.tofile(src)
    r = trcfile("a", "46", "4", src, comp)
    assert r.stdout.rstrip().endswith("choice z"), (r.stdout, r.stderr)
    trcfile("d", comp, back)
    assert np.array_equal(np.fromfile(back, dtype=np.uint8), d)
    trcfile("f", "46", "4", "z", src, ref)
    assert np.array_equal(np.fromfile(comp, dtype=np.uint8), np.fromfile(ref, dtype=np.uint8))
