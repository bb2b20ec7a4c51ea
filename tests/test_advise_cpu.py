"""CPU: the host half of the planes advisor -- trc_planes_advise on numpy histograms (advise_lib), trc_planes_hist_bytes, and the
magic dispatch of trc_decode_xplanes_host.  The library loads without a device.

What the choice has to be is known ahead of any code (order-0 estimates as fractions of the input, esize 2 / 4 / 8, seg 256,
m = 4105 and 65 539): weights lose 1.4 % or more under either filter; the sorted series gains 18 % or more from the zigzag delta
and less from xor; one flipped bit per element makes xor beat the zigzag delta by 19 % or more; on uniform words the three totals
differ by 0.1 % (m = 4105) or 0.03 % (m = 65 539) at most, far inside the 1/64 a filter has to earn."""
import numpy as np
import pytest

import advise_lib as AL
import fplanes_lib as FL
import trc
from planes_matrix_lib import LOW4, LOW4_TEXT

SEG = 256
MS = (4105, 65539)
CHOICE = {"weights": FL.NONE, "monotone": FL.ZDELTA, "walk": FL.ZDELTA, "bitflip": FL.XOR, "random": FL.NONE}
_cache = {}


def case(kind, esize, m):
    """-> (histograms [3, esize, 256] of all three filters, the model's advice): computed once, shared, left unchanged"""
    key = (kind, esize, m)
    if key not in _cache:
        h = AL.hist(AL.gen(kind, esize, m, esize - 1, 5 * m + esize), esize, SEG, AL.ALL)
        h.setflags(write=False)
        _cache[key] = (h, AL.advise(h, AL.ALL, esize, m))
    return _cache[key]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("esize", FL.ESIZES)
@pytest.mark.parametrize("kind", sorted(CHOICE))
def test_choice_and_estimates(kind, esize, m):
    h, (choice, bits, total) = case(kind, esize, m)
    assert choice == CHOICE[kind], "the model itself: %s" % (total / (8.0 * m * esize),)
    a = trc.planes_advise(h, AL.ALL, esize, m)
    assert a["filter"] == CHOICE[kind], (kind, esize, m, a["total_bits"] / (8.0 * m * esize))
    assert (a["esize"], a["filters"], a["m"]) == (esize, AL.ALL, m)
    # 256 double terms per plane, each within an ulp or two of numpy's: about 1e-13 relative
    assert np.allclose(a["bits"], bits, rtol=1e-9, atol=0), np.abs(a["bits"] - bits).max()
    assert np.allclose(a["total_bits"], total, rtol=1e-9, atol=0)
    assert not a["bits"][:, esize:].any()


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_margins_of_the_inputs(esize):
    """the margins the choices rest on (and the GPU test's size claim): not a property of the library, of the inputs"""
    for m in MS:
        frac = {k: case(k, esize, m)[1][2] / (8.0 * m * esize) for k in CHOICE}
        assert min(frac["weights"][1:]) >= 1.01 * frac["weights"][0]
        assert frac["monotone"][1] <= 0.82 * min(frac["monotone"][0], frac["monotone"][2])
        assert frac["bitflip"][2] <= 0.81 * frac["bitflip"][1] <= 0.5 * frac["bitflip"][0]
        assert np.ptp(frac["random"]) <= frac["random"][0] / 640     # sampling noise: a tenth of what the 1/64 rule asks for


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_subsets_of_filters(esize):
    m = MS[0]
    for kind in sorted(CHOICE):
        h = case(kind, esize, m)[0]
        for filters in range(1, 8):
            hf = h.copy()
            for f in range(3):
                if not filters >> f & 1:
                    hf[f] = 0xA5A5                               # rows that were not requested are not looked at
            choice, bits, total = AL.advise(hf, filters, esize, m)
            a = trc.planes_advise(hf, filters, esize, m)
            assert a["filter"] == choice and filters >> a["filter"] & 1, (kind, filters)
            assert np.allclose(a["bits"], bits, rtol=1e-9, atol=0)
            if filters == 6:
                assert a["filter"] != FL.NONE                    # random data included: the 1/64 rule needs NONE among the requested
            for f in range(3):
                if not filters >> f & 1:
                    assert not a["bits"][f].any() and a["total_bits"][f] == 0


def test_ties_go_to_the_lower_id():
    esize, m = 2, 1000
    h = np.zeros((3, esize, 256), dtype=np.uint64)
    h[:, :, 3] = 600
    h[:, :, 200] = 400
    for filters, want in ((7, 0), (6, 1), (4, 2), (5, 0)):
        assert trc.planes_advise(h, filters, esize, m)["filter"] == want


def test_the_one_in_64_rule_is_about_the_unfiltered_total():
    """two symbols per plane under no filter: 1000 bits per plane; a filter that gives (p, 1 - p)"""
    esize, m = 2, 1000
    h = np.zeros((3, esize, 256), dtype=np.uint64)
    h[0, :, 0] = h[0, :, 1] = 500
    h[2, :, 0], h[2, :, 1] = 1, 999                              # xor: nearly free
    for z0, want in ((400, FL.ZDELTA), (460, FL.NONE)):          # H(0.4) = 0.971: saves 2.9 %;  H(0.46) = 0.9954: saves 0.5 %
        h[1, :, 0], h[1, :, 1] = z0, m - z0
        assert trc.planes_advise(h, 3, esize, m)["filter"] == want
        assert trc.planes_advise(h, 7, esize, m)["filter"] == FL.XOR
        assert trc.planes_advise(h, 2, esize, m)["filter"] == FL.ZDELTA


def test_argument_errors():
    esize, m = 4, MS[0]
    h = case("monotone", esize, m)[0]
    trc.planes_advise(h, 7, esize, m)
    for filters in (0, 8):
        with pytest.raises(trc.TrcError, match="rc=-1.*filters"):
            trc.planes_advise(h, filters, esize, m)
    with pytest.raises(trc.TrcError, match="rc=-1.*esize 3"):
        trc.planes_advise(h, 7, 3, m)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_advise(h, 7, esize, 0)
    for f, k, delta in ((0, 0, 1), (1, 3, -1), (2, 2, 1)):
        bad = h.copy()
        b = int(np.flatnonzero(bad[f, k])[0])
        bad[f, k, b] = int(bad[f, k, b]) + delta
        with pytest.raises(trc.TrcError, match="rc=-1.*filter %d plane %d" % (f, k)):
            trc.planes_advise(bad, 7, esize, m)
        if f:
            assert trc.planes_advise(bad, 1, esize, m)["filter"] == FL.NONE      # ... which is not among the requested rows
    huge = h.copy()
    huge[1, 1, 7] = (1 << 64) - 1                                 # a row whose sum would wrap
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_advise(huge, 7, esize, m)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_advise(h, 7, esize, m + 1)


@pytest.mark.parametrize("codec", LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_aplanes_refuses_a_low_nibble_coder_before_any_device(codec):
    """the coder is refused before the input is uploaded for its histograms: 0, the reason, nothing written, with or without a GPU"""
    d = AL.gen("monotone", 4, MS[0], 3, 1)
    out = np.full(d.size + 4096, 0xA5, dtype=np.uint8)
    a = trc.PlanesAdvice()
    a.filter = 77
    cn = trc.ss_prm((4, 7)) if codec in trc.SSBIT else 0
    for chunk in (0, SEG):
        assert trc.lib().trc_encode_aplanes_host(codec, d.ctypes.data, d.size, 4, chunk, out.ctypes.data, out.size, cn, a) == 0
        assert LOW4_TEXT in trc.lib().trc_last_error().decode()
    assert (out == 0xA5).all() and a.filter == 77
    with pytest.raises(trc.TrcError, match=LOW4_TEXT):
        trc.encode_aplanes_host(codec, d, 4, 0, prm=(4, 7))


def test_hist_bytes():
    assert [trc.planes_hist_bytes(e) for e in (2, 4, 8)] == [3 * e * 256 * 8 for e in (2, 4, 8)]
    assert [trc.planes_hist_bytes(e) for e in (0, 1, 3, 16)] == [0, 0, 0, 0]


def test_xplanes_refuses_other_containers():
    """the dispatch looks at the magic before any device is needed: a TRC1 container and garbage are refused with a reason"""
    import struct
    trc1 = struct.pack("<IBBHIIQQ", 0x31435254, 4, 1, 0, 1024, 1, 100, 50) + struct.pack("<I", 50) + bytes(50)
    for buf in (trc1, b"TRCX" + bytes(100), bytes(64), b"TR", b""):
        comp = np.frombuffer(buf + bytes(8), dtype=np.uint8)[:len(buf)]
        with pytest.raises(trc.TrcError, match="neither a planes"):
            trc.host_decode_xplanes(comp, 100)
    # the two magics it knows go to their decoders, which refuse these stubs as corrupt, not as unknown
    for magic in (b"TRCP", b"TRCF"):
        with pytest.raises(trc.TrcError, match="container"):
            trc.host_decode_xplanes(np.frombuffer(magic + bytes(60), dtype=np.uint8), 100)
