"""The byte-plane calls around one coder of every launcher, on the MI355X.  test_gpu_planes.py / test_gpu_fplanes.py cover the edges of
split, join and the filters with four coders; the flat calls of every coder are covered by their family files.  This file covers the
product: what the planar wrapper does for a coder whose workspace holds more than a scratch region (a model area, an aux array, a
second scratch per lane), with an even number of directory bytes per plane, through the range workspace and through the host
containers.  And it pins that the seven coders of in[i] & 15 are refused by every coded planes entry point.  CODECS run at two
element sizes; every other whole-byte coder of the table (MORE) runs the same checks at esize 4, so no assigned id is left out.

Shape: chunk c = 256 (1024 for anscdf1), m = 66 c + 100 elements per plane (nc = 67: odd, two 64-chunk groups, a ragged last chunk,
plane 1's directory at byte 268), t = esize - 1 tail bytes.  Plane k is the input of test_gpu_range.py for that coder with its seeds
offset by 10 k, so every plane mixes raw and coded chunks of data the coder's own tests code; the call's input is the join of the
planes (behind a filter: the inverse filter of the join).  Every comparison is byte equality: plane k's directory, payload, total
and CDF against a fresh trc.DeviceCoder run on plane k, decoded bytes against the input, 0xA5 / 0x5A guards behind every buffer."""
import copy

import numpy as np
import pytest

import fplanes_lib as FL
import planes_lib as PL
import planes_matrix_lib as ML
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import GUARD, PRM, encode_guarded, guarded

pytestmark = pytest.mark.gpu
NCH, LAST = 67, 100
RANGES = [(0, 1), (63, 2), (1, 64), (66, 1), (0, 67)]
MIN_EACH = 10                                                   # raw and coded chunks in every plane's directory, at least
# one coder per launcher of csrc/trc_launch.h that codes whole bytes (test_gpu_range.py::CODECS without its two nibble coders), the
# varint coder on the ss predictor (its two parameters travel in cdfnum to every plane) and the word coder with the largest model
CODECS = [trc.ANS4S, trc.RCS1, trc.RCS2, trc.RCSM, trc.RCB, trc.RCA, trc.RCAI, trc.RCV8, trc.ANSA, trc.ANSO1, trc.ANSB,
          trc.VLCU16, trc.VLAU16, trc.RCC1, trc.RCG16, trc.RCR32, trc.RCBVZ16, trc.RCW16, trc.RCU3, trc.RCU3SS, trc.RCC2W32]
# every other coder that codes whole bytes, at esize 4 only: the remaining members of each family (their launchers are covered above;
# their model areas, element widths and scratch shapes differ)
MORE = [c for c in ML.ASSIGNED if c not in ML.LOW4 and c not in CODECS]
# the smallest chunk the automatic rules and the host-pointer calls use (include/trc_hip.h: 4096 for the order-1 rANS,
# TRC_O1BIT_CHUNK_MIN for the coders with trees in the workspace)
FLOOR = {trc.ANSO1: 4096}
FLOOR.update({c: 16384 for c in (trc.RCC1, trc.RCX1, trc.RCBV16, trc.RCBVZ16, trc.RCBVZ32, trc.RCW16, trc.RCW32, trc.RCCW32, trc.RCC2W32)})
AUTO_M = 40000                                                  # elements per plane of the automatic-chunk case: three chunks at 16384
PLANE_SEED = {}                                                 # (codec, plane) -> seed offset, where 10 * plane misses MIN_EACH
by_coder = pytest.mark.parametrize("codec", CODECS + MORE, ids=lambda c: trc.CODEC_NAMES[c])


def esizes(codec):
    """every coder at 4; those at even positions of CODECS at 2 as well, those at odd positions at 8 (rcc2s32, whose workspace is
    the largest, is at an even one)"""
    if codec in MORE:
        return (4,)
    return (4, 2) if CODECS.index(codec) % 2 == 0 else (4, 8)


assert CODECS.index(trc.RCC2W32) % 2 == 0 and len(CODECS) == 21 and len(CODECS) + len(MORE) + len(ML.LOW4) == len(ML.ASSIGNED)


class Data:
    """esize planes of one coder's mixed input, their tail and their join"""

    def __init__(self, codec, esize, nch, last, base=0, chunk=None):
        self.codec, self.esize = codec, esize
        planes = []
        for k in range(esize):
            self.m, self.c, p = ML.mixed_input(codec, nch, last, base + PLANE_SEED.get((codec, k), 10 * k), chunk)
            planes.append(p)
        self.planes = np.stack(planes)
        self.t = esize - 1
        self.tail = np.random.default_rng(1000 * codec + esize + base).integers(0, 256, self.t, dtype=np.uint8)
        self.d = PL.join(self.planes, self.tail)
        self.n = self.d.size
        assert self.n == self.m * esize + self.t and np.array_equal(PL.split(self.d, esize)[0], self.planes)


def reference(torch, data):
    """per plane what a fresh trc.DeviceCoder gives for it: dict(clen, payload, cdf, status)"""
    out = []
    for k in range(data.esize):
        dc = trc.DeviceCoder(data.codec, data.m, data.c, "cuda:0")
        d_plane = torch.from_numpy(np.concatenate([data.planes[k], np.zeros(GUARD, np.uint8)])).to("cuda:0")
        r = dict(cdf=None, status=None)
        if data.codec in trc.STATIC:
            dc.cdfini(d_plane, data.m, 256)
        dc.encode(d_plane, data.m, prm=PRM)
        r["clen"], r["payload"] = dc.result(data.m)
        if data.codec in trc.STATIC:
            r["cdf"], r["status"] = dc.cdf[:257].cpu().numpy().view(np.uint16).copy(), int(dc.status[0].item())
        out.append(r)
        del dc
    return out


def result_of(pc, k, n):
    """plane k's (clen, payload, total) of an encode of n bytes in a PlanesCoder that may be sized for more"""
    pc.torch.cuda.synchronize()
    m = n // pc.esize
    nc, pitch = trc.nchunks(m, pc.chunk), trc.planes_pitch(n, pc.esize)
    tot = int(pc.total[:8 * pc.esize].cpu().numpy().view("<u8")[k])
    clen = pc.clen[4 * k * nc:4 * (k + 1) * nc].cpu().numpy().view(np.uint32).copy()
    return clen, pc.payload[k * pitch:k * pitch + tot].cpu().numpy().copy(), tot, pitch


def assert_planes_are_the_flat_calls(pc, data, refs, tag):
    """check 1: plane by plane against the fresh per-plane results; the message names the first differing plane, chunk and byte"""
    for k in range(data.esize):
        clen, payload, total, pitch = result_of(pc, k, data.n)
        ref = refs[k]
        why = ML.first_difference("directory", clen, ref["clen"]) or ML.first_difference("payload", payload, ref["payload"], clen=ref["clen"])
        assert not why and total == ref["payload"].size, "%s plane %d: total %d, per-plane call %d; %s" % (tag, k, total, ref["payload"].size, why)
        behind = pc.payload[k * pitch + total:k * pitch + total + 64].cpu().numpy()
        assert (behind == 0x5A).all(), "%s plane %d: bytes behind the payload" % (tag, k)
        if data.codec in trc.STATIC:
            cdf, status = pc.cdf_of(k)
            assert status == ref["status"] == data.m and np.array_equal(cdf, ref["cdf"]), "%s plane %d: CDF or cdfini status" % (tag, k)
    assert pc.guards_ok(), tag + ": a guard behind the coder's buffers"


def where(got, exp, esize, c, e0=0):
    """the first differing byte of decoded elements as element, plane and chunk"""
    bad = np.flatnonzero(got != exp)
    if not bad.size:
        return ""
    i = int(bad[0])
    e = e0 + i // esize
    return "first difference at byte %d: element %d (chunk %d, element %d of it), plane %d: 0x%02x, expected 0x%02x" % (
        i, e, e // c, e % c, i % esize, int(got[i]), int(exp[i]))


def assert_decodes(torch, pc, data, tag):
    """check 2"""
    n, t = data.n, data.t
    d_out = guarded(torch, n + trc.PAD)
    pc.decode(d_out, n)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], data.d), "%s: decode does not return the input; %s" % (tag, where(out[:n], data.d, data.esize, data.c))
    assert (out[n:] == 0xA5).all(), tag + ": decode wrote behind its n bytes"
    assert np.array_equal(pc.tail[:t].cpu().numpy(), data.d[n - t:]), tag + ": tail bytes"
    assert pc.guards_ok(), tag + ": a guard behind the coder's buffers"


def assert_ranges(torch, pc, data, ranges, tag):
    """check 3"""
    esize, c, m = data.esize, data.c, data.m
    for first, count in ranges:
        e0, e1 = first * c, min(m, (first + count) * c)
        size = (e1 - e0) * esize
        d_out = guarded(torch, size + trc.PAD)
        pc.decode_range(d_out, first, count, data.n)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        exp = data.d[e0 * esize:e1 * esize]
        assert np.array_equal(out[:size], exp), "%s: chunks (%d, %d); %s" % (tag, first, count, where(out[:size], exp, esize, c, e0))
        assert (out[size:] == 0xA5).all(), "%s: chunks (%d, %d) wrote behind their elements" % (tag, first, count)
    assert pc.guards_ok(), tag + ": a guard behind the coder's buffers"


def encode_into(torch, pc, data, tag):
    encode_guarded(torch, pc, data.d, data.n, tag)


_cache = {}
_said = set()


def coded(torch, codec, esize):
    """-> (Data, PlanesCoder holding its container, the per-plane references): once per (coder, esize), shared, left as it is"""
    key = (codec, esize)
    if key not in _cache:
        data = Data(codec, esize, NCH, LAST)
        assert data.m == (NCH - 1) * data.c + LAST
        pc = trc.PlanesCoder(codec, data.n, esize, data.c, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD)
        assert pc.nch == NCH and (4 * NCH) % 8 == 4             # plane 1's directory is 4-byte, not 8-byte aligned
        if key not in _said:
            _said.add(key)
            print("\n[planes matrix] %s esize %d: trc_planes_work_bytes %d (%.1f MB), range workspace for all %d chunks %.1f MB"
                  % (trc.CODEC_NAMES[codec], esize, pc.work_bytes, pc.work_bytes / 1e6, NCH,
                     trc.lib().trc_planes_range_work_bytes(codec, data.n, esize, data.c, NCH) / 1e6))
        encode_into(torch, pc, data, "%s esize %d" % (trc.CODEC_NAMES[codec], esize))
        _cache[key] = (data, pc, reference(torch, data))
    return _cache[key]


def cases(torch, codec):
    for esize in esizes(codec):
        yield ("%s esize %d" % (trc.CODEC_NAMES[codec], esize), esize) + coded(torch, codec, esize)


# ---- checks 1 to 3 ---------------------------------------------------------------------------------------------------------
@by_coder
def test_planes_are_the_flat_calls(torch_cuda, codec):
    """check 1, and the condition on the input: every plane's directory, as the per-plane call wrote it, mixes raw and coded chunks"""
    for tag, esize, data, pc, refs in cases(torch_cuda, codec):
        lens = np.minimum(data.c, data.m - np.arange(0, data.m, data.c))
        for k, ref in enumerate(refs):
            raw, cod = int((ref["clen"] == lens).sum()), int((ref["clen"] < lens).sum())
            print("[planes matrix] %s plane %d: %d raw, %d coded chunks" % (tag, k, raw, cod))
            assert raw >= MIN_EACH and cod >= MIN_EACH and raw + cod == NCH, "%s plane %d: %d raw and %d coded chunks" % (tag, k, raw, cod)
        assert_planes_are_the_flat_calls(pc, data, refs, tag)


@by_coder
def test_round_trip_and_ranges(torch_cuda, codec):
    """checks 2 and 3"""
    torch = torch_cuda
    for tag, esize, data, pc, refs in cases(torch, codec):
        assert_decodes(torch, pc, data, tag)
        assert_ranges(torch, pc, data, RANGES, tag)
        d_out = guarded(torch, 4096)
        pc.decode_range(d_out, 7, 0, data.n)                     # no chunk: TRC_OK, nothing written
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xA5).all(), tag + ": an empty range wrote to its output"


# ---- check 4: a used workspace -------------------------------------------------------------------------------------------------
@by_coder
def test_used_workspace(torch_cuda, codec):
    """the coder sized for 67 chunks codes 3 c + 1 elements per plane (every slice and directory moves), then the 67 chunks again:
    what one call left in the slices, models and group sums does not reach the next"""
    torch = torch_cuda
    for tag, esize, data, pc, refs in cases(torch, codec):
        short = Data(codec, esize, 4, 1, base=500)
        assert short.m == 3 * short.c + 1 and short.c == data.c
        short_refs = reference(torch, short)
        for step, (x, r) in enumerate(((short, short_refs), (data, refs))):
            stag = "%s, %s input in the used workspace" % (tag, ("short", "long")[step])
            encode_into(torch, pc, x, stag)
            assert_planes_are_the_flat_calls(pc, x, r, stag)
            assert_decodes(torch, pc, x, stag)


# ---- check 5: a receiver -------------------------------------------------------------------------------------------------------
@by_coder
def test_receiver_with_a_decode_only_workspace(torch_cuda, codec):
    """a coder that has never encoded, its workspaces full of 0xEE, decodes the first one's directory, payload, tail and CDFs: in
    full and over ranges (what trc_decode_planes_host relies on)"""
    torch = torch_cuda
    for tag, esize, data, pc, refs in cases(torch, codec):
        rx = trc.PlanesCoder(codec, data.n, esize, data.c, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD)
        rx.work[:rx.work_bytes + trc.PAD] = 0xEE
        need = trc.lib().trc_planes_range_work_bytes(codec, data.n, esize, data.c, NCH)
        assert need
        rx.range_work, rx.range_work_bytes = rx._buf(need), need
        rx.range_work[:need + trc.PAD] = 0xEE
        for name in ("clen", "payload", "tail", "cdf"):
            getattr(rx, name).copy_(getattr(pc, name))
        assert_decodes(torch, rx, data, tag + " receiver")
        assert_ranges(torch, rx, data, [(63, 2), (0, 67)], tag + " receiver")
        assert rx.range_work_bytes == need                       # both ranges ran in the workspace that was filled
        del rx


# ---- check 6: filters ----------------------------------------------------------------------------------------------------------
@by_coder
def test_filters(torch_cuda, codec):
    """esize 4: the filtered call on the inverse-filtered join gives the container of the unfiltered call on the join, and decodes"""
    torch = torch_cuda
    esize = 4
    data, pc, refs = coded(torch, codec, esize)
    for filt in FL.FILTERS:
        tag = "%s esize %d filter %s" % (trc.CODEC_NAMES[codec], esize, FL.FILTER_NAMES[filt])
        src = copy.copy(data)                                    # the same planes, reached through the filter
        src.d = FL.inverse(data.d, esize, filt, data.c)
        assert np.array_equal(FL.forward(src.d, esize, filt, data.c), data.d) and not np.array_equal(src.d, data.d)
        fc = trc.FilteredPlanesCoder(codec, data.n, esize, data.c, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, filter=filt)
        encode_into(torch, fc, src, tag)
        ML.assert_same_container(fc, pc, esize, codec, tag)
        assert_planes_are_the_flat_calls(fc, data, refs, tag)
        assert_decodes(torch, fc, src, tag)
        assert_ranges(torch, fc, src, [(63, 2), (66, 1)], tag)
        del fc


# ---- check 7: host containers ----------------------------------------------------------------------------------------------------
@by_coder
def test_host_containers(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    data, pc, refs = coded(torch, codec, esize)
    d, n, t, c = data.d, data.n, data.t, data.c
    tag = "%s esize %d" % (trc.CODEC_NAMES[codec], esize)
    comp = trc.host_encode_planes(codec, d, esize, c, cdfnum=256, prm=PRM)
    trc.planes_check(comp, n)
    hdr, sections, tail = trc.parse_planes(comp)
    assert (hdr["codec"], hdr["esize"], hdr["tail"], hdr["chunk"], hdr["n"], hdr["size"]) == (codec, esize, t, c, n, comp.size)
    assert hdr["cdfnum"] == (256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0)
    assert all(o % 8 == 0 for o in hdr["off"]) and np.array_equal(tail, d[n - t:])
    for k in range(esize):
        cdf, cont = sections[k]
        exp = trc.encode_host_container(codec, data.planes[k], c, cdf=cdf, cdfnum=256, prm=PRM)
        assert np.array_equal(cont, exp), "%s: section %d is not trc_encode_host of plane %d; %s" % (tag, k, k, ML.first_difference("section", cont, exp))
        _, sclen, spay = trc.parse_container(cont)
        assert np.array_equal(sclen, refs[k]["clen"]) and np.array_equal(spay, refs[k]["payload"]), "%s: section %d against the device call" % (tag, k)
        if codec in trc.STATIC:
            assert np.array_equal(cdf, refs[k]["cdf"]), "%s: CDF of section %d" % (tag, k)
    got = trc.host_decode_planes(comp, n)
    assert np.array_equal(got, d), "%s: host decode; %s" % (tag, where(got, d, esize, c))
    for offset, length in ((0, 1), (esize * c - 1, 3), (n - t - 1, t + 1)):
        got = trc.host_decode_planes_range(comp, offset, length)
        assert np.array_equal(got, d[offset:offset + length]), "%s: bytes [%d, +%d)" % (tag, offset, length)
    src = FL.inverse(d, esize, FL.ZDELTA, c)
    fcomp = trc.host_encode_fplanes(codec, FL.ZDELTA, src, esize, c, cdfnum=256, prm=PRM)
    trc.fplanes_check(fcomp, n)
    assert np.array_equal(fcomp[16:], comp), tag + ": bytes [16:] of the filtered container are not the planes container of the filtered input"
    assert np.array_equal(trc.host_decode_xplanes(fcomp, n), src), tag + ": the filtered container through trc_decode_xplanes_host"
    assert np.array_equal(trc.host_decode_xplanes(comp, n), d), tag + ": the planes container through trc_decode_xplanes_host"


@by_coder
def test_host_automatic_chunk(torch_cuda, codec):
    """chunk 0: the coder's automatic chunk, never below its floor"""
    esize = 4
    chunk = max(trc.lib().trc_auto_chunk_codec(codec, AUTO_M), FLOOR.get(codec, 0))
    nch = trc.nchunks(AUTO_M, chunk)
    data = Data(codec, esize, nch, AUTO_M - (nch - 1) * chunk, base=900, chunk=chunk)
    assert data.m == AUTO_M and nch >= 3
    comp = trc.host_encode_planes(codec, data.d, esize, 0, cdfnum=256, prm=PRM)
    hdr, sections, _ = trc.parse_planes(comp)
    assert hdr["chunk"] == chunk and all(trc.parse_container(s)[0]["nchunks"] == nch for _, s in sections)
    trc.planes_check(comp, data.n)
    got = trc.host_decode_planes(comp, data.n)
    assert np.array_equal(got, data.d), "%s: %s" % (trc.CODEC_NAMES[codec], where(got, data.d, esize, chunk))


# ---- check 8: the coders of in[i] & 15 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ML.LOW4, ids=lambda c: trc.CODEC_NAMES[c])
def test_low_nibble_coders_are_refused(torch_cuda, codec):
    """TRC_E_ARG with the reason from all six device calls, nothing launched: every buffer keeps its fill"""
    torch = torch_cuda
    L = trc.lib()
    esize, c = 4, 256
    m = (NCH - 1) * c + LAST
    n = m * esize + esize - 1
    for cls in (trc.PlanesCoder, trc.FilteredPlanesCoder):
        with pytest.raises(trc.TrcError):
            cls(codec, n, esize, c, "cuda:0", prm=PRM)
    wb, rwb = L.trc_planes_work_bytes(trc.RCA, n, esize, c), L.trc_planes_range_work_bytes(trc.RCA, n, esize, c, 2)
    assert wb and rwb
    pitch = trc.planes_pitch(n, esize)
    b = dict(d_in=guarded(torch, n + trc.PAD), d_out=guarded(torch, n + trc.PAD), clen=guarded(torch, 4 * esize * NCH),
             payload=guarded(torch, esize * pitch, fill=0x5A), total=guarded(torch, 8 * esize), tail=guarded(torch, 8),
             work=guarded(torch, wb), rwork=guarded(torch, rwb))
    before = {k: v.clone() for k, v in b.items()}
    p = {k: v.data_ptr() for k, v in b.items()}
    s = torch.cuda.current_stream().cuda_stream
    z = trc.FILTER_ZDELTA

    args = (p["d_in"], n, esize, c, None)
    outs = (None, p["clen"], p["payload"], p["total"], p["tail"], p["work"], wb, s)
    calls = [("trc_encode_planes_dev", lambda cd, cn: L.trc_encode_planes_dev(cd, *args, cn, *outs)),
             ("trc_encode_fplanes_dev", lambda cd, cn: L.trc_encode_fplanes_dev(cd, z, *args, cn, *outs)),
             ("trc_decode_planes_dev", lambda cd, cn: L.trc_decode_planes_dev(cd, p["clen"], p["payload"], p["tail"], n, esize, c, None, cn, p["d_out"], p["work"], wb, s)),
             ("trc_decode_fplanes_dev", lambda cd, cn: L.trc_decode_fplanes_dev(cd, z, p["clen"], p["payload"], p["tail"], n, esize, c, None, cn, p["d_out"], p["work"], wb, s)),
             ("trc_decode_planes_range_dev", lambda cd, cn: L.trc_decode_planes_range_dev(cd, p["clen"], p["payload"], n, esize, c, 63, 2, None, cn, p["d_out"], p["rwork"], rwb, s)),
             ("trc_decode_fplanes_range_dev", lambda cd, cn: L.trc_decode_fplanes_range_dev(cd, z, p["clen"], p["payload"], n, esize, c, 63, 2, None, cn, p["d_out"], p["rwork"], rwb, s))]
    cn = trc.ss_prm(PRM) if codec in trc.SSBIT else 0
    for name, call in calls:                                    # (each is judged before the next is made)
        rc = call(codec, cn)
        why = L.trc_last_error().decode()
        assert rc == -1 and ML.LOW4_TEXT in why and "codec %d" % codec in why, "%s(%s) returned %d: %s" % (name, trc.CODEC_NAMES[codec], rc, why)
    torch.cuda.synchronize()
    for k, v in b.items():
        assert torch.equal(v, before[k]), "a refused call wrote to " + k
    d = PL.weights(m, esize)
    d = np.concatenate([d, d[:esize - 1]])
    with pytest.raises(trc.TrcError, match=ML.LOW4_TEXT):
        trc.host_encode_planes(codec, d, esize, c, prm=PRM)
    with pytest.raises(trc.TrcError, match=ML.LOW4_TEXT):
        trc.host_encode_fplanes(codec, z, d, esize, c, prm=PRM)
    with pytest.raises(trc.TrcError, match=ML.LOW4_TEXT):
        trc.encode_aplanes_host(codec, d, esize, c, prm=PRM)
    # the buffers are sound: the six calls of the coder they were sized for run in them
    done = [(name, call(trc.RCA, 0)) for name, call in calls]
    torch.cuda.synchronize()
    assert all(rc == 0 for _, rc in done), done
    for k in b:
        assert (b[k][-GUARD:] == 0xA5).all().item(), "guard behind " + k
