"""Filtered byte planes on the MI355X.  The whole contract is fplanes(filter, ..., in) == planes(..., F(filter, chunk, esize, in)) with F
the numpy model of fplanes_lib, so every comparison is byte equality: the two kernels alone against the model at the edges of a
vector, a tile, a restart segment and the grid; the coded calls against the unfiltered calls on the model-filtered input; chunk
ranges; argument errors; the TRCF container through host pointers and `trcfile f / d / x`; and what it is for: sorted ids store
fewer bytes.  Every device buffer is followed by a 512-byte guard of 0xA5 that must survive."""
import os
import subprocess

import numpy as np
import pytest

import fplanes_lib as FL
import planes_lib as PL
import trc
from planes_matrix_lib import assert_same_container

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 512
SEGS = (256, 320, 4096, 65536)
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
PRM = (4, 7)
CHUNK = 256
M6 = 5 * CHUNK + 3                                              # 6 chunks per plane, the last one of 3 elements


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def guarded(torch, nbytes, data=None):
    """a device buffer of nbytes (from `data`, else 0xA5 throughout) followed by the guard"""
    a = np.full(nbytes + GUARD, 0xA5, dtype=np.uint8)
    if data is not None:
        a[:nbytes] = data
    return torch.from_numpy(a).to("cuda:0")


def up256(x):
    return (x + 255) & ~255


def sizes(seg):
    """elements: one, around a thread's vector, around a restart, several segments and a ragged end, and (small segments) more
    segments than one workgroup has waves"""
    return [1, 7, 8, 9, seg - 1, seg, seg + 1, 3 * seg + 5] + ([64 * seg + 8] if seg <= 320 else [])


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, filt, seg, m, t, kind):
    n = m * esize + t
    d = FL.gen(kind, esize, m, t, 100 * m + 10 * esize + t)
    planes, tail = PL.split(FL.forward(d, esize, filt, seg), esize)
    pitch = up256(m)                                            # the smallest pitch the call takes
    d_in = guarded(torch, n, d)
    d_planes = guarded(torch, esize * pitch)
    d_tail = guarded(torch, 8)
    trc.planes_split_filter(filt, d_in, n, esize, seg, d_planes, pitch, d_tail if t else None)
    d_out = guarded(torch, n)
    trc.planes_join_filter(filt, d_planes, pitch, d_tail if t else None, n, esize, seg, d_out)
    torch.cuda.synchronize()
    tag = "esize %d, filter %s, seg %d, m %d, t %d, %s" % (esize, FL.FILTER_NAMES[filt], seg, m, t, kind)
    exp = np.full(esize * pitch + GUARD, 0xA5, dtype=np.uint8)
    for k in range(esize):
        exp[k * pitch:k * pitch + m] = planes[k]
    got = d_planes.cpu().numpy()
    assert np.array_equal(got, exp), tag + ": planes or the bytes behind them (first difference at %d)" % int(np.flatnonzero(got != exp)[0])
    exp_tail = np.full(8 + GUARD, 0xA5, dtype=np.uint8)
    exp_tail[:t] = tail
    assert np.array_equal(d_tail.cpu().numpy(), exp_tail), tag + ": tail or the bytes behind it"
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], d), tag + ": join(split(x)) != x (first difference at byte %d)" % int(np.flatnonzero(out[:n] != d)[0])
    assert (out[n:] == 0xA5).all(), tag + ": join wrote behind its output"
    assert np.array_equal(d_in.cpu().numpy()[:n], d) and (d_in.cpu().numpy()[n:] == 0xA5).all()


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("esize", FL.ESIZES)
def test_split_join(torch_cuda, esize, filt, seg):
    for i, m in enumerate(sizes(seg)):
        for t in (0, esize - 1):
            split_join_case(torch_cuda, esize, filt, seg, m, t, FL.KINDS[(i + (t > 0)) % 4])


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_split_join_grid_capped(torch_cuda, esize, monkeypatch):
    """one workgroup = 4 waves: the split's loop turns 9 and 19 times; the join's waves take 2 or 3 of the 9 spans of 8 segments
    of 256 (4 tiles each; the 65th segment is a span of its own), 3 or 4 of the 13 spans of 5 segments of 320 + 5 elements, and 2 or
    3 of the 10 segments of 4096 (8 tiles each)"""
    monkeypatch.setenv("TRC_PLANES_GRID", "1")
    for filt in FL.FILTERS:
        split_join_case(torch_cuda, esize, filt, 256, 64 * 256 + 8, esize - 1, "wrap")
        split_join_case(torch_cuda, esize, filt, 320, 100 * 320 + 5, 0, "walk")
        split_join_case(torch_cuda, esize, filt, 4096, 9 * 4096 + 5, esize - 1, "monotone")


@pytest.mark.parametrize("esize", FL.ESIZES)
def test_largest_input(torch_cuda, esize):
    """2^20 elements: every workgroup of the split's full grid at esize 2 upwards, 16 segments of 65536 with 128 tiles each"""
    split_join_case(torch_cuda, esize, FL.ZDELTA, 65536, 1 << 20, 0, "walk")
    split_join_case(torch_cuda, esize, FL.XOR, 256, (1 << 20) - 3, esize - 1, "monotone")


def test_filter_none_is_the_unfiltered_kernel(torch_cuda):
    torch = torch_cuda
    esize, m, t = 4, 1000, 3
    n = m * esize + t
    d = FL.gen("random", esize, m, t, 1)
    planes, tail = PL.split(d, esize)
    d_in, d_planes, d_tail, d_out = guarded(torch, n, d), guarded(torch, esize * 1024), guarded(torch, 8), guarded(torch, n)
    trc.planes_split_filter(trc.FILTER_NONE, d_in, n, esize, 256, d_planes, 1024, d_tail)
    trc.planes_join_filter(trc.FILTER_NONE, d_planes, 1024, d_tail, n, esize, 256, d_out)
    torch.cuda.synchronize()
    got = d_planes.cpu().numpy()
    for k in range(esize):
        assert np.array_equal(got[k * 1024:k * 1024 + m], planes[k]) and (got[k * 1024 + m:(k + 1) * 1024] == 0xA5).all()
    assert np.array_equal(d_tail.cpu().numpy()[:t], tail)
    assert np.array_equal(d_out.cpu().numpy()[:n], d) and (d_out.cpu().numpy()[n:] == 0xA5).all()


def test_split_join_argument_errors(torch_cuda):
    torch = torch_cuda
    d_in, d_planes, d_tail = guarded(torch, 4096), guarded(torch, 8 * 1024), guarded(torch, 8)
    bad = [(f, 4096, 2, 256, 2048, None) for f in (-1, 3)]                                     # the filter
    bad += [(f, 4096, 2, seg, 2048, None) for f in (0, 1, 2) for seg in (100, 128, 65600, 0)]   # the restart length
    bad += [(1, 4096, 3, 256, 2048, None), (2, 1, 2, 256, 256, d_tail), (1, 3, 4, 256, 256, d_tail)]      # esize 3, no whole element
    bad += [(1, 4096, 2, 256, 2000, None), (1, 4096, 2, 256, 1792, None), (2, 4097, 2, 256, 2048, None)]  # pitch, a tail without a buffer
    for filt, n, esize, seg, pitch, tail in bad:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split_filter(filt, d_in, n, esize, seg, d_planes, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join_filter(filt, d_planes, pitch, tail, n, esize, seg, d_in)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_split_filter(1, d_in[8:], 1024, 2, 256, d_planes, 1024, None)              # an input that is not 16-byte aligned
    torch.cuda.synchronize()
    assert (d_planes.cpu().numpy() == 0xA5).all() and (d_in.cpu().numpy() == 0xA5).all() and (d_tail.cpu().numpy() == 0xA5).all()


# ---- the coded calls ---------------------------------------------------------------------------------------------------
_cache = {}


def coded(torch, codec, esize, filt, chunk=CHUNK, m=M6):
    """-> (input bytes, FilteredPlanesCoder holding their container, PlanesCoder holding the container of the model-filtered input):
    computed once per key, shared, left unchanged"""
    key = (codec, esize, filt, chunk, m)
    if key not in _cache:
        t = esize - 1
        d = FL.gen("monotone" if esize > 2 else "walk", esize, m, t, 17 * esize + filt)
        n = d.size
        out = []
        for cls, src, kw in ((trc.FilteredPlanesCoder, d, dict(filter=filt)), (trc.PlanesCoder, FL.forward(d, esize, filt, chunk), {})):
            pc = cls(codec, n, esize, chunk, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, **kw)
            d_in = guarded(torch, n + trc.PAD, np.concatenate([src, np.zeros(trc.PAD, np.uint8)]))
            pc.payload[:esize * pc.pitch] = 0x5A
            pc.encode(d_in, n)
            assert pc.guards_ok(), "encode wrote behind one of its buffers"
            got = d_in.cpu().numpy()
            assert np.array_equal(got[:n], src) and (got[n + trc.PAD:] == 0xA5).all()
            out.append(pc)
        _cache[key] = (d, out[0], out[1])
    return _cache[key]


def assert_decodes(torch, fc, d, tag):
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    fc.decode(d_out, n)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], d), tag + ": decode does not return the input"
    assert (out[n:] == 0xA5).all(), tag + ": decode wrote behind its n bytes"
    assert fc.guards_ok()


@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract_and_every_range(torch_cuda, codec, filt):
    torch = torch_cuda
    esize = 4
    d, fc, pc = coded(torch, codec, esize, filt)
    tag = "%s filter %s" % (trc.CODEC_NAMES[codec], FL.FILTER_NAMES[filt])
    assert fc.nch == 6
    assert_same_container(fc, pc, esize, codec, tag)
    assert_decodes(torch, fc, d, tag)
    n = d.size
    for first in range(6):
        for count in range(1, 6 - first + 1):
            e0, e1 = first * CHUNK, min(M6, (first + count) * CHUNK)
            size = (e1 - e0) * esize
            d_out = guarded(torch, size + trc.PAD)
            fc.decode_range(d_out, first, count, n)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:size], d[e0 * esize:e1 * esize]), "%s: chunks (%d, %d)" % (tag, first, count)
            assert (out[size:] == 0xA5).all(), "%s: chunks (%d, %d) wrote behind their elements" % (tag, first, count)
    assert fc.guards_ok()


@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("esize,codec", [(2, trc.RCA), (8, trc.ANS4S)])
def test_encode_contract_other_widths(torch_cuda, esize, codec, filt):
    torch = torch_cuda
    chunk, m = 4096, 2 * 4096 + 77
    d, fc, pc = coded(torch, codec, esize, filt, chunk, m)
    tag = "%s esize %d filter %s" % (trc.CODEC_NAMES[codec], esize, FL.FILTER_NAMES[filt])
    assert_same_container(fc, pc, esize, codec, tag)
    assert_decodes(torch, fc, d, tag)
    d_out = guarded(torch, (m - chunk) * esize + trc.PAD)
    fc.decode_range(d_out, 1, 2, d.size)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:(m - chunk) * esize], d[chunk * esize:m * esize]) and (out[(m - chunk) * esize:] == 0xA5).all()


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_filter_none_is_the_unfiltered_call(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d = FL.gen("monotone", esize, M6, esize - 1, 3)
    n = d.size
    fc = trc.FilteredPlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    assert fc.filter == trc.FILTER_NONE
    pc = trc.PlanesCoder(codec, n, esize, CHUNK, "cuda:0", cdfnum=256, guard=GUARD)
    d_in = guarded(torch, n + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
    for c in (fc, pc):
        c.payload[:esize * c.pitch] = 0x5A
        c.encode(d_in, n)
    assert_same_container(fc, pc, esize, codec, trc.CODEC_NAMES[codec] + " filter none")
    for name in ("clen", "total", "tail", "cdf", "status"):
        assert torch.equal(getattr(fc, name), getattr(pc, name)), name
    assert_decodes(torch, fc, d, "filter none")
    d_out = guarded(torch, 2 * CHUNK * esize + trc.PAD)
    fc.decode_range(d_out, 2, 2, n)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:2 * CHUNK * esize], d[2 * CHUNK * esize:4 * CHUNK * esize])


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize = 4
    d, fc, _ = coded(torch, codec, esize, FL.ZDELTA)
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    d_in = guarded(torch, n + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
    names = ("clen", "payload", "total", "tail", "cdf")
    before = [getattr(fc, x).clone() for x in names]

    def rejected(nbytes=n, flags=0, **attrs):
        """the three calls with some of the coder's attributes replaced: each is TRC_E_ARG"""
        saved = {k: getattr(fc, k) for k in attrs}
        for k, v in attrs.items():
            setattr(fc, k, v)
        try:
            with pytest.raises(trc.TrcError, match="rc=-1"):
                fc.encode(d_in, nbytes, flags=flags)
            with pytest.raises(trc.TrcError, match="rc=-1"):
                fc.decode(d_out, nbytes, flags=flags)
            with pytest.raises(trc.TrcError, match="rc=-1"):
                fc.decode_range(d_out, 0, 1, nbytes, flags=flags)
        finally:
            for k, v in saved.items():
                setattr(fc, k, v)

    for filt in (-1, 3):
        rejected(filter=filt)
    for chunk in (100, 128, 65600):
        rejected(chunk=chunk)
    for flag in (trc.TABLES_READY, trc.DIR_READY):
        rejected(flags=flag)
    rejected(esize=3)
    rejected(nbytes=esize - 1)                                  # m == 0
    for first, count in ((6, 1), (0, 7), (3, 4)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            fc.decode_range(d_out, first, count, n)
    fc.decode_range(d_out, 2, 0, n)                             # count 0: TRC_OK, nothing launched
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its output"
    for x, b in zip(names, before):
        assert torch.equal(getattr(fc, x), b), "a rejected encode changed the container"
    assert fc.guards_ok()


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (256, 0))
@pytest.mark.parametrize("filt", FL.FILTERS)
@pytest.mark.parametrize("codec", (trc.RCA, trc.ANS4S))
def test_host_container(torch_cuda, codec, filt, chunk):
    esize, m = 4, 9 * 256 + 3
    t = esize - 1
    d = FL.gen("monotone", esize, m, t, 23)
    n = d.size
    comp = trc.host_encode_fplanes(codec, filt, d, esize, chunk)
    trc.fplanes_check(comp, n)
    assert comp[:4].tobytes() == b"TRCF" and (comp[4], comp[5], comp[6], comp[7]) == (filt, 1, 0, 0)
    assert int(comp[8:16].view("<u8")[0]) == comp.size
    hdr, _, tail = trc.parse_planes(comp[16:])
    resolved = hdr["chunk"]
    assert resolved == (chunk or trc.lib().trc_auto_chunk_codec(codec, m)) and hdr["size"] == comp.size - 16 and hdr["n"] == n
    exp = trc.host_encode_planes(codec, FL.forward(d, esize, filt, resolved), esize, chunk)
    assert np.array_equal(comp[16:], exp), "bytes [16:] are not trc_encode_planes_host of the filtered input"
    assert np.array_equal(tail, d[n - t:])
    assert np.array_equal(trc.host_decode_fplanes(comp, n), d)
    c = resolved * esize
    ranges = [(0, 1), (c - 1, 3), (c // 2, 2 * c), (5, n - 5), (n - t - 1, t + 1), (n - t, t), (n - 1, 1), (0, n)]
    for offset, length in ranges:
        if offset + length > n:
            continue
        got = trc.host_decode_fplanes_range(comp, offset, length)
        assert np.array_equal(got, d[offset:offset + length]), "bytes [%d, +%d)" % (offset, length)
    with pytest.raises(trc.TrcError):
        trc.host_decode_fplanes_range(comp, n - 1, 2)
    with pytest.raises(trc.TrcError, match="container"):
        trc.host_decode_fplanes(comp[:-1], n)
    with pytest.raises(trc.TrcError, match="filter 0"):
        trc.host_encode_fplanes(codec, trc.FILTER_NONE, d, esize, chunk)


def test_sorted_ids_store_fewer_bytes_with_zdelta(torch_cuda):
    """1 MiB of sorted 32-bit ids (2^18 draws from [0, 2^32), sorted: neighbours differ by 2^14 on average) through rccdf at the
    automatic chunk: order-0 entropy 7.75 bits per byte as planes, 3.1 behind the zigzag delta"""
    m = 1 << 18
    ids = np.sort(np.random.default_rng(7).integers(0, 1 << 32, m, dtype=np.uint64)).astype("<u4")
    d = ids.view(np.uint8)
    plain = trc.host_encode_planes(trc.RCA, d, 4, 0)
    filtered = trc.host_encode_fplanes(trc.RCA, trc.FILTER_ZDELTA, d, 4, 0)
    xored = trc.host_encode_fplanes(trc.RCA, trc.FILTER_XOR, d, 4, 0)
    print("sorted u32 ids, %d bytes: planes %d, zigzag delta + planes %d, xor + planes %d" % (d.size, plain.size, filtered.size, xored.size))
    assert filtered.size < plain.size
    assert np.array_equal(trc.host_decode_fplanes(filtered, d.size), d)


def test_trcfile_fplanes(torch_cuda, tmp_path):
    exe = os.path.join(ROOT, "harness", "trcfile")
    assert os.path.exists(exe), "harness/trcfile is not built"
    d = FL.gen("monotone", 4, 40000, 3, 9)
    src, comp, back, part = (str(tmp_path / f) for f in ("in.bin", "in.trcf", "out.bin", "part.bin"))
    d.tofile(src)
    for letter, filt in (("z", 1), ("x", 2)):
        for args in (["f", "46", "4", letter, src, comp], ["d", comp, back], ["x", comp, "70001", "3000", part]):
            r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (args, r.stdout, r.stderr)
        head = np.fromfile(comp, dtype=np.uint8)
        assert head[:4].tobytes() == b"TRCF" and head[4] == filt and head[16:20].tobytes() == b"TRCP"
        assert np.array_equal(np.fromfile(back, dtype=np.uint8), d)
        assert np.array_equal(np.fromfile(part, dtype=np.uint8), d[70001:73001])
    r = subprocess.run([exe, "f", "46", "4", "q", src, comp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "filter" in r.stderr
