"""Byte planes on the MI355X: the split / join kernels at the edges of a thread's vector, a wave, a workgroup and the grid-stride
loop; the contract of the planar calls (plane k's directory, payload and total are what trc_encode_dev gives for plane k); chunk
ranges; the TRCP container through host pointers and `trcfile p / d / x`; and what it is for: bf16 weights store fewer bytes as
planes than flat.  Every comparison is byte equality against planes_lib (numpy) or against the existing per-plane calls, and
every device buffer is followed by a 512-byte guard of 0xA5 that must survive (the kernels' buffers have one on both sides).  The
device calls and comparisons shared with the other plane files are in gpu_planes.py."""
import numpy as np
import pytest

import planes_lib as PL
import trc
from gpu_contracts import torch_cuda  # noqa: F401 (the fixture)
from gpu_planes import CHUNK, GUARD, PRM, coded_flat, decodes_flat, decodes_ranges_flat, guarded, split_join_flat, trcfile_round_trip

pytestmark = pytest.mark.gpu
M = 200 * CHUNK + 100                                           # 201 chunks per plane, the last one of 100 bytes
SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4097, 65539]     # elements: around a thread's vector (8), a wave (512), a workgroup (2048) ...
LOOP_M, LOOP_GRID = 65539, 3                                    # ... and 8192 vectors on a grid capped at 3 workgroups: 11 turns of the loop
CODECS = [trc.ANS4S, trc.RCA, trc.RCB, trc.RCSS]
RANGES = [(0, 1), (63, 2), (65, 64), (137, 64), (200, 1), (0, 201)]
NCH = 201


# ---- the two kernels -----------------------------------------------------------------------------------------------------
def split_join_case(torch, esize, m, t):
    d = np.random.default_rng(100 * m + 10 * esize + t).integers(0, 256, m * esize + t, dtype=np.uint8)
    planes, tail = PL.split(d, esize)
    split_join_flat(torch, d, esize, m, t, planes, tail, "esize %d, m %d, t %d" % (esize, m, t))


@pytest.mark.parametrize("esize", PL.ESIZES)
@pytest.mark.parametrize("m", SIZES)
def test_split_join(torch_cuda, esize, m):
    for t in range(esize):
        split_join_case(torch_cuda, esize, m, t)


@pytest.mark.parametrize("esize", PL.ESIZES)
def test_split_join_grid_stride_loop(torch_cuda, esize, monkeypatch):
    monkeypatch.setenv("TRC_PLANES_GRID", str(LOOP_GRID))
    for t in (0, esize - 1):
        split_join_case(torch_cuda, esize, LOOP_M, t)


def test_split_join_argument_errors(torch_cuda):
    torch = torch_cuda
    d_in, d_planes, d_tail = guarded(torch, 4096), guarded(torch, 8 * 1024), guarded(torch, 8)
    for n, esize, pitch, tail in ((4096, 3, 2048, None), (1, 2, 256, d_tail), (4096, 2, 2000, None), (4096, 2, 1792, None), (4097, 2, 2048, None)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_split(d_in, n, esize, d_planes, pitch, tail)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            trc.planes_join(d_planes, pitch, tail, n, esize, d_in)
    with pytest.raises(trc.TrcError, match="rc=-1"):
        trc.planes_split(d_in[8:], 1024, 2, d_planes, 1024, None)      # an input that is not 16-byte aligned
    torch.cuda.synchronize()
    assert (d_planes.cpu().numpy() == 0xA5).all() and (d_in.cpu().numpy() == 0xA5).all()


# ---- the coded calls ---------------------------------------------------------------------------------------------------
def coded(torch, codec, esize):
    """-> (input bytes, PlanesCoder holding their planar container): computed once per (codec, esize), shared, left unchanged"""
    d = PL.mixed_weights(M, esize, CHUNK, esize - 1)
    return d, coded_flat(torch, codec, esize, CHUNK, d)[0]


@pytest.mark.parametrize("esize", (2, 4))
@pytest.mark.parametrize("codec", CODECS)
def test_encode_contract(torch_cuda, codec, esize):
    torch = torch_cuda
    d, pc = coded(torch, codec, esize)
    planes, tail = PL.split(d, esize)
    assert np.array_equal(pc.tail[:esize - 1].cpu().numpy(), tail)
    raw = coded_chunks = 0
    for k in range(esize):
        dc = trc.DeviceCoder(codec, M, CHUNK, "cuda:0")
        d_plane = torch.from_numpy(np.concatenate([planes[k], np.zeros(GUARD, np.uint8)])).to("cuda:0")
        if codec in trc.STATIC:
            dc.cdfini(d_plane, M, 256)
        dc.encode(d_plane, M, prm=PRM)
        exp_clen, exp_payload = dc.result(M)
        clen, payload, total = pc.result(k)
        tag = "%s esize %d plane %d" % (trc.CODEC_NAMES[codec], esize, k)
        assert total == exp_payload.size, tag
        assert np.array_equal(clen, exp_clen), tag + ": directory"
        assert np.array_equal(payload, exp_payload), tag + ": payload"
        assert (pc.payload[k * pc.pitch + total:k * pc.pitch + total + 64].cpu().numpy() == 0x5A).all(), tag + ": bytes behind the payload"
        if codec in trc.STATIC:
            cdf, status = pc.cdf_of(k)
            assert status == M and np.array_equal(cdf, dc.cdf[:257].cpu().numpy().view(np.uint16)), tag + ": CDF"
        lens = np.minimum(CHUNK, M - np.arange(0, M, CHUNK))
        raw += int((clen == lens).sum()); coded_chunks += int((clen < lens).sum())
    assert raw and coded_chunks, "the input is meant to mix raw and coded chunks"
    decodes_flat(torch, pc, d, "%s esize %d" % (trc.CODEC_NAMES[codec], esize))


@pytest.mark.parametrize("esize", (2, 4))
@pytest.mark.parametrize("codec", CODECS)
def test_decode_range(torch_cuda, codec, esize):
    torch = torch_cuda
    d, pc = coded(torch, codec, esize)
    assert pc.nch == NCH
    decodes_ranges_flat(torch, pc, d, esize, CHUNK, RANGES, "%s esize %d" % (trc.CODEC_NAMES[codec], esize))


@pytest.mark.parametrize("codec", (trc.ANS4S, trc.RCA))
def test_argument_errors_launch_nothing(torch_cuda, codec):
    torch = torch_cuda
    esize = 2
    d, pc = coded(torch, codec, esize)
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    d_in = guarded(torch, n + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))
    before = [x.clone() for x in (pc.clen, pc.payload, pc.total, pc.tail, pc.cdf)]
    for first, count in ((NCH, 1), (0, NCH + 1), (100, 102), (NCH + 1, 0)):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.decode_range(d_out, first, count, n)
    for flag in (trc.TABLES_READY, trc.DIR_READY):
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.decode_range(d_out, 0, 1, n, flags=flag)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.decode(d_out, n, flags=flag)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.encode(d_in, n, flags=flag)
    pc.decode_range(d_out, 7, 0, n)                             # count 0: TRC_OK, nothing launched
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all(), "a rejected call wrote to its output"
    for x, b in zip((pc.clen, pc.payload, pc.total, pc.tail, pc.cdf), before):
        assert torch.equal(x, b), "a rejected encode changed the container"


# ---- host pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", (2, 4))
@pytest.mark.parametrize("codec", CODECS)
def test_host_container(torch_cuda, codec, esize):
    d, _ = coded(torch_cuda, codec, esize)
    n, t = d.size, esize - 1
    comp = trc.host_encode_planes(codec, d, esize, CHUNK, cdfnum=256, prm=PRM)
    trc.planes_check(comp, n)
    hdr, sections, tail = trc.parse_planes(comp)
    assert (hdr["codec"], hdr["esize"], hdr["tail"], hdr["chunk"], hdr["n"], hdr["size"]) == (codec, esize, t, CHUNK, n, comp.size)
    assert hdr["cdfnum"] == (256 if codec in trc.STATIC else trc.ss_prm(PRM) if codec in trc.SSBIT else 0)
    assert all(o % 8 == 0 for o in hdr["off"]) and np.array_equal(tail, d[n - t:])
    planes, _ = PL.split(d, esize)
    for k in range(esize):
        cdf, cont = sections[k]
        exp = trc.encode_host_container(codec, planes[k], CHUNK, cdf=cdf, cdfnum=256, prm=PRM)
        assert np.array_equal(cont, exp), "%s esize %d: section %d is not trc_encode_host of plane %d" % (trc.CODEC_NAMES[codec], esize, k, k)
        if codec in trc.STATIC:
            _, ref_cdf, _ = trc.host_cdfini(planes[k], 256)
            assert np.array_equal(cdf, ref_cdf[:257])
    assert np.array_equal(trc.host_decode_planes(comp, n), d)
    for offset, length in ((0, 1), (esize * CHUNK - 1, 3), (n - t - 1, t + 1), (0, n)):
        got = trc.host_decode_planes_range(comp, offset, length)
        assert np.array_equal(got, d[offset:offset + length]), "%s esize %d: bytes [%d, +%d)" % (trc.CODEC_NAMES[codec], esize, offset, length)
    with pytest.raises(trc.TrcError):
        trc.host_decode_planes_range(comp, n - 1, 2)
    with pytest.raises(trc.TrcError, match="container"):
        trc.host_decode_planes(comp[:-1], n)


def test_host_automatic_chunk(torch_cuda):
    d, _ = coded(torch_cuda, trc.RCA, 4)
    comp = trc.host_encode_planes(trc.RCA, d, 4, 0)
    hdr, _, _ = trc.parse_planes(comp)
    assert hdr["chunk"] == trc.lib().trc_auto_chunk_codec(trc.RCA, d.size // 4)
    trc.planes_check(comp, d.size)
    assert np.array_equal(trc.host_decode_planes(comp, d.size), d)
    assert np.array_equal(trc.host_decode_planes_range(comp, 4 * hdr["chunk"] - 2, 7), d[4 * hdr["chunk"] - 2:4 * hdr["chunk"] + 5])


def test_trcfile_planes(torch_cuda, tmp_path):
    d, _ = coded(torch_cuda, trc.RCA, 2)
    comp = trcfile_round_trip(tmp_path, d, "trcp", ["p", "46", "2"], 2 * CHUNK - 1, 1000)
    assert comp[:4].tobytes() == b"TRCP"


# ---- what it is for --------------------------------------------------------------------------------------------------------
def test_bf16_weights_store_fewer_bytes_as_planes(torch_cuda):
    """256 KiB of bf16 N(0, 0.02^2) weights through rccdf at chunk 4096: order-0 entropy 6.21 bits per byte flat, 5.32 as two planes
    (14 % less), so payload + directory of the planar form is strictly smaller"""
    torch = torch_cuda
    n, chunk = 256 * 1024, 4096
    d = PL.weights(n // 2, 2)
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(GUARD, np.uint8)])).to("cuda:0")
    dc = trc.DeviceCoder(trc.RCA, n, chunk, "cuda:0")
    dc.encode(d_in, n)
    clen, payload = dc.result(n)
    flat = payload.size + 4 * clen.size
    pc = trc.PlanesCoder(trc.RCA, n, 2, chunk, "cuda:0", guard=GUARD)
    pc.encode(d_in, n)
    planar = sum(pc.result(k)[2] + 4 * pc.nch for k in range(2))
    print("flat %d bytes, planar %d bytes (%.1f %% less)" % (flat, planar, 100.0 * (flat - planar) / flat))
    assert planar < flat
    d_out = guarded(torch, n + trc.PAD)
    pc.decode(d_out, n)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:n], d) and pc.guards_ok()
