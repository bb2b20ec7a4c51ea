"""Random-access decode on the MI355X: trc_decode_range_dev for one coder of every decode launcher (slices of a directory that
mixes raw and coded chunks, ranges that start and end anywhere in a 64-chunk group, TRC_DIR_READY), the index across the scan
kernel's loop, a payload at an odd-word offset, argument errors, trc_decode_range_host and `trcfile x`.  Expected bytes are
slices of the input: nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import trc
import trc_testlib as T
import nibbit_lib as NL
import sweep_lib as S
from gpu_contracts import to_dev, torch_cuda  # noqa: F401 (torch_cuda: the fixture)
from planes_matrix_lib import chunk_of, mixed_input  # noqa: F401 (the generator, shared with test_gpu_planes_matrix.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 512
NCHUNKS = 201                                                  # 200 chunks and a final one of TAIL bytes
TAIL = 100
RANGES = [(0, 1), (1, 1), (63, 1), (63, 2), (64, 64), (65, 64), (1, 128), (137, 64), (200, 1), (0, 201)]
# one coder per decode launcher of csrc/trc_launch.h, all four static coders; the smallest chunk its existing GPU tests use
CODECS = [trc.ANS4S, trc.RCS1, trc.RCS2, trc.RCSM, trc.RCB, trc.RCA, trc.RCAI, trc.RCA4, trc.RCV8, trc.ANSA, trc.ANSO1, trc.ANSB,
          trc.VLCU16, trc.VLAU16, trc.RCC1, trc.RCG16, trc.RCR32, trc.RCBVZ16, trc.RCW16, trc.RC4, trc.RCU3]
NIBBLE = (trc.RCA4, trc.RC4)                                   # values 0..15 in, never stored raw: 4 bits per byte at the worst


def make_input(codec):
    """chunks alternate between uniform and skewed data of the coder's kind -> (n, chunk, bytes)"""
    return mixed_input(codec, NCHUNKS, TAIL)


def encoded(torch, codec, n, chunk, d):
    """-> (DeviceCoder holding the container, directory, what a full decode returns)"""
    dc = trc.DeviceCoder(codec, n, chunk, "cuda:0")
    d_in = to_dev(torch, d)
    if codec in trc.STATIC:
        dc.cdfini(d_in, n, 256)
    dc.encode(d_in, n)
    clen, _ = dc.result(n)
    d_out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    dc.decode(d_out, n)
    torch.cuda.synchronize()
    full = d_out.cpu().numpy()
    assert (full[n:] == 0xA5).all()
    return dc, clen, full[:n].copy()


def check_ranges(torch, dc, full, n, chunk, ranges, dir_ready, tag):
    size = max(min(n, (f + c) * chunk) - f * chunk for f, c in ranges)
    d_out = torch.empty(size + GUARD, dtype=torch.uint8, device="cuda:0")
    for first, count in ranges:
        nb = min(n, (first + count) * chunk) - first * chunk
        d_out.fill_(0xA5)
        dc.decode_range(d_out, first, count, n, dir_ready=dir_ready)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:nb], full[first * chunk:first * chunk + nb]), tag + (first, count, dir_ready)
        assert (out[nb:nb + GUARD] == 0xA5).all(), tag + (first, count, dir_ready, "guard")


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: trc.CODEC_NAMES[c])
def test_slices(torch_cuda, codec):
    torch = torch_cuda
    n, chunk, d = make_input(codec)
    dc, clen, full = encoded(torch, codec, n, chunk, d)
    lens = S.chunk_lens(n, chunk)
    assert clen.size == NCHUNKS and len(set(clen.tolist())) >= 4          # irregular offsets
    if codec not in NIBBLE:
        assert int((clen == lens).sum()) >= 50 and int((clen < lens).sum()) >= 50, "the directory must mix raw and coded chunks"
    assert np.array_equal(full, NL.expected(codec, d, clen, chunk) if codec == trc.RC4 else d)
    tag = (trc.CODEC_NAMES[codec],)
    check_ranges(torch, dc, full, n, chunk, RANGES, False, tag)
    assert dc.range_work_bytes == trc.range_work_bytes(codec, n, chunk, NCHUNKS)
    check_ranges(torch, dc, full, n, chunk, RANGES[::-1], True, tag)     # the index of the last call serves every range


def test_group_boundaries_of_the_index(torch_cuda):
    """70 000 chunks: 1094 groups, so the scan kernel takes a second trip and goff crosses its 1024-group boundary"""
    torch = torch_cuda
    codec, chunk, nch = trc.ANS4S, 256, 70000
    n = nch * chunk
    d = np.where((np.arange(n) // chunk) % 3 == 0, T.uniform_bytes(n, 8), T.nibble_bytes(n, 9, "geo")).astype(np.uint8)
    dc, clen, full = encoded(torch, codec, n, chunk, d)
    assert np.array_equal(full, d) and int((clen == chunk).sum()) > 20000
    first = min(8191 * 64 - 1, nch)                                # clipped to the directory: it ends far below, nothing is left
    ranges = [(65535, 130), (69999, 1), (first, min(66, nch - first))]
    assert ranges[2] == (nch, 0)                                   # ... and an empty range is TRC_OK and writes nothing
    check_ranges(torch, dc, full, n, chunk, ranges, False, ("index",))
    check_ranges(torch, dc, full, n, chunk, ranges[::-1], True, ("index",))


def test_payload_offset(torch_cuda):
    """the payload at offset 6 of a 256-byte aligned allocation: the alignment promise of include/trc_hip.h"""
    torch = torch_cuda
    codec = trc.RCA
    n, chunk, d = make_input(codec)
    dc, clen, full = encoded(torch, codec, n, chunk, d)
    buf = torch.zeros(n + trc.PAD + 64 + 256, dtype=torch.uint8, device="cuda:0")
    base = (buf.data_ptr() + 255) & ~255
    shifted = buf[base - buf.data_ptr() + 6:]
    assert shifted.data_ptr() % 16 == 6
    shifted[:n + trc.PAD].copy_(dc.payload[:n + trc.PAD])
    dc.payload = shifted
    check_ranges(torch, dc, full, n, chunk, RANGES, False, ("offset6",))


def test_argument_errors(torch_cuda):
    """refused before anything is launched"""
    torch = torch_cuda
    lib = trc.lib()
    codec = trc.RCA
    n, chunk, d = make_input(codec)
    dc, clen, full = encoded(torch, codec, n, chunk, d)
    wb = trc.range_work_bytes(codec, n, chunk, 64)
    work = torch.zeros(wb + 512, dtype=torch.uint8, device="cuda:0")
    w = (work.data_ptr() + 255) & ~255
    out = torch.full((64 * chunk + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    o = (out.data_ptr() + 15) & ~15
    TRC_E_ARG, TRC_E_WORK = -1, -3
    args = (dc.clen.data_ptr(), dc.payload.data_ptr(), n, chunk)
    assert lib.trc_decode_range_dev(codec, *args, 138, 64, None, 0, o, w, wb, None) == TRC_E_ARG          # 138 + 64 > 201
    assert lib.trc_decode_range_dev(codec, *args, 202, 0, None, 0, o, w, wb, None) == TRC_E_ARG
    assert lib.trc_decode_range_dev(codec, *args, 64, 64, None, 0, o + 8, w, wb, None) == TRC_E_ARG        # d_out misaligned by 8
    assert lib.trc_decode_range_dev(codec, *args, 64, 64, None, 0, o, w, wb - 1, None) == TRC_E_WORK
    assert lib.trc_decode_range_dev(codec, *args, 64, 0, None, 0, o, w, 0, None) == 0                      # count == 0: nothing to do
    torch.cuda.synchronize()
    assert (out == 0xA5).all().item() and not work.any().item()


@pytest.mark.parametrize("chunk", [0, 256], ids=["auto", "chunk256"])
@pytest.mark.parametrize("codec", [trc.ANS4S, trc.RCA, trc.RCB], ids=lambda c: trc.CODEC_NAMES[c])
def test_host_pointers(torch_cuda, codec, chunk):
    lib = trc.lib()
    n = 1000007
    d = T.text_bytes(n, 7)
    _, cdf, cdfnum = T.orc_cdfini(d) if codec == trc.ANS4S else (0, None, 256)
    prev = lib.trc_get_chunk()
    assert lib.trc_set_chunk(chunk) == 0
    try:
        comp = trc.host_encode(codec, d, cdf, cdfnum)
    finally:
        lib.trc_set_chunk(prev)
    assert comp.size < n
    ch = trc.parse_container(comp)[0]["chunk"]
    assert ch == (chunk or lib.trc_auto_chunk_codec(codec, n))
    for off, ln in ((0, 1), (ch - 1, 2), (12345, 100000), (n - 1, 1), (0, n)):
        got = trc.host_decode_range(codec, comp, n, off, ln, cdf, cdfnum)
        assert np.array_equal(got, d[off:off + ln]), (off, ln)
        plan = trc.container_range(comp, off, ln)
        assert plan["first_chunk"] == off // ch and plan["out_skip"] == off % ch
    with pytest.raises(trc.TrcError):
        trc.host_decode_range(codec, comp, n, n - 5, 6, cdf, cdfnum)


def test_host_range_of_a_raw_stream(torch_cuda):
    """an incompressible input: the encoder returns n, the range is a copy"""
    n = 1000007
    d = T.uniform_bytes(n, 3)
    comp = trc.host_encode(trc.RCA, d)
    assert comp.size == n
    for off, ln in ((0, 1), (4095, 2), (12345, 100000), (n - 1, 1), (0, n)):
        assert np.array_equal(trc.host_decode_range(trc.RCA, comp, n, off, ln), d[off:off + ln]), (off, ln)


def test_trcfile_extract(torch_cuda, tmp_path):
    """trcfile c, then trcfile x in a child process: a slice of a 1 MB file, static (CDF in the file) and adaptive"""
    exe = os.path.join(ROOT, "harness", "trcfile")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    n = 1000003
    d = T.text_bytes(n, 4)
    src = tmp_path / "in.bin"
    src.write_bytes(d.tobytes())
    for fid, (off, ln) in ((46, (123457, 54321)), (65, (n - 4097, 4097))):
        comp, out = tmp_path / ("c%d.trcf" % fid), tmp_path / ("x%d.bin" % fid)
        r = subprocess.run([exe, "c", str(fid), str(src), str(comp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert os.path.getsize(comp) < n
        r = subprocess.run([exe, "x", str(comp), str(off), str(ln), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert out.read_bytes() == d[off:off + ln].tobytes(), fid
    r = subprocess.run([exe, "x", str(comp), str(n - 1), "2", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "range" in r.stderr
