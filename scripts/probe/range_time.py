"""What a range decode costs (profiles/range/range_notes.md): 100 MB of text at chunk 4096, ANS4S and RCA.
Device: HIP-event time of trc_decode_range_dev for 64 and 4096 chunks from the middle, without and with TRC_DIR_READY, and of a
full trc_decode_dev, each the median of REPS calls after one warm-up call, every value kept.  Host pointers: wall time of
trc_decode_range_host for 1 MB from the middle against trc_decode_host of the whole container (pageable numpy buffers).
Every output is compared with the input.  usage: range_time.py <out.jsonl>"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "turbo-range-coder_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import trc
import trc_testlib as T

N, CHUNK, REPS = 100 * 1000 * 1000, 4096, 9


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(round(a.elapsed_time(b), 4))
    return {"median_ms": float(np.median(ms)), "all_ms": ms}


def main(path):
    d = T.text_bytes(N, 7)
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
    nch = trc.nchunks(N, CHUNK)
    rows = []
    for codec in (trc.ANS4S, trc.RCA):
        name = trc.CODEC_NAMES[codec]
        dc = trc.DeviceCoder(codec, N, CHUNK, "cuda:0")
        if codec in trc.STATIC:
            dc.cdfini(d_in, N, 256)
        dc.encode(d_in, N)
        clen, payload = dc.result(N)
        d_out = torch.zeros(N + 512, dtype=torch.uint8, device="cuda:0")
        for ready in (False, True):
            r = timed(lambda: dc.decode(d_out, N, dir_ready=ready))
            assert np.array_equal(d_out[:N].cpu().numpy(), d)
            rows.append(dict(what="trc_decode_dev", codec=name, n=N, chunk=CHUNK, chunks=nch, dir_ready=ready, **r))
        for count in (64, 4096):
            first = (nch - count) // 2 | 1                          # inside a 64-chunk group of the full directory
            nb = count * CHUNK
            for ready in (False, True):
                d_out.zero_()
                r = timed(lambda: dc.decode_range(d_out, first, count, N, dir_ready=ready))
                assert np.array_equal(d_out[:nb].cpu().numpy(), d[first * CHUNK:first * CHUNK + nb])
                rows.append(dict(what="trc_decode_range_dev", codec=name, n=N, chunk=CHUNK, first=first, chunks=count, bytes=nb,
                                 dir_ready=ready, work_bytes=trc.range_work_bytes(codec, N, CHUNK, count),
                                 full_work_bytes=dc.work_bytes, **r))
        # host pointers: the automatic chunk, pageable buffers
        cdf = dc.cdf[:257].cpu().numpy().view(np.uint16).copy() if codec in trc.STATIC else None
        comp = trc.host_encode(codec, d, cdf, 256)
        lib = trc.lib()
        lib.trc_decode_host.restype = C.c_size_t
        lib.trc_decode_host.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint]
        out = np.zeros(N + 64, np.uint8)
        pc = cdf.ctypes.data if cdf is not None else None
        off, ln = N // 2 + 12345, 1 << 20
        for what, call, nbytes in (("trc_decode_host", lambda: lib.trc_decode_host(codec, comp.ctypes.data, comp.size, out.ctypes.data, N, pc, 256 if pc else 0), N),
                                   ("trc_decode_range_host", lambda: lib.trc_decode_range_host(codec, comp.ctypes.data, comp.size, N, off, ln, out.ctypes.data, pc, 256 if pc else 0), ln)):
            assert call() == nbytes
            ms = []
            for _ in range(REPS):
                t0 = time.perf_counter(); got = call(); ms.append(round((time.perf_counter() - t0) * 1e3, 4))
                assert got == nbytes
            assert np.array_equal(out[:nbytes], d[off:off + ln] if nbytes == ln else d)
            rows.append(dict(what=what, codec=name, n=N, chunk=trc.parse_container(comp)[0]["chunk"], container_bytes=int(comp.size),
                             bytes=nbytes, median_ms=float(np.median(ms)), all_ms=ms))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main(sys.argv[1])
