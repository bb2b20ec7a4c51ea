#!/usr/bin/env python3
"""Times the TRCB container calls on the GPU, on the two batches of about 100 MB of scripts/measure_abatch.py (values from N(0, 1),
TRC_RCA, chunk 4096):
  many-large : 400 bf16 items of 131 072 elements
  many-small : 25 600 fp32 items of 1 024 elements
  pack          trc_planes_batch_pack_dev on the coded batch (front upload + kernel)
  d2d           hipMemcpyAsync, device to device, of the container's `size` bytes: the memory-bound yardstick
  host_dev      trc_encode_planes_batch_host, device items (encode + pack + one copy of `size` bytes to pageable memory)
  host_host     the same with host items (gathered through the page-locked staging slots)
  planes_host   trc_encode_planes_host on the materialised virtual buffer V of the same batch, in pageable host memory
  h2d_per_item  one pageable hipMemcpyAsync per item and a synchronise: what host_host's gather avoids
Every figure is a host clock around calls that end in a device synchronise, per repetition, after a warm-up of the same calls; the
variants take turns within a round and the rounds' minimum, median and maximum are reported.  Also printed: the container's size
against PlanesBatchCoder.stored_bytes().  Not a test and not part of bench.py.

    python scripts/measure_container.py [--rounds 5] [--variants pack,d2d] [--out FILE] [--small]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import planes_batch_lib as BL  # noqa: E402
import trc  # noqa: E402

CHUNK = 4096
CODEC = trc.RCA
VARIANTS = ("pack", "d2d", "host_dev", "host_host", "planes_host", "h2d_per_item")
BATCHES = {"many-large": (torch.bfloat16, 400, 131072), "many-small": (torch.float32, 25600, 1024)}


def hip_runtime():
    """the HIP runtime this process already uses (torch's)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    sys.exit("measure_container: no HIP runtime is loaded")


class Batch:
    def __init__(self, dtype, count, m):
        self.count, self.m = count, m
        g = torch.Generator(device="cuda:0").manual_seed(count)
        self.vals = torch.randn(count, m, generator=g, device="cuda:0").to(dtype)
        self.esize = self.vals.element_size()
        self.n = m * self.esize
        self.tensors = [self.vals[i] for i in range(count)]
        self.host = [t.view(torch.uint8).cpu().numpy() for t in self.tensors]
        self.bc = trc.PlanesBatchCoder(CODEC, self.tensors, CHUNK)
        self.bc.encode()
        self.cont, self.size = self.bc.pack()
        self.copy = torch.empty(self.size, dtype=torch.uint8, device="cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.hip = hip_runtime()
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.v = BL.virtual(self.host, self.esize, CHUNK)
        self.flat = np.concatenate(self.host)
        self.d_flat = torch.empty(self.flat.size, dtype=torch.uint8, device="cuda:0")

    def pack(self):
        bc, st = self.bc, False
        trc._chk(trc.lib().trc_planes_batch_pack_dev(bc.codec, bc.items, bc.filters, bc.count, bc.esize, bc.chunk, None, bc.cdfnum, None,
                                                     bc.clen.data_ptr(), bc.payload.data_ptr(), bc.total.data_ptr(), bc.packed.data_ptr(),
                                                     bc.packed.numel(), self.d_size.data_ptr(), self.stream))

    def d2d(self):
        assert self.hip.hipMemcpyAsync(self.copy.data_ptr(), self.cont.data_ptr(), self.size, 3, self.stream) == 0

    def host_dev(self):
        self.out = trc.host_encode_planes_batch(CODEC, self.tensors, self.esize, CHUNK)

    def host_host(self):
        self.out = trc.host_encode_planes_batch(CODEC, self.host, self.esize, CHUNK)

    def planes_host(self):
        self.ref = trc.host_encode_planes(CODEC, self.v, self.esize, CHUNK)

    def h2d_per_item(self):
        base, src, n, f, s = self.d_flat.data_ptr(), self.flat.ctypes.data, self.n, self.hip.hipMemcpyAsync, self.stream
        for i in range(self.count):
            f(base + i * n, src + i * n, n, 1, s)


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a hundredth of the items: a rehearsal of the script, not a measurement")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated, of: " + " ".join(VARIANTS))
    a = ap.parse_args()
    want = a.variants.split(",")
    if not torch.cuda.is_available():
        sys.exit("measure_container: no GPU; there is nothing to measure without one")
    lines = []
    for name, (dtype, count, m) in BATCHES.items():
        b = Batch(dtype, count // 100 if a.small else count, m)
        b.d_size = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        # the calls must agree before any is timed
        b.host_dev()
        got = b.out
        b.host_host()
        b.planes_host()
        inner = trc.parse_planes_batch(got)["inner"]
        assert np.array_equal(got, b.out) and np.array_equal(got, b.cont.cpu().numpy()) and np.array_equal(got[inner:], b.ref), name
        stored = b.bc.stored_bytes()
        lines.append(dict(batch=name, items=b.count, esize=b.esize, elements=b.m, MB=round(b.count * b.n / 1e6, 1), chunk=CHUNK,
                          container_bytes=b.size, stored_bytes=stored, beyond_stored=b.size - stored, payload_buffer_bytes=b.esize * b.bc.pitch,
                          virtual_MB=round(b.v.size / 1e6, 1)))
        print(json.dumps(lines[-1]), flush=True)
        variants = []
        for v in VARIANTS:
            if v not in want:
                continue
            fn = getattr(b, v)
            timed(fn, 2)                                          # warm-up, then as many repetitions as fill about 0.3 s
            variants.append((v, fn, max(2, min(500, int(0.3 / timed(fn, 2)) + 1))))
        times = {v: [] for v, _, _ in variants}
        for _ in range(a.rounds):
            for v, fn, reps in variants:
                times[v].append(timed(fn, reps))
        for v, _, reps in variants:
            ts = sorted(times[v])
            moved = b.size if v in ("pack", "d2d") else b.count * b.n
            lines.append(dict(batch=name, variant=v, reps=reps, rounds=a.rounds, ms_min=round(1e3 * ts[0], 4),
                              ms_median=round(1e3 * statistics.median(ts), 4), ms_max=round(1e3 * ts[-1], 4),
                              bytes=moved, GBps_median=round(moved / 1e9 / statistics.median(ts), 1)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
