#!/usr/bin/env python3
"""Times the batch advisor's kernel on the GPU: trc_planes_hist_batch_dev(7, ...) on two batches of about 100 MB at chunk 4096,
  many-large : 400 bf16 items of 131 072 elements
  many-small : 25 600 fp32 items of 1 024 elements
each against (a) the loop a caller writes without it -- one trc_planes_hist_dev per item into a histogram of its own, the items
having TRC_PAD of slack behind them -- and (b) trc_planes_split_fbatch_dev over the same items (zigzag delta on every item), the
memory-bound yardstick.  Two more lines take the batched call apart: trc_planes_hist_dev on the same bytes as ONE buffer (the
batched kernel's counting without its per-item flushes) and the zeroing of the histograms alone.

Every figure is a host clock around calls that end in a device synchronise, per repetition, after a warm-up of the same calls;
the variants take turns within a round and the rounds' minimum, median and maximum are reported.  (a) is driven from Python through
ctypes like everything else here: it is launch bound, and a C caller saves the interpreter's share of each call, not the launches.
Not a test and not part of bench.py.  One JSON line per (batch, variant); --out also writes them to a file.

    python scripts/measure_abatch.py [--rounds 5] [--variants hist_batch,split_fbatch] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))

import torch  # noqa: E402

import trc  # noqa: E402

CHUNK = 4096
VARIANTS = ("hist_batch", "hist_loop", "split_fbatch", "hist_one_buffer", "zero_only")
BATCHES = {"many-large": (torch.bfloat16, 400, 131072), "many-small": (torch.float32, 25600, 1024)}


def up256(x):
    return (x + 255) & ~255


class Batch:
    """`count` items of m elements of normal-distributed values (weights), each followed by TRC_PAD of slack, in one allocation"""

    def __init__(self, dtype, count, m):
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.count, self.m, self.n = count, m, m * self.esize
        self.stride = up256(self.n + trc.PAD)
        self.buf = torch.zeros(count * self.stride, dtype=torch.uint8, device="cuda:0")
        g = torch.Generator(device="cuda:0").manual_seed(count)
        vals = torch.randn(count, m, generator=g, device="cuda:0").to(dtype).view(torch.uint8).reshape(count, self.n)
        self.buf.view(count, self.stride)[:, :self.n] = vals
        self.flat = vals.reshape(-1).contiguous()                 # the same bytes as one buffer
        self.flat = torch.cat([self.flat, torch.zeros(trc.PAD, dtype=torch.uint8, device="cuda:0")])
        base = self.buf.data_ptr()
        self.ptrs = [base + i * self.stride for i in range(count)]
        self.items = trc.planes_items([(p, self.n) for p in self.ptrs])
        self.plan, _ = trc.planes_batch_plan(self.items, count, self.esize, CHUNK)
        L = trc.lib()
        self.tb = L.trc_planes_batch_table_bytes(count, self.plan["chunks"])
        self.table = torch.empty(self.tb, dtype=torch.uint8, device="cuda:0")
        self.hist = torch.empty(trc.planes_hist_batch_bytes(count, self.esize), dtype=torch.uint8, device="cuda:0")
        self.hist_one = torch.empty(trc.planes_hist_bytes(self.esize), dtype=torch.uint8, device="cuda:0")
        self.planes = torch.empty(self.esize * self.plan["pitch"], dtype=torch.uint8, device="cuda:0")
        self.filters = trc.planes_filters(trc.FILTER_ZDELTA, count)
        self.stream = torch.cuda.current_stream().cuda_stream

    def batched(self):
        trc._chk(trc.lib().trc_planes_hist_batch_dev(7, self.items, self.count, 0, self.count, self.esize, CHUNK, self.hist.data_ptr(),
                                                     self.table.data_ptr(), self.tb, self.stream))

    def zero(self):
        """what the batched call spends before its kernel starts counting: the histograms zeroed on the stream"""
        self.hist.zero_()

    def loop(self):
        call, hb, h0 = trc.lib().trc_planes_hist_dev, trc.planes_hist_bytes(self.esize), self.hist.data_ptr()
        for i, p in enumerate(self.ptrs):
            if call(7, p, self.n, self.esize, CHUNK, h0 + i * hb, self.stream):
                raise trc.TrcError(trc.lib().trc_last_error().decode())

    def split(self):
        trc._chk(trc.lib().trc_planes_split_fbatch_dev(self.items, self.filters, self.count, self.esize, CHUNK, self.planes.data_ptr(),
                                                       self.plan["pitch"], self.table.data_ptr(), self.tb, self.stream))

    def one_buffer(self):
        trc._chk(trc.lib().trc_planes_hist_dev(7, self.flat.data_ptr(), self.count * self.n, self.esize, CHUNK, self.hist_one.data_ptr(), self.stream))


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
        sys.exit("measure_abatch: no GPU; there is nothing to measure without one")
    lines = []
    for name, (dtype, count, m) in BATCHES.items():
        b = Batch(dtype, count // 100 if a.small else count, m)
        if "hist_batch" in want and "hist_loop" in want:          # the two must agree before either is timed
            b.batched()
            got = b.hist.clone()
            b.hist.fill_(0xA5)
            b.loop()
            torch.cuda.synchronize()
            assert torch.equal(got, b.hist), name + ": the batched call and the loop disagree"
        variants = []
        for v, fn in (("hist_batch", b.batched), ("hist_loop", b.loop), ("split_fbatch", b.split), ("hist_one_buffer", b.one_buffer),
                      ("zero_only", b.zero)):
            if v not in want:
                continue
            timed(fn, 2)                                          # warm-up, then as many repetitions as fill about 0.3 s
            variants.append((v, fn, max(2, min(500, int(0.3 / timed(fn, 2)) + 1))))
        times = {v: [] for v, _, _ in variants}
        for _ in range(a.rounds):
            for v, fn, reps in variants:
                times[v].append(timed(fn, reps))
        mb = b.count * b.n / 1e6
        for v, _, reps in variants:
            ts = sorted(times[v])
            lines.append(dict(batch=name, items=b.count, esize=b.esize, elements=b.m, MB=round(mb, 1), chunk=CHUNK, variant=v, reps=reps,
                              rounds=a.rounds, ms_min=round(1e3 * ts[0], 4), ms_median=round(1e3 * statistics.median(ts), 4),
                              ms_max=round(1e3 * ts[-1], 4), GBps_median=round(mb / 1e3 / statistics.median(ts), 1)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
