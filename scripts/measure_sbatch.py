#!/usr/bin/env python3
"""Times the batched split, join and histogram kernels with a stride per item on the GPU, on two batches of about 100 MB at chunk 4096,
  many-large : 400 bf16 items of 131 072 elements (normal-distributed values)
  many-small : 25 600 u32 items of 1 024 elements -- 256 rows of 4 fields (sorted id, two timestamps, a counter) each
for every operation at the uniform strides 2, 4 and 8 and under the mixed assignment (1, 2, .. 8, 1, ..), each against
  fbatch   the same batch at stride 1: the trc_fplanes_*_batch_kernel / trc_planes_hist_batch_kernel code objects, which
           scripts/compare_isa.py shows to be the parent commit's instruction for instruction, and
  flat     the unbatched trc_planes_split_sfilter_dev / trc_planes_join_sfilter_dev / trc_planes_hist_stride_dev at the same stride
           (and at stride 1) on ONE contiguous buffer of the same bytes.
Every item takes the zigzag delta; the histogram counts all three filters.

A figure is the time between two events on the stream around `reps` calls, divided by reps, after a warm-up of the same calls that
also brings the clocks up; a batched call holds its table upload (32 bytes per item, host to device) and the map kernel, as it does
for a caller.  The variants take turns within a round; the rounds' minimum, median and maximum are reported.  Not a test and not part
of bench.py.  One JSON line per (batch, operation, variant); --out also writes them to a file.

    python scripts/measure_sbatch.py [--rounds 7] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))

import torch  # noqa: E402

import trc  # noqa: E402

CHUNK = 4096
STRIDES = (2, 4, 8)
BATCHES = {"many-large": (2, 400, 131072), "many-small": (4, 25600, 1024)}


class Batch:
    """`count` items of m elements, 256 bytes apart at least, in one allocation; the same bytes as one buffer with TRC_PAD behind it"""

    def __init__(self, esize, count, m):
        self.esize, self.count, self.m, self.n = esize, count, m, m * esize
        g = torch.Generator(device="cuda:0").manual_seed(count)
        if esize == 2:
            vals = torch.randn(count, m, generator=g, device="cuda:0").to(torch.bfloat16)
        else:                                                  # rows of (id, t0, t1, counter)
            rows = m // 4
            steps = torch.stack([torch.randint(1, 40, (count, rows), generator=g, device="cuda:0"), torch.randint(0, 3, (count, rows), generator=g, device="cuda:0"),
                                 torch.randint(0, 3, (count, rows), generator=g, device="cuda:0"), torch.randint(0, 2, (count, rows), generator=g, device="cuda:0")], dim=2)
            base = torch.tensor([100000, 1700000000, 1700000400, 0], device="cuda:0")
            vals = (torch.cumsum(steps, dim=1) + base).to(torch.int32).reshape(count, m)
        vals = vals.contiguous().view(torch.uint8).reshape(count, self.n)
        self.pitch_item = (self.n + 255 + 16) & ~255
        self.buf = torch.zeros(count * self.pitch_item, dtype=torch.uint8, device="cuda:0")
        self.buf.view(count, self.pitch_item)[:, :self.n] = vals
        self.out = torch.zeros_like(self.buf)
        self.flat = torch.cat([vals.reshape(-1), torch.zeros(trc.PAD, dtype=torch.uint8, device="cuda:0")])
        self.flat_out = torch.zeros_like(self.flat)
        self.total = count * self.n
        self.items = trc.planes_items([(self.buf.data_ptr() + i * self.pitch_item, self.n) for i in range(count)])
        self.items_out = trc.planes_items([(self.out.data_ptr() + i * self.pitch_item, self.n) for i in range(count)])
        self.plan, _ = trc.planes_batch_plan(self.items, count, esize, CHUNK)
        L = trc.lib()
        self.tb = L.trc_planes_batch_table_bytes(count, self.plan["chunks"])
        self.table = torch.empty(self.tb, dtype=torch.uint8, device="cuda:0")
        self.pitch = self.plan["pitch"]
        self.planes = torch.zeros(esize * self.pitch, dtype=torch.uint8, device="cuda:0")
        self.flat_pitch = trc.planes_pitch(self.total, esize)
        self.flat_planes = torch.zeros(esize * self.flat_pitch, dtype=torch.uint8, device="cuda:0")
        self.hist = torch.empty(trc.planes_hist_batch_bytes(count, esize), dtype=torch.uint8, device="cuda:0")
        self.hist_one = torch.empty(trc.planes_hist_bytes(esize), dtype=torch.uint8, device="cuda:0")
        self.filters = trc.planes_filters(trc.FILTER_ZDELTA, count)
        self.stream = torch.cuda.current_stream().cuda_stream

    def strides(self, s):
        return trc.planes_strides([1 + i % 8 for i in range(self.count)] if s == "mixed" else s, self.count)

    def split(self, st):
        trc._chk(trc.lib().trc_planes_split_sbatch_dev(self.items, self.filters, st, self.count, self.esize, CHUNK, self.planes.data_ptr(), self.pitch,
                                                       self.table.data_ptr(), self.tb, self.stream))

    def join(self, st):
        trc._chk(trc.lib().trc_planes_join_sbatch_dev(self.planes.data_ptr(), self.pitch, self.items_out, self.filters, st, self.count, 0, self.count,
                                                      self.esize, CHUNK, self.table.data_ptr(), self.tb, self.stream))

    def hist_(self, st):
        trc._chk(trc.lib().trc_planes_hist_sbatch_dev(7, self.items, st, self.count, 0, self.count, self.esize, CHUNK, self.hist.data_ptr(),
                                                      self.table.data_ptr(), self.tb, self.stream))

    def flat_split(self, s):
        trc._chk(trc.lib().trc_planes_split_sfilter_dev(trc.FILTER_ZDELTA, s, self.flat.data_ptr(), self.total, self.esize, CHUNK,
                                                        self.flat_planes.data_ptr(), self.flat_pitch, None, self.stream))

    def flat_join(self, s):
        trc._chk(trc.lib().trc_planes_join_sfilter_dev(trc.FILTER_ZDELTA, s, self.flat_planes.data_ptr(), self.flat_pitch, None, self.total, self.esize,
                                                       CHUNK, self.flat_out.data_ptr(), self.stream))

    def flat_hist(self, s):
        trc._chk(trc.lib().trc_planes_hist_stride_dev(7, s, self.flat.data_ptr(), self.total, self.esize, CHUNK, self.hist_one.data_ptr(), self.stream))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a hundredth of the items: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_sbatch: no GPU; there is nothing to measure without one")
    lines = []
    for name, (esize, count, m) in BATCHES.items():
        b = Batch(esize, count // 100 if a.small else count, m)
        for s in STRIDES + ("mixed",):                         # a round trip at every assignment before anything is timed
            st = b.strides(s)
            b.split(st)
            b.out.zero_()
            b.join(st)
            torch.cuda.synchronize()
            assert torch.equal(b.out, b.buf), "%s stride %s: join(split(x)) != x" % (name, s)
        for op, batched, flat in (("split", b.split, b.flat_split), ("join", b.join, b.flat_join), ("hist", b.hist_, b.flat_hist)):
            if op == "join":                                   # planes that belong to the stride being joined do not matter for the time
                b.split(b.strides(1))
                b.flat_split(1)
            variants = [("fbatch", lambda batched=batched: batched(None))]
            for s in STRIDES + ("mixed",):
                variants.append(("sbatch_%s" % s, lambda batched=batched, st=b.strides(s): batched(st)))
            for s in (1,) + STRIDES:
                variants.append(("flat_%d" % s, lambda flat=flat, s=s: flat(s)))
            sized = []
            for v, fn in variants:
                timed(fn, 3)                                   # warm-up, then as many repetitions as fill about 0.2 s
                sized.append((v, fn, max(3, min(300, int(0.2 / timed(fn, 3)) + 1))))
            times = {v: [] for v, _, _ in sized}
            for _ in range(a.rounds):
                for v, fn, reps in sized:
                    times[v].append(timed(fn, reps))
            mb = b.total / 1e6
            for v, _, reps in sized:
                ts = sorted(times[v])
                lines.append(dict(batch=name, items=b.count, esize=esize, elements=m, MB=round(mb, 1), chunk=CHUNK, op=op, variant=v, reps=reps,
                                  rounds=a.rounds, ms_min=round(1e3 * ts[0], 4), ms_median=round(1e3 * statistics.median(ts), 4),
                                  ms_max=round(1e3 * ts[-1], 4), GBps_median=round(mb / 1e3 / statistics.median(ts), 1)))
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
