#!/usr/bin/env python3
"""Times the batched split, join and histogram kernels with a predictor order per item on the GPU, on the two batches of
scripts/measure_sbatch.py, about 100 MB each at chunk 4096,
  many-large : 400 bf16 items of 131 072 elements (normal-distributed values)
  many-small : 25 600 u32 items of 1 024 elements -- 256 rows of 4 fields (sorted id, two timestamps, a counter) each
for every operation at the uniform orders 2 and 3 at the strides 1, 2 and 8 and under the mixed orders (1, 2, 3, 1, ..) at stride 1,
each against
  sbatch   the same batch at the same stride behind the zigzag delta: trc_planes_split_sbatch_dev / _join_sbatch_dev /
           trc_planes_hist_sbatch_dev, the parent commit's kernels and the order-1 cost that the ordered kernels extend,
  obatch_ones  the ordered calls with order 1 everywhere at that stride, which launch those same kernels, and
  flat     trc_planes_split_ofilter_dev / _join_ofilter_dev / trc_planes_hist_order_dev at the same (order, stride), and at order 1, on
           ONE contiguous buffer of the same bytes: the single-buffer cost of the same arithmetic.
Every item takes the zigzag delta; the filter histogram counts all three filters, the order histogram all four orders.

A figure is the time between two events on the stream around `reps` calls, divided by reps, after a warm-up of the same calls that
also brings the clocks up; a batched call holds its table upload (32 bytes per item, host to device) and the map kernel, as it does
for a caller.  The variants take turns within a round; the rounds' minimum, median and maximum are reported.  Not a test and not part
of bench.py.  One JSON line per (batch, operation, variant); --out also writes them to a file.

    python scripts/measure_obatch.py [--rounds 7] [--out FILE] [--small] [--ops split,join,hist] [--variants REGEX]"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import measure_sbatch as MS  # noqa: E402
import trc  # noqa: E402

CHUNK = MS.CHUNK
STRIDES = (1, 2, 8)
ORDERS = (2, 3)


class Batch(MS.Batch):
    """the batch of measure_sbatch.py with the ordered calls and the order histograms"""

    def __init__(self, esize, count, m):
        MS.Batch.__init__(self, esize, count, m)
        self.ohist = torch.empty(trc.planes_hist_obatch_bytes(count, esize), dtype=torch.uint8, device="cuda:0")
        self.ohist_one = torch.empty(trc.planes_hist_order_bytes(esize), dtype=torch.uint8, device="cuda:0")

    def orders(self, k):
        return trc.planes_orders([1 + i % 3 for i in range(self.count)] if k == "mixed" else k, self.count)

    def osplit(self, st, od):
        trc._chk(trc.lib().trc_planes_split_obatch_dev(self.items, self.filters, st, od, self.count, self.esize, CHUNK, self.planes.data_ptr(), self.pitch,
                                                       self.table.data_ptr(), self.tb, self.stream))

    def ojoin(self, st, od):
        trc._chk(trc.lib().trc_planes_join_obatch_dev(self.planes.data_ptr(), self.pitch, self.items_out, self.filters, st, od, self.count, 0, self.count,
                                                      self.esize, CHUNK, self.table.data_ptr(), self.tb, self.stream))

    def ohist_(self, st, od):
        trc._chk(trc.lib().trc_planes_hist_obatch_dev(15, self.items, st, self.count, 0, self.count, self.esize, CHUNK, self.ohist.data_ptr(),
                                                      self.table.data_ptr(), self.tb, self.stream))

    def flat_osplit(self, k, s):
        trc._chk(trc.lib().trc_planes_split_ofilter_dev(k, s, self.flat.data_ptr(), self.total, self.esize, CHUNK, self.flat_planes.data_ptr(),
                                                        self.flat_pitch, None, self.stream))

    def flat_ojoin(self, k, s):
        trc._chk(trc.lib().trc_planes_join_ofilter_dev(k, s, self.flat_planes.data_ptr(), self.flat_pitch, None, self.total, self.esize, CHUNK,
                                                       self.flat_out.data_ptr(), self.stream))

    def flat_ohist(self, k, s):
        trc._chk(trc.lib().trc_planes_hist_order_dev(15, s, self.flat.data_ptr(), self.total, self.esize, CHUNK, self.ohist_one.data_ptr(), self.stream))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a hundredth of the items: a rehearsal of the script, not a measurement")
    ap.add_argument("--ops", default="split,join,hist")
    ap.add_argument("--variants", default="", help="time only the variants whose name matches this regular expression")
    ap.add_argument("--fill", type=float, default=0.2, help="seconds of work per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_obatch: no GPU; there is nothing to measure without one")
    lines = []
    for name, (esize, count, m) in MS.BATCHES.items():
        b = Batch(esize, count // 100 if a.small else count, m)
        for k in ORDERS + ("mixed",):                          # a round trip at every assignment before anything is timed
            for s in STRIDES if k != "mixed" else (1, "mixed"):
                st, od = b.strides(s), b.orders(k)
                b.osplit(st, od)
                b.out.zero_()
                b.ojoin(st, od)
                torch.cuda.synchronize()
                assert torch.equal(b.out, b.buf), "%s order %s stride %s: join(split(x)) != x" % (name, k, s)
        ops = (("split", b.split, b.osplit, b.flat_osplit), ("join", b.join, b.ojoin, b.flat_ojoin), ("hist", b.hist_, b.ohist_, b.flat_ohist))
        for op, sbatched, obatched, flat in ops:
            if op not in a.ops.split(","):
                continue
            if op == "join":                                   # planes that belong to the predictor being undone do not matter for the time
                b.split(b.strides(1))
                b.flat_split(1)
            variants = []
            for s in STRIDES:
                variants.append(("sbatch_s%d" % s, lambda f=sbatched, st=b.strides(s): f(st)))
                variants.append(("obatch_ones_s%d" % s, lambda f=obatched, st=b.strides(s), od=b.orders(1): f(st, od)))
                variants.append(("flat_o1_s%d" % s, lambda f=flat, s=s: f(1, s)))
                for k in ORDERS if op != "hist" else (3,):     # (the order histogram counts all four orders whatever the items' orders are)
                    variants.append(("obatch_o%d_s%d" % (k, s), lambda f=obatched, st=b.strides(s), od=b.orders(k): f(st, od)))
                    variants.append(("flat_o%d_s%d" % (k, s), lambda f=flat, k=k, s=s: f(k, s)))
            if op != "hist":
                variants.append(("obatch_mixed_s1", lambda f=obatched, st=b.strides(1), od=b.orders("mixed"): f(st, od)))
                variants.append(("obatch_mixed_smixed", lambda f=obatched, st=b.strides("mixed"), od=b.orders("mixed"): f(st, od)))
            variants = [(v, fn) for v, fn in variants if re.search(a.variants, v)]
            sized = []
            for v, fn in variants:
                MS.timed(fn, 3)                                # warm-up, then as many repetitions as fill the window
                sized.append((v, fn, max(3, min(300, int(a.fill / MS.timed(fn, 3)) + 1))))
            times = {v: [] for v, _, _ in sized}
            for _ in range(a.rounds):
                for v, fn, reps in sized:
                    times[v].append(MS.timed(fn, reps))
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
