#!/usr/bin/env python3
"""Times the calls that put a batch coded against bases into one piece, each against its sibling, on 100 MB of weights next to bases
that differ by small noise, as 400 bf16 items of 125 000 elements and as 25 600 fp32 items of 1024 elements:
  fingerprint   trc_base_fingerprint_batch_dev over all bases against trc_base_fingerprint_dev over the same bytes as ONE buffer and
                against one trc_base_fingerprint_dev per item
  hist          trc_planes_hist_bbatch_dev(7) against trc_planes_hist_batch_dev(7) on the same items
  pack          trc_planes_bbatch_pack_dev against trc_planes_batch_pack_dev on the same coded batch (the difference is the fingerprint)
Items and bases each lie in one allocation, item after item; 100 MB fits the Infinity Cache, so these are sibling comparisons and
not HBM figures.

A figure is the time between two events on the stream around `reps` calls, divided by reps, after a warm-up of the same calls.  The
batched calls upload their table inside the call, which the figure includes.  The variants take turns within a round; the rounds'
minimum, median and maximum are reported.  Not a test and not part of bench.py.  One JSON line per (shape, operation, variant);
--out also writes them to a file.

    python scripts/measure_bbatch_container.py [--rounds 7] [--out FILE] [--small]"""
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
SHAPES = {"400x_bf16": (400, 125000, torch.bfloat16), "25600x_fp32": (25600, 1024, torch.float32)}
SMALL = {"40x_bf16": (40, 12800, torch.bfloat16), "256x_fp32": (256, 1024, torch.float32)}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps                  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1 MB instead of 100 MB: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L = trc.lib()
    lines = []
    for name, (count, m, dt) in (SMALL if args.small else SHAPES).items():
        esize = torch.empty(0, dtype=dt).element_size()
        n = m * esize
        assert n % 16 == 0
        g = torch.Generator(device="cuda:0").manual_seed(esize)
        w = torch.randn(count * m, generator=g, device="cuda:0", dtype=torch.float32) * 0.02
        base = w.to(dt).view(torch.uint8)
        data = (w + torch.randn(count * m, generator=g, device="cuda:0", dtype=torch.float32) * 1e-4).to(dt).view(torch.uint8)
        items = [data[i * n:(i + 1) * n] for i in range(count)]
        bases = [base[i * n:(i + 1) * n] for i in range(count)]
        it = trc.planes_items([(t.data_ptr(), n) for t in items])
        bs = trc.planes_bases(bases, count)
        fl = trc.planes_filters(trc.FILTER_ZDELTA, count)
        stream = torch.cuda.current_stream().cuda_stream
        # fingerprint
        tb = L.trc_base_fingerprint_batch_table_bytes(count)
        table = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
        fps = torch.zeros(8 * count, dtype=torch.uint8, device="cuda:0")
        fp1 = torch.zeros(8 * count, dtype=torch.uint8, device="cuda:0")

        def per_item():
            for i in range(count):
                L.trc_base_fingerprint_dev(bases[i].data_ptr(), n, fp1.data_ptr() + 8 * i, stream)
        # hist
        plan, _ = trc.planes_batch_plan(it, count, esize, CHUNK)
        htb = L.trc_planes_batch_table_bytes(count, plan["chunks"])
        htable = torch.empty(htb, dtype=torch.uint8, device="cuda:0")
        hist = torch.empty(trc.planes_hist_batch_bytes(count, esize), dtype=torch.uint8, device="cuda:0")
        # pack: one coded batch, both containers
        bc = trc.BasePlanesBatchCoder(trc.RCA, [t.view(dt) for t in items], CHUNK, filters=trc.FILTER_ZDELTA, bases=bases)
        bc.encode()
        bound = L.trc_planes_bbatch_bound(bc.codec, bc.items, count, esize, CHUNK, bc.cdfnum)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
        d_size = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        coded = (count, esize, CHUNK, None, bc.cdfnum, None, bc.clen.data_ptr(), bc.payload.data_ptr(), bc.total.data_ptr(), out.data_ptr(), bound, d_size.data_ptr())
        ops = {
            "fingerprint": {"batch": lambda: trc._chk(L.trc_base_fingerprint_batch_dev(it, bs, fl, count, 0, count, fps.data_ptr(), table.data_ptr(), tb, stream)),
                            "single_whole_buffer": lambda: trc._chk(L.trc_base_fingerprint_dev(base.data_ptr(), count * n, fp1.data_ptr(), stream)),
                            "single_per_item": per_item},
            "hist": {"batch_pred": lambda: trc._chk(L.trc_planes_hist_batch_dev(7, it, count, 0, count, esize, CHUNK, hist.data_ptr(), htable.data_ptr(), htb, stream)),
                     "bbatch_base": lambda: trc._chk(L.trc_planes_hist_bbatch_dev(7, it, bs, count, 0, count, esize, CHUNK, hist.data_ptr(), htable.data_ptr(), htb, stream))},
            "pack": {"batch_TRCB": lambda: trc._chk(L.trc_planes_batch_pack_dev(bc.codec, bc.items, fl, *coded, stream)),
                     "bbatch_TRCE": lambda: trc._chk(L.trc_planes_bbatch_pack_dev(bc.codec, bc.items, bs, fl, *coded, table.data_ptr(), tb, stream))},
        }
        # the values first: the batch's fingerprints are the per-item calls'
        ops["fingerprint"]["batch"]()
        per_item()
        torch.cuda.synchronize()
        assert torch.equal(fps, fp1), "the batched fingerprints differ from the per-item calls'"
        for op, variants in ops.items():
            reps = {v: max(2, args.reps // 10) if v == "single_per_item" else args.reps for v in variants}
            for v, fn in variants.items():                    # warm-up: code objects, clocks
                timed(fn, reps[v])
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v, fn in variants.items():
                    times[v].append(timed(fn, reps[v]))
            for v, t in times.items():
                med = statistics.median(t)
                line = {"shape": name, "items": count, "esize": esize, "bytes": count * n, "op": op, "variant": v, "us_min": round(min(t), 2),
                        "us_median": round(med, 2), "us_max": round(max(t), 2), "rounds": args.rounds, "reps": reps[v]}
                if op == "pack":                               # (what this variant writes, from a call of its own)
                    variants[v]()
                    line["container_bytes"] = int(d_size.item())
                print(json.dumps(line), flush=True)
                lines.append(line)
        del bc, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
