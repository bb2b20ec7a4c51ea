#!/usr/bin/env python3
"""Times the split, join, histogram and fingerprint kernels of the planes calls AGAINST A BASE on the GPU, on 100 MB of bf16, fp32
and fp64 weights with a base that differs by small noise, each against its sibling that takes no base:
  split / join      trc_planes_split_base_dev / trc_planes_join_base_dev (zigzag delta and xor; the join also in place, out == base)
                    against trc_planes_split_dev / trc_planes_join_dev and the predecessor filter's pair at seg 4096
  hist              trc_planes_hist_base_dev(7) against trc_planes_hist_dev(7, seg 4096)
  fingerprint       trc_base_fingerprint_dev over the same bytes
A base call reads n bytes more than its sibling (the base), so at equal bandwidth a split or join that moves 2n bytes becomes one
that moves 3n.

A figure is the time between two events on the stream around `reps` calls, divided by reps, after a warm-up of the same calls that
also brings the clocks up.  The variants take turns within a round; the rounds' minimum, median and maximum are reported.  Not a test
and not part of bench.py.  One JSON line per (esize, operation, variant); --out also writes them to a file.

    python scripts/measure_bplanes.py [--rounds 7] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))

import torch  # noqa: E402

import trc  # noqa: E402

SEG = 4096
DTYPES = {2: torch.bfloat16, 4: torch.float32, 8: torch.float64}


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1 MB instead of 100 MB: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    nbytes = (1 << 20) if args.small else 100 * 1000 * 1000
    lines = []
    for esize, dt in DTYPES.items():
        m = nbytes // esize
        n = m * esize
        g = torch.Generator(device="cuda:0").manual_seed(esize)
        w = torch.randn(m, generator=g, device="cuda:0", dtype=torch.float64) * 0.02
        pad = torch.zeros(trc.PAD, dtype=torch.uint8, device="cuda:0")
        base = torch.cat([w.to(dt).view(torch.uint8), pad])
        data = torch.cat([(w + torch.randn(m, generator=g, device="cuda:0", dtype=torch.float64) * 1e-4).to(dt).view(torch.uint8), pad])
        out, inplace = torch.zeros_like(data), base.clone()
        pitch = trc.planes_pitch(n, esize)
        planes = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")
        hist = torch.empty(trc.planes_hist_bytes(esize), dtype=torch.uint8, device="cuda:0")
        fp = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        Z, X = trc.FILTER_ZDELTA, trc.FILTER_XOR
        ops = {
            "split": {"plain": lambda: trc.planes_split(data, n, esize, planes, pitch),
                      "pred_z": lambda: trc.planes_split_filter(Z, data, n, esize, SEG, planes, pitch),
                      "base_z": lambda: trc.planes_split_base(Z, data, base, n, esize, planes, pitch),
                      "base_x": lambda: trc.planes_split_base(X, data, base, n, esize, planes, pitch)},
            "join": {"plain": lambda: trc.planes_join(planes, pitch, None, n, esize, out),
                     "pred_z": lambda: trc.planes_join_filter(Z, planes, pitch, None, n, esize, SEG, out),
                     "base_z": lambda: trc.planes_join_base(Z, planes, pitch, None, base, n, esize, out),
                     "base_x": lambda: trc.planes_join_base(X, planes, pitch, None, base, n, esize, out),
                     "base_z_in_place": lambda: trc.planes_join_base(Z, planes, pitch, None, inplace, n, esize, inplace)},
            "hist": {"pred": lambda: trc.planes_hist(7, data, n, esize, SEG, hist),
                     "base": lambda: trc.planes_hist_base(7, data, base, n, esize, hist)},
            "fingerprint": {"base": lambda: trc.base_fingerprint_enqueue(base, n, fp)},
        }
        trc.planes_split_base(Z, data, base, n, esize, planes, pitch)          # (planes that the joins read)
        for op, variants in ops.items():
            for fn in variants.values():                      # warm-up: code objects, clocks
                timed(fn, args.reps)
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v, fn in variants.items():
                    times[v].append(timed(fn, args.reps))
            for v, t in times.items():
                moved = {"split": 2, "join": 2, "hist": 1, "fingerprint": 1}[op] + (1 if v.startswith("base") and op != "fingerprint" else 0)
                med = statistics.median(t)
                line = {"esize": esize, "bytes": n, "op": op, "variant": v, "us_min": round(min(t), 2), "us_median": round(med, 2),
                        "us_max": round(max(t), 2), "bytes_moved_over_n": moved, "GBps_at_median": round(moved * n / med / 1e3, 1),
                        "rounds": args.rounds, "reps": args.reps}
                print(json.dumps(line), flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
