"""What the strided split / join / histogram kernels cost (profiles/planes/splanes_notes.md).
HIP-event time at 100 MB for esize 2 / 4 / 8 of trc_planes_split_sfilter_dev, trc_planes_join_sfilter_dev (both filters) and
trc_planes_hist_stride_dev (all three rows) at strides 2, 3, 4 and 8, next to the existing stride-1 calls (trc_planes_split_filter_dev,
trc_planes_join_filter_dev, trc_planes_hist_dev) on the same buffers and a device-to-device copy of the same n bytes, all in one
process, restart length 4096.  One round times every variant once (an event pair around INNER back-to-back calls, divided by
INNER); ROUNDS rounds after one warm-up round, so the variants alternate and share whatever else the machine is doing.  Every
value is kept; the rows give median, min and max and the ratio to the stride-1 call.  In the warm-up round every join output is
compared with the input on the device and every histogram's rows are checked to sum to m (the values against the numpy model are
what tests/test_gpu_splanes.py checks).
usage: splanes_time.py <out.jsonl> [n_bytes]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))
import trc

ROUNDS, INNER = 9, 50
SEG = 4096
STRIDES = (1, 2, 3, 4, 8)
FILTERS = ((trc.FILTER_ZDELTA, "zdelta"), (trc.FILTER_XOR, "xor"))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


def main(path, n):
    assert torch.cuda.is_available(), "this probe needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "w")
    g = torch.Generator(device="cuda:0"); g.manual_seed(n)
    d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    d_copy = torch.empty_like(d_in)
    d_out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_tail = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    for esize in (2, 4, 8):
        m = n // esize
        pitch = trc.planes_pitch(n, esize)
        d_hist = torch.zeros(trc.planes_hist_bytes(esize), dtype=torch.uint8, device="cuda:0")
        planes = {}
        variants = [("copy", "none", 0, lambda: d_copy.copy_(d_in))]
        for stride in STRIDES:
            for filt, fname in FILTERS:
                p = planes[(filt, stride)] = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")
                if stride == 1:                                  # the existing calls, by their own entry points
                    variants.append(("split", fname, 1, lambda filt=filt, p=p: trc.planes_split_filter(filt, d_in, n, esize, SEG, p, pitch, d_tail)))
                    variants.append(("join", fname, 1, lambda filt=filt, p=p: trc.planes_join_filter(filt, p, pitch, d_tail, n, esize, SEG, d_out)))
                else:
                    variants.append(("split", fname, stride, lambda filt=filt, p=p, s=stride: trc.planes_split_sfilter(filt, s, d_in, n, esize, SEG, p, pitch, d_tail)))
                    variants.append(("join", fname, stride, lambda filt=filt, p=p, s=stride: trc.planes_join_sfilter(filt, s, p, pitch, d_tail, n, esize, SEG, d_out)))
            if stride == 1:
                variants.append(("hist", "all", 1, lambda: trc.planes_hist(7, d_in, n, esize, SEG, d_hist)))
            else:
                variants.append(("hist", "all", stride, lambda s=stride: trc.planes_hist_stride(7, s, d_in, n, esize, SEG, d_hist)))
        for what, fname, stride, fn in variants:                 # warm-up round, with the checks
            d_out.zero_()
            fn()
            torch.cuda.synchronize()
            if what == "join":
                assert torch.equal(d_out, d_in), (what, fname, stride, esize)
            if what == "hist":
                h = d_hist.cpu().numpy().view("<u8").reshape(3 * esize, 256)
                assert (h.sum(axis=1) == m).all(), (what, stride, esize)
        times = [[] for _ in variants]
        for _ in range(ROUNDS):
            for i, (_, _, _, fn) in enumerate(variants):
                times[i].append(round(event_ms(fn), 5))
        base = {}
        for (what, fname, stride, _), t in zip(variants, times):
            med = float(np.median(t))
            if stride <= 1:
                base[(what, fname)] = med
            row = dict(what=what, filter=fname, stride=stride, seg=SEG, esize=esize, n=n, median_ms=round(med, 5), min_ms=min(t), max_ms=max(t),
                       gbps_in=round(n / med / 1e6, 1), over_stride1=round(med / base[(what, fname)], 4), over_copy=round(med / base[("copy", "none")], 4), all_ms=t)
            out.write(json.dumps(row) + "\n"); out.flush()
            print(json.dumps({k: v for k, v in row.items() if k != "all_ms"}), flush=True)
        del planes, variants
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 100 * 1000 * 1000)
