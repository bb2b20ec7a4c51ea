"""What the filtered split / join kernels cost (profiles/planes/fplanes_notes.md).
HIP-event time at 256 MiB for esize 2 / 4 / 8 of trc_planes_split_filter_dev and trc_planes_join_filter_dev, both filters, at the
restart lengths 256 / 4096 / 65536, next to the UNFILTERED trc_planes_split_dev / trc_planes_join_dev on the same buffers and a
device-to-device copy of the same n bytes, all in one process.  One round times every variant once (an event pair around INNER
back-to-back calls, divided by INNER); ROUNDS rounds after one warm-up round, so the variants alternate and share whatever else
the machine is doing.  Every value is kept; the rows give median, min and max.  Every join output is compared with the input on
the device (join of split is the identity; the split against the numpy model is what tests/test_gpu_fplanes.py checks).
usage: fplanes_time.py <out.jsonl> [n_bytes]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))
import trc

ROUNDS, INNER = 9, 10
SEGS = (256, 4096, 65536)
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
        d_planes = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")      # the unfiltered planes of d_in
        d_fplanes = {}                                                                 # (filter, seg) -> filtered planes of d_in
        variants = [("copy", None, None, lambda: d_copy.copy_(d_in)),
                    ("split", None, None, lambda: trc.planes_split(d_in, n, esize, d_planes, pitch, d_tail)),
                    ("join", None, None, lambda: trc.planes_join(d_planes, pitch, d_tail, n, esize, d_out))]
        for filt, fname in FILTERS:
            for seg in SEGS:
                p = d_fplanes[(filt, seg)] = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")
                variants.append(("split", fname, seg, lambda filt=filt, seg=seg, p=p: trc.planes_split_filter(filt, d_in, n, esize, seg, p, pitch, d_tail)))
                variants.append(("join", fname, seg, lambda filt=filt, seg=seg, p=p: trc.planes_join_filter(filt, p, pitch, d_tail, n, esize, seg, d_out)))
        # warm-up round, with the checks: every join returns d_in (a filtered join reads what the filtered split in front of it in
        # `variants` has just written), and the filtered planes are not the unfiltered ones
        for what, fname, seg, fn in variants:
            d_out.zero_()
            fn()
            torch.cuda.synchronize()
            if what == "join":
                assert torch.equal(d_out, d_in), (what, fname, seg, esize)
        for p in d_fplanes.values():
            assert not torch.equal(p.view(esize, pitch)[:, :m], d_planes.view(esize, pitch)[:, :m])
        times = [[] for _ in variants]
        for _ in range(ROUNDS):
            for i, (_, _, _, fn) in enumerate(variants):
                times[i].append(round(event_ms(fn), 5))
        base = {}
        for (what, fname, seg, _), t in zip(variants, times):
            med = float(np.median(t))
            if fname is None:
                base[what] = med
            row = dict(what=what, filter=fname or "none", seg=seg, esize=esize, n=n, median_ms=round(med, 5), min_ms=min(t), max_ms=max(t),
                       gbps_in_plus_out=round(2 * n / med / 1e6, 1), all_ms=t)
            if fname is not None:
                row["over_unfiltered"] = round(med / base[what], 4)
            row["over_copy"] = round(med / base["copy"], 4)
            out.write(json.dumps(row) + "\n"); out.flush()
            print(json.dumps({k: v for k, v in row.items() if k != "all_ms"}), flush=True)
        del d_planes, d_fplanes, variants
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 256 << 20)
