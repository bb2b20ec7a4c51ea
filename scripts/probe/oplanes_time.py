"""What the order-2 / order-3 split, join and histogram kernels cost, and what the orders store (profiles/planes/oplanes_notes.md).
HIP-event time at 100 MB for esize 2 / 4 / 8 of trc_planes_split_ofilter_dev and trc_planes_join_ofilter_dev at orders 2 and 3 and
strides 1, 2 and 8, next to the order-1 calls of the same stride (trc_planes_split_sfilter_dev / join, zigzag delta: unchanged code),
of trc_planes_hist_order_dev(15) next to trc_planes_hist_stride_dev(7) at the same strides, and of a device-to-device copy of the
same n bytes, all in one process, restart length 4096.  One round times every variant once (an event pair around INNER back-to-back
calls, divided by INNER); ROUNDS rounds after one warm-up round, so the variants alternate and share whatever else the machine is
doing.  Every value is kept; the rows give median, min and max and the ratio to the order-1 call of the same stride.  In the
warm-up round every join output is compared with the input on the device and every histogram's rows are checked to sum to m (the
values against the numpy model are what tests/test_gpu_oplanes.py checks).
Then the table of the notes: the five inputs of tests/oplanes_lib.table_inputs (2^20 elements each), their order-0 model estimates
under orders 0 .. 3 at restart 4096 from the numpy model, the size of the rccdf container trc_encode_*_host writes for each order
at chunk 4096, and the order advisor's choice.
usage: oplanes_time.py <out.jsonl> [n_bytes]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trc

ROUNDS, INNER = 9, 50
SEG = 4096
STRIDES = (1, 2, 8)
ORDERS = (1, 2, 3)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


def kernels(out, n):
    g = torch.Generator(device="cuda:0"); g.manual_seed(n)
    d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    d_copy = torch.empty_like(d_in)
    d_out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_tail = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    for esize in (2, 4, 8):
        m = n // esize
        pitch = trc.planes_pitch(n, esize)
        d_hist = torch.zeros(trc.planes_hist_order_bytes(esize), dtype=torch.uint8, device="cuda:0")
        planes = {}
        variants = [("copy", 0, 0, lambda: d_copy.copy_(d_in))]
        for stride in STRIDES:
            for order in ORDERS:
                p = planes[(order, stride)] = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")
                if order == 1:                                   # the existing calls, by their own entry points
                    variants.append(("split", 1, stride, lambda p=p, s=stride: trc.planes_split_sfilter(trc.FILTER_ZDELTA, s, d_in, n, esize, SEG, p, pitch, d_tail)))
                    variants.append(("join", 1, stride, lambda p=p, s=stride: trc.planes_join_sfilter(trc.FILTER_ZDELTA, s, p, pitch, d_tail, n, esize, SEG, d_out)))
                else:
                    variants.append(("split", order, stride, lambda p=p, k=order, s=stride: trc.planes_split_ofilter(k, s, d_in, n, esize, SEG, p, pitch, d_tail)))
                    variants.append(("join", order, stride, lambda p=p, k=order, s=stride: trc.planes_join_ofilter(k, s, p, pitch, d_tail, n, esize, SEG, d_out)))
            variants.append(("hist", 1, stride, lambda s=stride: trc.planes_hist_stride(7, s, d_in, n, esize, SEG, d_hist)))       # (rows: none, zdelta, xor)
            variants.append(("hist", 3, stride, lambda s=stride: trc.planes_hist_order(15, s, d_in, n, esize, SEG, d_hist)))       # (rows: orders 0 .. 3)
        for what, order, stride, fn in variants:                 # warm-up round, with the checks
            d_out.zero_()
            fn()
            torch.cuda.synchronize()
            if what == "join":
                assert torch.equal(d_out, d_in), (what, order, stride, esize)
            if what == "hist":
                rows = (3 if order == 1 else 4) * esize
                h = d_hist.cpu().numpy().view("<u8")[:rows * 256].reshape(rows, 256)
                assert (h.sum(axis=1) == m).all(), (what, order, stride, esize)
        times = [[] for _ in variants]
        for _ in range(ROUNDS):
            for i, (_, _, _, fn) in enumerate(variants):
                times[i].append(round(event_ms(fn), 5))
        base = {}
        for (what, order, stride, _), t in zip(variants, times):
            med = float(np.median(t))
            if order <= 1:
                base[(what, stride)] = med
            row = dict(what=what, order=order, stride=stride, seg=SEG, esize=esize, n=n, median_ms=round(med, 5), min_ms=min(t), max_ms=max(t),
                       gbps_in=round(n / med / 1e6, 1), over_order1=round(med / base[(what, stride)], 4), over_copy=round(med / base[("copy", 0)], 4), all_ms=t)
            out.write(json.dumps(row) + "\n"); out.flush()
            print(json.dumps({k: v for k, v in row.items() if k != "all_ms"}), flush=True)
        del planes, variants
        torch.cuda.empty_cache()


def table(out):
    import oplanes_lib as OL
    for name, esize, stride, d in OL.table_inputs():
        m = d.size // esize
        est = OL.estimates(OL.hist4(d, esize, SEG, stride), esize, m) / 8
        sizes = [trc.host_encode_planes(trc.RCA, d, esize, SEG).size,
                 (trc.host_encode_fplanes(trc.RCA, trc.FILTER_ZDELTA, d, esize, SEG) if stride == 1
                  else trc.host_encode_splanes(trc.RCA, trc.FILTER_ZDELTA, stride, d, esize, SEG)).size]
        for order in (2, 3):
            comp = trc.host_encode_oplanes(trc.RCA, order, stride, d, esize, SEG)
            assert np.array_equal(trc.host_decode_oplanes(comp, d.size), d), (name, order)
            sizes.append(comp.size)
        comp, a = trc.host_encode_aoplanes(trc.RCA, stride, d, esize, SEG)
        assert comp.size == sizes[a["order"]] and a["order"] == OL.advise(OL.hist4(d, esize, SEG, stride), 15, esize, m), name
        row = dict(what="table", input=name, esize=esize, stride=stride, bytes=int(d.size), estimate_bytes=[int(round(x)) for x in est],
                   rccdf_container_bytes=sizes, advisor_order=a["order"])
        out.write(json.dumps(row) + "\n"); out.flush()
        print(json.dumps(row), flush=True)


def main(path, n):
    assert torch.cuda.is_available(), "this probe needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        table(out)
        kernels(out, n)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 100 * 1000 * 1000)
