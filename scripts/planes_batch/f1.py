"""kernel times of the filtered batched split and join and of their yardsticks, all cases in one process under the kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d OUT -o f1 -- python scripts/planes_batch/f1.py OUT/cases.json
    python scripts/planes_batch/f1_sum.py OUT
100 MB as 1, 1024 and 100 000 equal items back to back in one buffer; esize 2 and 4; chunk 256 and 4096; per case 3 warm-up + 10 timed
split + join pairs and join(split(x)) == x at the end.  kinds: none = trc_planes_split_batch_dev / join (the cost of the filter),
delta = every item TRC_FILTER_ZDELTA, cycle = filters (0, 1, 2, ..); flat-none = trc_planes_split_dev / join on the contiguous
buffer (the cost of the map of the unfiltered pair).
OUT/cases.json lists the cases in the order they ran with the pattern of plane-kernel dispatches of one pair."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, trc
REPS = 13
SIZE = {1: 100007936, 1024: 97664, 100000: 1008}               # bytes per item, multiples of 16
rng = np.random.default_rng(1)
N = max(c * s for c, s in SIZE.items())
d_in = torch.from_numpy(rng.integers(0, 256, N + 256, dtype=np.uint8)).to("cuda:0")
d_out = torch.empty(N + 256, dtype=torch.uint8, device="cuda:0")
cases = []


def done(name, n, pattern, **more):
    torch.cuda.synchronize()
    assert torch.equal(d_in[:n], d_out[:n]), name
    d_out.zero_()
    cases.append(dict(name=name, reps=REPS, pattern=pattern, **more))
    print("ok", name, more, flush=True)


for esize in (2, 4):
    n = SIZE[1]
    pitch = trc.planes_pitch(n, esize)
    d_planes = torch.empty(esize * pitch, dtype=torch.uint8, device="cuda:0")
    for i in range(REPS):
        trc.planes_split(d_in, n, esize, d_planes, pitch, None)
        trc.planes_join(d_planes, pitch, None, n, esize, d_out)
    done("flat-none esize %d" % esize, n, ["split", "join"])
    del d_planes
    for count in (1, 1024, 100000):
        size = SIZE[count]
        n = count * size
        src = trc.planes_items([(d_in.data_ptr() + i * size, size) for i in range(count)])
        dst = trc.planes_items([(d_out.data_ptr() + i * size, size) for i in range(count)])
        for chunk in (256, 4096):
            plan, first = trc.planes_batch_plan(src, count, esize, chunk)
            pitch = plan["pitch"]
            d_planes = torch.empty(esize * pitch, dtype=torch.uint8, device="cuda:0")
            tb = trc.lib().trc_planes_batch_table_bytes(count, plan["chunks"])
            d_table = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
            for kind in ("none", "delta", "cycle"):
                filters = None if kind == "none" else trc.planes_filters(1 if kind == "delta" else [i % 3 for i in range(count)], count)
                for i in range(REPS):
                    if kind == "none":
                        trc.planes_split_batch(src, count, esize, chunk, d_planes, pitch, d_table, tb)
                        trc.planes_join_batch(d_planes, 0, pitch, dst, count, 0, count, esize, chunk, d_table, tb)
                    else:
                        trc.planes_split_fbatch(src, filters, count, esize, chunk, d_planes, pitch, d_table, tb)
                        trc.planes_join_fbatch(d_planes, 0, pitch, dst, filters, count, 0, count, esize, chunk, d_table, tb)
                done("batch-%s items %d esize %d chunk %d" % (kind, count, esize, chunk), n, ["map", "split", "map", "join"],
                     m_total=plan["m_total"], pad_elems=plan["pad_elems"], chunks=plan["chunks"])
            del d_planes, d_table
json.dump(cases, open(sys.argv[1], "w"), indent=1)
