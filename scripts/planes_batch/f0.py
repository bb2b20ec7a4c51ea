"""order-0 estimate of the planes of a mixed batch under three filter assignments (numpy only, no GPU):
    python scripts/planes_batch/f0.py
The batch: sorted u32 ids, u32 timestamps with small steps, fp32 N(0, 1) values bit-cast; 1 M elements each, chunk 4096.
Prints bits per byte of every plane (order-0 entropy of the plane of VF, pad included) and of the whole batch."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fplanes_batch_lib as FBL
import planes_lib as PL

M, ESIZE, CHUNK = 1 << 20, 4, 4096
rng = np.random.default_rng(7)
ids = np.sort(rng.integers(0, 1 << 32, M, dtype=np.uint64)).astype("<u4")
stamps = (1_700_000_000 + np.cumsum(rng.integers(0, 4, M))).astype("<u4")
values = rng.standard_normal(M).astype("<f4")
items = [x.view(np.uint8) for x in (ids, stamps, values)]


def bits(plane):
    c = np.bincount(plane, minlength=256).astype(np.float64)
    c = c[c > 0]
    return float((c * np.log2(plane.size / c)).sum())


for name, filters in (("no filter", [0, 0, 0]), ("delta on every item", [1, 1, 1]), ("xor on every item", [2, 2, 2]), ("per item (1, 1, 0)", [1, 1, 0])):
    planes, _ = PL.split(FBL.virtual_filtered(items, filters, ESIZE, CHUNK), ESIZE)
    b = [bits(p) for p in planes]
    print("%-22s planes %s   all %.3f bits per byte" % (name, " ".join("%.3f" % (x / planes[0].size) for x in b), sum(b) / (ESIZE * planes[0].size)))
    for i, col in enumerate(("ids", "timestamps", "values")):
        pl, _ = PL.split(FBL.filtered(items, filters, ESIZE, CHUNK)[i], ESIZE)
        print("    %-12s filter %d: %.3f bits per byte" % (col, filters[i], sum(bits(p) for p in pl) / (ESIZE * M)))
