"""one case of measurement 1: CASE in flat / batch1 / batch1024, ESIZE, CHUNK; 3 warm-up + 20 timed split + join pairs on 100 MB"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, trc
case, esize, chunk = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
ITEM = 97664                                   # bytes; 1024 items = 100 007 936 bytes
count = 1024
n = ITEM * count
rng = np.random.default_rng(1)
d_in = torch.from_numpy(rng.integers(0, 256, n + 256, dtype=np.uint8)).to("cuda:0")
d_out = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
if case == "flat":
    pitch = trc.planes_pitch(n, esize)
    d_planes = torch.empty(esize * pitch, dtype=torch.uint8, device="cuda:0")
    for i in range(23):
        trc.planes_split(d_in, n, esize, d_planes, pitch, None)
        trc.planes_join(d_planes, pitch, None, n, esize, d_out)
else:
    cnt = 1 if case == "batch1" else count
    size = n // cnt
    src = trc.planes_items([(d_in.data_ptr() + i * size, size) for i in range(cnt)])
    dst = trc.planes_items([(d_out.data_ptr() + i * size, size) for i in range(cnt)])
    plan, first = trc.planes_batch_plan(src, cnt, esize, chunk)
    pitch = plan["pitch"]
    d_planes = torch.empty(esize * pitch, dtype=torch.uint8, device="cuda:0")
    tb = trc.lib().trc_planes_batch_table_bytes(cnt, plan["chunks"])
    d_table = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
    for i in range(23):
        trc.planes_split_batch(src, cnt, esize, chunk, d_planes, pitch, d_table, tb)
        trc.planes_join_batch(d_planes, 0, pitch, dst, cnt, 0, cnt, esize, chunk, d_table, tb)
    print("plan", plan)
torch.cuda.synchronize()
assert torch.equal(d_in[:n], d_out[:n])
print("ok", case, esize, chunk)
