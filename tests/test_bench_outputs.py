"""bench.py --dump-outputs: what the last timed step computed, as float arrays two builds can be compared on, and the plain
line (no --full) carrying the headline only.  The format and the sampling are checked on the CPU; on the GPU a plain run's dump
is compared with the same encode / decode called directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "beyond_cache", "host_pointer", "configs", "value_cold", "value_cold_clocks", "payload_sha256")


def test_dump_format_and_seeded_sample(tmp_path, monkeypatch):
    import torch
    # the largest dump: every array sampled -> float64 directory + two float32 byte arrays + one float64 total, within 64 MB
    assert bench.DUMP_MAX * (8 + 4 + 4) + 8 + 4 * 128 < 64 * 10**6
    monkeypatch.setattr(bench, "DUMP_MAX", 1000)
    rng = np.random.default_rng(5)
    n, nch, total = 5000, 700, 3000
    clen = torch.from_numpy(rng.integers(0, 2**31, nch + 64).astype(np.int32))
    clen[3] = -2                                                # the directory holds uint32 lengths in an int32 tensor
    payload = torch.from_numpy(rng.integers(0, 256, n + 64).astype(np.uint8))
    out = torch.from_numpy(rng.integers(0, 256, n + 512).astype(np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), (clen, payload, torch.tensor([total, 0])), total, nch, out, n)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["chunk_lengths", "compressed_bytes", "decoded", "payload"]
    assert got["chunk_lengths"].dtype == np.float64 and np.array_equal(got["chunk_lengths"], clen[:nch].numpy().view(np.uint32))
    assert got["compressed_bytes"].dtype == np.float64 and got["compressed_bytes"].tolist() == [total]
    idx = {m: np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, m, 1000)) for m in (total, n)}
    assert got["payload"].dtype == np.float32 and np.array_equal(got["payload"], payload.numpy()[idx[total]])
    assert got["decoded"].dtype == np.float32 and np.array_equal(got["decoded"], out.numpy()[idx[n]])
    for name, a in got.items():                                 # the same arguments give the same files
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_computed(tmp_path):
    import torch
    import trc
    assert torch.cuda.is_available(), "GPU tests need a GPU (and must not silently fall back)"
    n, steps = 3 * 10**6, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--size", str(n),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert all(k in j for k in HEADLINE) and j["steps"] == steps and j["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in j], "a plain run carries only the headline"

    chunk = j["config"]["chunk"]
    d, _ = bench.make_input(n, 0, "text")
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
    dc = trc.DeviceCoder(trc.ANS4S, n, chunk, "cuda:0")
    dc.cdfini(d_in, n, 256)
    dc.encode(d_in, n)
    clen, payload = dc.result(n)
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("chunk_lengths", "compressed_bytes", "payload", "decoded")}
    assert got["compressed_bytes"].tolist() == [payload.size] == [j["config"]["compressed_bytes_per_gpu"]]
    assert np.array_equal(got["chunk_lengths"], clen.astype(np.float64))
    assert np.array_equal(got["payload"], payload.astype(np.float32))
    assert np.array_equal(got["decoded"], d.astype(np.float32))
