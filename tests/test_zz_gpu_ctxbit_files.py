"""GPU (-m gpu), behind the parity tests in collection order (it starts separate programs): the reference's own file format
for file codecs 2 (rccsenc per block) and 4 (rcxsenc per block), in the shape of test_reference_file_format_interop.  With
blocks that are legal chunk sizes a block IS a chunk, so `trcfile C` writes the reference's bytes and each tool reads the
other's files."""
import os
import subprocess

import pytest

import ctxbit_lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fc", [2, 4])
def test_reference_file_format_interop_ctxbit(fc, tmp_path):
    ref = os.path.join(ROOT, "oracle", "_ref", "turborc_ref")
    exe = os.path.join(ROOT, "harness", "trcfile")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/turborc_ref not built (scripts/link_reference_harness.sh --install, build container only)")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    for kind, n, bs in (("markov", 3000001, 65536), ("text", 65536 * 3, 65536), ("uniform", 200000, 65536), ("runs", 100000, 16384),
                        ("markov", 70, 65536)):
        src, ours, theirs, back = tmp_path / "in.bin", tmp_path / "ours.rc", tmp_path / "theirs.rc", tmp_path / "back.bin"
        L.gen(kind, n, 77).tofile(src)
        r = subprocess.run([exe, "C", str(src), str(ours), str(bs), str(fc)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([ref, "-0%d" % fc, "-b%dB" % bs, str(src), str(theirs)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(ours, "rb").read() == open(theirs, "rb").read(), (fc, kind, n, "files differ")
        r = subprocess.run([ref, "-d", str(ours), str(back)], capture_output=True, text=True, timeout=120)     # reference reads ours
        assert r.returncode == 0 and open(back, "rb").read() == open(src, "rb").read(), (fc, kind, n, r.stdout + r.stderr)
        os.remove(back)
        r = subprocess.run([exe, "D", str(theirs), str(back)], capture_output=True, text=True, timeout=120)   # we read the reference's
        assert r.returncode == 0 and open(back, "rb").read() == open(src, "rb").read(), (fc, kind, n, r.stdout + r.stderr)
