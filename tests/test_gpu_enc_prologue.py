"""The static rANS encoder's start-up at the edges of its workgroup shapes (csrc/trc_ans_static.hip, top of trc_ans4s_enc_kernel):
every wave of a workgroup fills its share of the symbol table and reaches the workgroup's barrier, a wave that has no chunks leaves
behind it, and the first input line is requested for the rows a wave really has.  (Three orders of the table fill, the barrier and
the first line were measured, profiles/edges/edges_notes.md; whichever one the kernel runs has to pass here.)

Against the oracle's encode of every chunk, in each workgroup shape of the encoder (TRC_ENC_WPB = 1 / 4 / 12, read once per process:
a fresh child for each):

  chunk counts  1, 64, 65, 64 * 12 - 1, 64 * 12 + 1: one lane; exactly one wave (in a workgroup of 4 or 12 the others are empty and
                only pass the barrier); one wave and a lane; a workgroup of twelve waves one chunk short; one chunk more, which opens
                a second workgroup with one live lane and eleven (or three) empty waves
  chunks        256, 320 and 512 bytes.  256 is TRC_CHUNK_MIN, the smallest chunk the library takes (a chunk of 64 bytes, one segment,
                is refused with TRC_E_ARG by every entry point and cannot be run); 320 is five segments: the top segment is an even
                one, and the start requests that segment alone; 256 and 512 have an odd top segment (both halves of the top line)
  last chunk    whole, and ragged (its length no multiple of 4 or of 64)

Expected lengths and payloads are computed once here and handed to the children in a file; the children compare the device's
directory and payload with them byte for byte and decode."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import trc
import trc_testlib as T

pytestmark = pytest.mark.gpu

CHUNKS = (256, 320, 512)
NCHUNKS = (1, 64, 65, 64 * 12 - 1, 64 * 12 + 1)
RAGGED_CUT = 101                     # the ragged last chunk is this much short: 155 / 219 / 411 bytes, = 3 mod 4, no multiple of 64


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    _, cdf, cdfnum = T.orc_cdfini(T.text_bytes(1 << 20, 3), 256)
    assert cdfnum == 256
    arrays, names, seed = {"cdf": cdf}, [], 300
    for chunk in CHUNKS:
        for nch in NCHUNKS:
            for n in (nch * chunk, nch * chunk - RAGGED_CUT):
                seed += 1
                d = T.text_bytes(n, seed)
                payload, clen, _ = T.orc_chunked_enc(T.ANS4S, d, chunk, cdf, cdfnum)
                assert clen.size == nch and (n == nch * chunk or (n % 4 and n % 64))
                name = "%d-%d-%d" % (chunk, nch, n)
                names.append(name)
                for k, v in (("d", d), ("clen", clen), ("payload", payload)):
                    arrays[name + "/" + k] = v
    path = str(tmp_path_factory.mktemp("enc_prologue") / "cases.npz")
    np.savez(path, names=np.array(names), **arrays)
    return path


CHILD = textwrap.dedent("""
    import sys, numpy as np, torch
    sys.path[:0] = [%r, %r]
    import trc, trc_testlib as T
    z = np.load(sys.argv[1])
    cdf = z["cdf"]
    for name in z["names"]:
        name = str(name)
        chunk, nch, n = (int(x) for x in name.split("-"))
        d = z[name + "/d"]
        dc = trc.DeviceCoder(trc.ANS4S, n, chunk, "cuda:0")
        dc.set_cdf(cdf, 256)
        d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
        dc.encode(d_in, n)
        clen, payload = dc.result(n)
        assert np.array_equal(clen, z[name + "/clen"]), ("clen", name, np.flatnonzero(clen != z[name + "/clen"])[:8])
        assert np.array_equal(payload, z[name + "/payload"]), ("payload", name)
        out = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
        dc.decode(out, n, dir_ready=True); torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:n], d) and (o[n:] == 0xA5).all(), ("roundtrip", name)
    print("ok", len(z["names"]))
""") % (os.path.dirname(os.path.abspath(trc.__file__)), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wpb", (1, 4, 12))
def test_workgroup_edges_match_oracle(cases, wpb):
    r = subprocess.run([sys.executable, "-c", CHILD, cases], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TRC_ENC_WPB=str(wpb)))
    want = "ok %d" % (len(CHUNKS) * len(NCHUNKS) * 2)
    assert r.returncode == 0 and want in r.stdout, (wpb, r.stdout[-2000:] + r.stderr[-3000:])
