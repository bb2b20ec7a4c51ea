"""What the byte-plane calls cost (profiles/planes/planes_notes.md).
Kernels: HIP-event time of trc_planes_split_dev and trc_planes_join_dev at 100 MB and 1 GB for esize 2 / 4 / 8, against a
device-to-device copy of the same n bytes taken in the same process and alternated with the kernel: the median of REPS calls after
one warm-up call, every value kept, every output compared with the transpose torch computes.
Coded: trc_encode_planes_dev + trc_decode_planes_dev for anscdf4s and rccdf on 100 MB of bf16 weights at trc_round_chunk(codec, m),
next to the flat trc_encode_dev + trc_decode_dev on the same bytes at trc_round_chunk(codec, n), with both stored sizes.
usage: planes_time.py <out.jsonl> [kernels|coded]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "turbo-range-coder_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import trc
import planes_lib as PL

REPS = 9
SIZES = (100 * 1000 * 1000, 1 << 30)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b), 4)


def alternated(fn, copy, verify):
    """-> (kernel times, copy times): one warm-up each, then REPS rounds of copy, kernel; verify() after every kernel call"""
    fn(); copy()
    torch.cuda.synchronize()
    k, c = [], []
    for _ in range(REPS):
        c.append(event_ms(copy))
        k.append(event_ms(fn))
        verify()
    return k, c


def kernels(rows):
    for n in SIZES:
        g = torch.Generator(device="cuda:0"); g.manual_seed(n)
        d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
        d_copy = torch.empty_like(d_in)
        for esize in PL.ESIZES:
            m, t = n // esize, n % esize
            pitch = trc.planes_pitch(n, esize)
            d_planes = torch.zeros(esize * pitch, dtype=torch.uint8, device="cuda:0")
            d_tail = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
            d_out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            exp = d_in[:m * esize].view(m, esize).t().contiguous()

            def check_split():
                assert torch.equal(d_planes.view(esize, pitch)[:, :m], exp) and torch.equal(d_tail[:t], d_in[m * esize:])

            def check_join():
                assert torch.equal(d_out, d_in)
            for what, fn, verify in (("trc_planes_split_dev", lambda: trc.planes_split(d_in, n, esize, d_planes, pitch, d_tail), check_split),
                                     ("trc_planes_join_dev", lambda: trc.planes_join(d_planes, pitch, d_tail, n, esize, d_out), check_join)):
                k, c = alternated(fn, lambda: d_copy.copy_(d_in), verify)
                mk, mc = float(np.median(k)), float(np.median(c))
                rows.append(dict(what=what, n=n, esize=esize, median_ms=mk, copy_median_ms=mc, ratio=round(mk / mc, 4),
                                 gbps_in_plus_out=round(2 * n / mk / 1e6, 1), all_ms=k, copy_all_ms=c))
                print(json.dumps(rows[-1]), flush=True)
            del d_planes, d_out, exp
        del d_in, d_copy
        torch.cuda.empty_cache()


def coded(rows):
    n, esize = 100 * 1000 * 1000, 2
    m = n // esize
    d = PL.weights(m, esize)
    d_in = torch.from_numpy(np.concatenate([d, np.zeros(512, np.uint8)])).to("cuda:0")
    d_out = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
    for codec in (trc.ANS4S, trc.RCA):
        name = trc.CODEC_NAMES[codec]
        chunk_p, chunk_f = trc.lib().trc_round_chunk(codec, m), trc.lib().trc_round_chunk(codec, n)
        pc = trc.PlanesCoder(codec, n, esize, chunk_p, "cuda:0")
        dc = trc.DeviceCoder(codec, n, chunk_f, "cuda:0")

        def planar():
            pc.encode(d_in, n); pc.decode(d_out, n)

        def flat():
            if codec in trc.STATIC:
                dc.cdfini(d_in, n, 256)                        # the planar encode builds its CDFs inside the call: the flat side pays for its own
            dc.encode(d_in, n); dc.decode(d_out, n)

        def verify():
            assert torch.equal(d_out[:n], d_in[:n])
        kp, kf = alternated(planar, flat, verify)
        verify()
        stored_p = sum(pc.result(k)[2] + 4 * pc.nch for k in range(esize))
        clen, payload = dc.result(n)
        rows.append(dict(what="encode + decode", codec=name, n=n, esize=esize, planar_chunk=chunk_p, flat_chunk=chunk_f,
                         planar_median_ms=float(np.median(kp)), flat_median_ms=float(np.median(kf)), planar_all_ms=kp, flat_all_ms=kf,
                         planar_stored=int(stored_p), flat_stored=int(payload.size + 4 * clen.size)))
        print(json.dumps(rows[-1]), flush=True)
        del pc, dc
        torch.cuda.empty_cache()


def main(path, which):
    rows = []
    if which in ("all", "kernels"):
        kernels(rows)
    if which in ("all", "coded"):
        coded(rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "all")
