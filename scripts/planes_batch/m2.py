"""measurements 2 and 3: whole-step time (HIP events) and stored bytes of trc_encode_planes_batch_dev against a loop of
trc_encode_planes_dev, bf16 weights, item sets 1024 x 64 KiB and 64 x 1.5 MiB, codecs ANS4S and RCA, chunk 512 and 4096"""
import sys, os, statistics, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, trc, planes_lib as PL
esize = 2
REPS = 10
def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)
for name, count, size in (("1024 x 64 KiB", 1024, 65536), ("64 x 1.5 MiB", 64, 1536 * 1024)):
    w = PL.weights(count * size // esize, esize, seed=5)
    stride = size + 256                                         # the unbatched call wants TRC_PAD readable bytes behind every input
    host = np.zeros(count * stride, dtype=np.uint8)
    host.reshape(count, stride)[:, :size] = w.reshape(count, size)
    d_all = torch.from_numpy(host).to("cuda:0")
    tensors = [d_all[i * stride:i * stride + size] for i in range(count)]
    d_flat = torch.from_numpy(np.concatenate([w, np.zeros(256, np.uint8)])).to("cuda:0")
    for codec in (trc.ANS4S, trc.RCA):
        for chunk in (512, 4096):
            st = codec in trc.STATIC
            bc = trc.PlanesBatchCoder(codec, tensors, chunk, esize=esize)
            pc = trc.PlanesCoder(codec, size, esize, chunk, "cuda:0")
            def loop():
                for t in tensors:
                    pc.encode(t, size)
            for _ in range(3):
                bc.encode(); loop()
            tb, tl = [], []
            for _ in range(REPS):                               # alternating
                tb.append(timed(bc.encode)); tl.append(timed(loop))
            stored_b = bc.stored_bytes()
            stored_l = 0
            for t in tensors:                                   # untimed: every item's totals
                pc.encode(t, size)
                stored_l += sum(pc.result(k)[2] for k in range(esize)) + esize * (4 * pc.nch + (514 if st else 0))
            fc = trc.PlanesCoder(codec, count * size, esize, chunk, "cuda:0")
            fc.encode(d_flat, count * size)
            stored_f = sum(fc.result(k)[2] for k in range(esize)) + esize * (4 * fc.nch + (514 if st else 0))
            # round trip of the batch, once
            outs = [torch.empty_like(t) for t in tensors]
            bc.decode(out=outs); torch.cuda.synchronize()
            ok = all(torch.equal(o, t) for o, t in zip(outs, tensors))
            r = dict(items=name, codec=trc.CODEC_NAMES[codec], chunk=chunk, raw_bytes=count * size, pad_elems=bc.plan["pad_elems"], m_total=bc.plan["m_total"],
                     batch_ms_median=round(statistics.median(tb), 3), batch_ms_min=round(min(tb), 3), batch_ms_max=round(max(tb), 3),
                     loop_ms_median=round(statistics.median(tl), 3), loop_ms_min=round(min(tl), 3), loop_ms_max=round(max(tl), 3),
                     stored_batch=stored_b, stored_loop=stored_l, stored_contiguous=stored_f, roundtrip=ok)
            print(json.dumps(r), flush=True)
            del bc, pc, fc, outs
