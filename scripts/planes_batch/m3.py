"""measurement 3 on a set whose pad is not zero: 1024 bf16 items of 32 768 - 1 - (37 i mod 2000) elements; stored bytes of the batch
against the planes call on the concatenated items (no pad) and against the per-item loop, chunk 512 and 4096"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "turbo-range-coder_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, trc, planes_lib as PL
esize, count = 2, 1024
ms = [32768 - 1 - (37 * i) % 2000 for i in range(count)]
w = PL.weights(sum(ms), esize, seed=5)
stride = 65536 + 256
host = np.zeros(count * stride, dtype=np.uint8)
pos = 0
for i, m in enumerate(ms):
    host[i * stride:i * stride + m * esize] = w[pos:pos + m * esize]; pos += m * esize
d_all = torch.from_numpy(host).to("cuda:0")
tensors = [d_all[i * stride:i * stride + m * esize] for i, m in enumerate(ms)]
d_flat = torch.from_numpy(np.concatenate([w, np.zeros(256, np.uint8)])).to("cuda:0")
for codec in (trc.ANS4S, trc.RCA):
    for chunk in (512, 4096):
        st = codec in trc.STATIC
        bc = trc.PlanesBatchCoder(codec, tensors, chunk, esize=esize)
        bc.encode()
        stored_b = bc.stored_bytes()
        stored_l = 0
        for t, m in zip(tensors, ms):
            pc = trc.PlanesCoder(codec, m * esize, esize, chunk, "cuda:0")
            pc.encode(t, m * esize)
            stored_l += sum(pc.result(k)[2] for k in range(esize)) + esize * (4 * pc.nch + (514 if st else 0))
        fc = trc.PlanesCoder(codec, w.size, esize, chunk, "cuda:0")
        fc.encode(d_flat, w.size)
        stored_f = sum(fc.result(k)[2] for k in range(esize)) + esize * (4 * fc.nch + (514 if st else 0))
        outs = [torch.empty_like(t) for t in tensors]
        bc.decode(out=outs); torch.cuda.synchronize()
        ok = all(torch.equal(o, t) for o, t in zip(outs, tensors))
        print(json.dumps(dict(codec=trc.CODEC_NAMES[codec], chunk=chunk, raw_bytes=int(w.size), elems=sum(ms), pad_elems=bc.plan["pad_elems"], m_total=bc.plan["m_total"],
                              chunks_batch=bc.nch, chunks_contiguous=fc.nch, stored_batch=stored_b, stored_loop=stored_l, stored_contiguous=stored_f, roundtrip=ok)), flush=True)
        del bc, fc, outs
