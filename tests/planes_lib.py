"""Byte planes of 16 / 32 / 64-bit elements: the numpy definition the planar calls are checked against, the inputs of the GPU
tests, and the reference's own byte transpose (tpenc) for the fixture tests/golden/planes_vectors.npz.

Plane k of n bytes of esize-byte elements is byte k of every whole element (m = n // esize of them); the t = n % esize tail
bytes follow.  The reference's tpenc gives this layout where n % (32 * esize) < esize -- the lengths the fixture records -- and
an ISA-dependent one elsewhere, so it is built here only to pin the definition: Ref(dir) compiles the reference's
transpose sources as its makefile does into a directory of the caller's, outside the repository, where the sources exist.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ESIZES = (2, 4, 8)
REF_DIR = os.environ.get("TRC_REFERENCE", "/root/reference")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planes_vectors.npz")


def split(data, esize):
    """-> (planes: uint8 array [esize, m], tail: uint8 array [n % esize]) -- the reshape-transpose plus the tail"""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    m = d.size // esize
    return np.ascontiguousarray(d[:m * esize].reshape(m, esize).T), d[m * esize:].copy()


def join(planes, tail):
    return np.concatenate([np.ascontiguousarray(planes.T).reshape(-1), tail]).astype(np.uint8)


def flat(data, esize):
    """the split as one byte string: plane 0 | plane 1 | ... | tail (what tpenc writes)"""
    p, t = split(data, esize)
    return np.concatenate([p.reshape(-1), t])


def golden_lengths(esize):
    """lengths with n % (32 * esize) < esize, where the reference's tpenc is the plain layout whatever ISA it was built for"""
    return [32 * esize * j + r for j in (1, 8, 64) for r in (0, esize - 1)]


def golden_input(esize, n):
    return np.random.default_rng(1000 * esize + n).integers(0, 256, n, dtype=np.uint8)


def load_golden():
    """-> {(esize, n): tpenc output} of tests/golden/planes_vectors.npz"""
    z = np.load(GOLDEN)
    index = json.loads(bytes(z["index"]).decode())
    return {(e["esize"], e["n"]): z["out"][e["at"]:e["at"] + e["n"]] for e in index}


def weights(m, esize, seed=7, sigma=0.02):
    """m seeded Gaussian weights N(0, sigma^2) as the bytes of bf16 (esize 2), fp32 (4) or fp64 (8) values, little endian"""
    w = np.random.default_rng(seed).normal(0.0, sigma, m)
    if esize == 8:
        return w.astype("<f8").view(np.uint8)
    b = w.astype("<f4").view(np.uint8)
    if esize == 4:
        return b.copy()
    return np.ascontiguousarray(b.reshape(m, 4)[:, 2:]).reshape(-1)   # bf16 by truncation: the two high bytes of the fp32 value


def mixed_weights(m, esize, chunk, t, seed=7):
    """weights(m) with every third chunk-span of ELEMENTS overwritten by uniform bytes (so that raw and coded chunks mix in every
    plane), followed by t tail bytes"""
    rng = np.random.default_rng(seed + 1)
    d = weights(m, esize, seed).reshape(m, esize).copy()
    for c in range(0, (m + chunk - 1) // chunk, 3):
        e0, e1 = c * chunk, min(m, (c + 1) * chunk)
        d[e0:e1] = rng.integers(0, 256, (e1 - e0, esize), dtype=np.uint8)
    return np.concatenate([d.reshape(-1), rng.integers(0, 256, t, dtype=np.uint8)])


def have_ref_sources():
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in ("transpose.c", "transpose_.c", "cpu.c"))


class Ref:
    """the reference's tpenc / tpdec, compiled into `outdir` by its makefile's recipe: transpose.c twice (-mavx -mpopcnt and
    -march=haswell), transpose_.c and cpu.c, all with -D_TRANSPOSE -D_NCPUISA"""

    def __init__(self, outdir):
        outdir = str(outdir)
        base = ["gcc", "-O3", "-w", "-fPIC", "-D_TRANSPOSE", "-D_NCPUISA", "-I" + REF_DIR]
        objs = []
        for src, extra, obj in (("transpose.c", ["-mavx", "-mpopcnt"], "transpose.o"), ("transpose.c", ["-march=haswell"], "transpose_avx2.o"),
                                ("transpose_.c", ["-mavx", "-mpopcnt"], "transpose_.o"), ("cpu.c", ["-mavx", "-mpopcnt"], "cpu.o")):
            objs.append(os.path.join(outdir, obj))
            subprocess.check_call(base + extra + ["-c", os.path.join(REF_DIR, src), "-o", objs[-1]])
        so = os.path.join(outdir, "libtrc_ref_tp.so")
        subprocess.check_call(["gcc", "-shared", "-o", so] + objs)
        self.lib = C.CDLL(so)
        for name in ("tpenc", "tpdec"):
            f = getattr(self.lib, name)
            f.restype = None
            f.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]

    def _call(self, name, data, esize):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        src = np.zeros(data.size + 256, dtype=np.uint8); src[:data.size] = data
        out = np.zeros(data.size + 256, dtype=np.uint8)
        getattr(self.lib, name)(src.ctypes.data, data.size, out.ctypes.data, esize)
        return out[:data.size].copy()

    def tpenc(self, data, esize):
        return self._call("tpenc", data, esize)

    def tpdec(self, data, esize):
        return self._call("tpdec", data, esize)
