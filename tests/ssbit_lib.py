"""Inputs and reference calls for the byte-level bitwise coders on the dual-rate "ss" predictor (rcss, rc4ss, rc4css, rcu3ss:
codecs TRC_RCSS = 62, TRC_RC4SS = 63, TRC_RC4CSS = 64, TRC_RCU3SS = 65).

The inputs are the six kinds of nibbit_lib.gen.  The reference's library build under oracle/_ref/ holds no "ss" function, so
build_ref(dir) compiles the two reference sources that make them (rc_ss.c; rc_s.c supplies mbc_c) into a directory of the
caller's, outside the repository, where the reference sources exist.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import nibbit_lib as N
import trc_testlib as T

RCSS, RC4SS, RC4CSS, RCU3SS = 62, 63, 64, 65
CODECS = [RCSS, RC4SS, RC4CSS, RCU3SS]
NAMES = {RCSS: "rcss", RC4SS: "rc4ss", RC4CSS: "rc4css", RCU3SS: "rcu3ss"}
REF_FN = {RCSS: ("rcssenc", "rcssdec"), RC4SS: ("rc4ssenc", "rc4ssdec"), RC4CSS: ("rc4cssenc", "rc4cssdec"),
          RCU3SS: ("rcu3ssenc", "rcu3ssdec")}
NIBBLE = (RC4SS, RC4CSS)                                       # code d & 15
KINDS = N.KINDS
DEFAULT = (5, 6)
PRMS = [(5, 6), (4, 7), (1, 1), (1, 9), (15, 15)]
REF_DIR = os.environ.get("TRC_REFERENCE", "/root/reference")
gen = N.gen


def prm_tag(prm):
    return "%d_%d" % tuple(prm)


def expected(codec, d, clen, chunk):
    """what a decoder returns for input d coded into the directory clen: the nibble coders keep the low nibble only, in the
    chunks they coded (a raw chunk holds the input bytes as they were)"""
    if codec not in NIBBLE:
        return d
    lens = np.minimum(chunk, d.size - np.arange(0, d.size, chunk))
    coded = np.repeat(np.asarray(clen) != lens, lens)
    return np.where(coded, d & 15, d).astype(np.uint8)


def load_fixtures(path):
    """-> (arrays, index) of tests/golden/ssbit_vectors.npz"""
    z = np.load(path)
    return {"clen": z["clen"], "out": z["out"]}, json.loads(bytes(z["index"]).decode())


def fixture(arrays, ent, codec, prm):
    """-> (clen, payload) of index entry `ent` for (codec, prm): slices of the two packed arrays"""
    c0, p0, plen = ent["at"][NAMES[codec]][prm_tag(prm)]
    nch = (ent["n"] + ent["chunk"] - 1) // ent["chunk"]
    return arrays["clen"][c0:c0 + nch], arrays["out"][p0:p0 + plen]


def have_ref_sources():
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in ("rc_ss.c", "rc_s.c", "rc_.c", "mbc_ss.h"))


class Ref:
    """the reference's eight functions, compiled into `outdir`"""

    def __init__(self, outdir):
        so = os.path.join(str(outdir), "libtrc_ref_ss.so")
        flags = ["-O3", "-w", "-fPIC", "-DNDEBUG", "-D_NCPUISA", "-mavx", "-mpopcnt", "-I" + REF_DIR]
        subprocess.check_call(["gcc"] + flags + ["-shared", os.path.join(REF_DIR, "rc_ss.c"), os.path.join(REF_DIR, "rc_s.c"), "-o", so])
        self.lib = C.CDLL(so)
        for codec in REF_FN:
            for name in REF_FN[codec]:
                f = getattr(self.lib, name)
                f.restype = C.c_size_t
                f.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_uint, C.c_uint]

    def enc(self, codec, data, prm=DEFAULT):
        """one call of the reference encoder on `data`, `in` below `out` in one arena (trc_testlib._arena)"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = data.size
        buf, io, oo = T._arena(n)
        buf[io:io + n] = data
        base = buf.ctypes.data
        l = getattr(self.lib, REF_FN[codec][0])(C.cast(base + io, C.POINTER(C.c_uint8)), n, C.cast(base + oo, C.POINTER(C.c_uint8)),
                                                prm[0], prm[1])
        return buf[oo:oo + l].copy()

    def chunked_enc(self, codec, data, chunk, prm=DEFAULT):
        """-> (clen u32 array, payload u8 array): the reference called once per chunk"""
        outs = [self.enc(codec, data[i:i + chunk], prm) for i in range(0, data.size, chunk)]
        clen = np.array([o.size for o in outs], dtype=np.uint32)
        payload = np.concatenate(outs) if outs else np.zeros(0, np.uint8)
        return clen, payload

    def dec(self, codec, comp, n, prm=DEFAULT):
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        if comp.size == n:
            return comp.copy()
        src = np.zeros(comp.size + 1024, dtype=np.uint8); src[:comp.size] = comp
        out = np.zeros(n + 64, dtype=np.uint8)
        getattr(self.lib, REF_FN[codec][1])(src.ctypes.data_as(C.POINTER(C.c_uint8)), n, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            prm[0], prm[1])
        return out[:n].copy()
