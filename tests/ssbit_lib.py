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
    """the reference's eight functions, compiled into `outdir`; every call takes prm=(prm0, prm1) behind its own arguments"""

    def __init__(self, outdir):
        so = os.path.join(str(outdir), "libtrc_ref_ss.so")
        flags = ["-O3", "-w", "-fPIC", "-DNDEBUG", "-D_NCPUISA", "-mavx", "-mpopcnt", "-I" + REF_DIR]
        subprocess.check_call(["gcc"] + flags + ["-shared", os.path.join(REF_DIR, "rc_ss.c"), os.path.join(REF_DIR, "rc_s.c"), "-o", so])
        self.calls = T.RefCalls(REF_FN, so, extra=(C.c_uint, C.c_uint))

    def enc(self, codec, data, prm=DEFAULT):
        return self.calls.enc(codec, data, *prm)

    def chunked_enc(self, codec, data, chunk, prm=DEFAULT):
        return self.calls.chunked_enc(codec, data, chunk, *prm)

    def dec(self, codec, comp, n, prm=DEFAULT):
        return self.calls.dec(codec, comp, n, *prm)
