"""ctypes binding of libturborc_hip.so for tests / bench.py (plumbing only).

The product is the C-ABI shared library (include/*.h).  This module only
  * builds/loads it (in-tree, so the GPU box sees the .so that was actually used),
  * wraps the device-resident entry points around torch tensors (torch = device memory + streams),
  * wraps the reference-signature host-pointer calls around numpy arrays.
There is no CPU fallback: loading fails loudly if the library is missing.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB = os.environ.get("TRC_LIB") or os.path.join(PKG, "libturborc_hip.so")   # TRC_LIB: A/B builds for ablations

ANS4S, RCS1, RCS2, RCA, ANSA, RCB, RCAI, RCA4, RCAI4, ANSA4, RCSM, ANSO1, ANSB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
VLCU16, VLCU32, VLCV16, VLCV32, VLCVZ16, VLCVZ32 = 14, 15, 16, 17, 18, 19   # Turbo-VLC integer coders
VLAU16, VLAUZ16, VLAV16, VLAVZ16, VLAV32, VLAVZ32 = 20, 21, 22, 23, 24, 25   # ... over the CDF rANS
RCV8, RCVI8 = 26, 27                                                          # "vnibble" coders (turborc -e48 / -e49)
RCC1, RCX1 = 28, 29                                                           # bitwise order-1 coders (turborc -e2 / -e4)
RCG8, RCG16, RCG32, RCGZ8, RCGZ16, RCGZ32 = 30, 31, 32, 33, 34, 35             # gamma integer coders (turborc -e26 / -e27)
RCR8, RCR16, RCR32, RCRZ8, RCRZ16, RCRZ32 = 36, 37, 38, 39, 40, 41             # Rice integer coders (turborc -e28 / -e29)
INTBIT = ((RCG8, 1), (RCG16, 2), (RCG32, 4), (RCGZ8, 1), (RCGZ16, 2), (RCGZ32, 4),   # (codec, element bytes); kept out of AVAILABLE
          (RCR8, 1), (RCR16, 2), (RCR32, 4), (RCRZ8, 1), (RCRZ16, 2), (RCRZ32, 4))   # and VLC_CODECS for the same reason as CTXBIT
RCBV16, RCBV32, RCBVZ16, RCBVZ32, RCBVG16, RCBVG32, RCBVGZ16, RCBVGZ32 = 43, 44, 45, 46, 47, 48, 49, 50   # Turbo-VLC on the bitwise coder (-e30/33/35/36)
BVLC = ((RCBV16, 2), (RCBV32, 4), (RCBVZ16, 2), (RCBVZ32, 4),        # (codec, element bytes); kept out of AVAILABLE and VLC_CODECS
        (RCBVG16, 2), (RCBVG32, 4), (RCBVGZ16, 2), (RCBVGZ32, 4))    # for the same reason as CTXBIT
RCW16, RCW32, RCCW32, RCC2W32 = 52, 53, 54, 55                                  # bitwise word coders (turborc -e6 / -e7 / -e8)
WORD = ((RCW16, 2), (RCW32, 4), (RCCW32, 4), (RCC2W32, 4))          # (codec, element bytes); kept out of AVAILABLE for the same reason as CTXBIT
RC4, RC4C, RCU3 = 58, 59, 60                                                    # bitwise nibble coders (turborc -n -e41 / -e40), 3/5/8-bit varint (-e17)
NIBBIT = ((RC4, 1), (RC4C, 1), (RCU3, 1))                           # (codec, element bytes); kept out of AVAILABLE for the same reason as CTXBIT
RCSS, RC4SS, RC4CSS, RCU3SS = 62, 63, 64, 65                                    # the same on the dual-rate "ss" predictor (turborc -pss -e1 / -n -e41 / -n -e40 / -e17)
SSBIT = (RCSS, RC4SS, RC4CSS, RCU3SS)                               # kept out of AVAILABLE for the same reason as CTXBIT; they take prm=(prm0, prm1)
CTXBIT = (RCC1, RCX1)      # HIP kernels too, kept out of AVAILABLE: the suites over AVAILABLE check parity against the oracle/ restatement,
                           # which has no order-1 bitwise coder; tests/test_gpu_ctxbit.py checks them against fixtures made through the reference
CODEC_NAMES = {ANS4S: "anscdf4s", RCS1: "rccdfs", RCS2: "rccdfs2", RCA: "rccdf", ANSA: "anscdf", RCB: "rcs", RCAI: "rccdfi",
               RCA4: "rccdf4", RCAI4: "rccdf4i", ANSA4: "anscdf4", RCSM: "rccdfsm", ANSO1: "anscdf1", ANSB: "ansb",
               VLCU16: "rccdfu16", VLCU32: "rccdfu32", VLCV16: "rccdfv16", VLCV32: "rccdfv32", VLCVZ16: "rccdfvz16", VLCVZ32: "rccdfvz32",
               VLAU16: "anscdfu16", VLAUZ16: "anscdfuz16", VLAV16: "anscdfv16", VLAVZ16: "anscdfvz16", VLAV32: "anscdfv32", VLAVZ32: "anscdfvz32",
               RCV8: "rccdf8", RCVI8: "rccdfi8", RCC1: "rccs", RCX1: "rcxs",
               RCG8: "rcgs8", RCG16: "rcgs16", RCG32: "rcgs32", RCGZ8: "rcgzs8", RCGZ16: "rcgzs16", RCGZ32: "rcgzs32",
               RCR8: "rcrs8", RCR16: "rcrs16", RCR32: "rcrs32", RCRZ8: "rcrzs8", RCRZ16: "rcrzs16", RCRZ32: "rcrzs32",
               RCBV16: "rcvs16", RCBV32: "rcvs32", RCBVZ16: "rcvzs16", RCBVZ32: "rcvzs32",
               RCBVG16: "rcvgs16", RCBVG32: "rcvgs32", RCBVGZ16: "rcvgzs16", RCBVGZ32: "rcvgzs32",
               RCW16: "rcs16", RCW32: "rcs32", RCCW32: "rccs32", RCC2W32: "rcc2s32",
               RC4: "rc4s", RC4C: "rc4cs", RCU3: "rcu3s", RCSS: "rcss", RC4SS: "rc4ss", RC4CSS: "rc4css", RCU3SS: "rcu3ss"}
VLC_CODECS = (VLCU16, VLCU32, VLCV16, VLCV32, VLCVZ16, VLCVZ32, VLAU16, VLAUZ16, VLAV16, VLAVZ16, VLAV32, VLAVZ32)
VLC_ELEM = {VLCU16: 2, VLCU32: 4, VLCV16: 2, VLCV32: 4, VLCVZ16: 2, VLCVZ32: 4,
            VLAU16: 2, VLAUZ16: 2, VLAV16: 2, VLAVZ16: 2, VLAV32: 4, VLAVZ32: 4}
NIBBLE_CODECS = (RCA4, RCAI4, ANSA4)                           # `turborc -n` coders: input values 0..15
STATIC = (ANS4S, RCS1, RCS2, RCSM)
TABLES_READY = 0x100                                          # include/trc_hip.h
DIR_READY = 0x200
AVAILABLE = (ANS4S, RCS1, RCS2, RCB, RCA, ANSA, RCAI, RCA4, RCAI4, ANSA4, RCSM, ANSO1, ANSB) + VLC_CODECS + (RCV8, RCVI8)          # codecs with HIP kernels behind them (grows per round)
PAD = 256
HDR = 32

_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_vp = C.c_void_p
_sz = C.c_size_t


class Range(C.Structure):
    """struct trc_range (include/trc_hip.h)"""
    _fields_ = [(f, C.c_uint64) for f in ("first_chunk", "nchunks", "payload_off", "payload_len", "out_skip", "out_bytes")]


class PlanesItem(C.Structure):
    """struct trc_planes_item (include/trc_hip.h)"""
    _fields_ = [("d_ptr", C.c_void_p), ("n", C.c_uint64)]


class PlanesBatchPlan(C.Structure):
    """struct trc_planes_batch_plan (include/trc_hip.h)"""
    _fields_ = [(f, C.c_uint64) for f in ("m_total", "n_virtual", "chunks", "pitch", "pad_elems")]


class PlanesBatchHdr(C.Structure):
    """struct trc_planes_batch_hdr (include/trc_hip.h)"""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint8), ("esize", C.c_uint8), ("zero", C.c_uint16), ("chunk", C.c_uint32),
                ("zero2", C.c_uint32), ("count", C.c_uint64), ("inner", C.c_uint64), ("size", C.c_uint64), ("bytes", C.c_uint64)]


class PlanesBatchLayout(C.Structure):
    """struct trc_planes_batch_layout (include/trc_hip.h)"""
    _fields_ = [("inner", C.c_uint64), ("off", C.c_uint64 * 8), ("size", C.c_uint64)]


class PlanesAdvice(C.Structure):
    """struct trc_planes_advice (include/trc_hip.h)"""
    _fields_ = [("filter", C.c_int), ("esize", C.c_uint), ("filters", C.c_uint), ("m", C.c_uint64),
                ("bits", C.c_double * 8 * 3), ("total_bits", C.c_double * 3)]


class PlanesOrderAdvice(C.Structure):
    """struct trc_planes_order_advice (include/trc_hip.h)"""
    _fields_ = [("order", C.c_int), ("esize", C.c_uint), ("orders", C.c_uint), ("m", C.c_uint64),
                ("bits", C.c_double * 8 * 4), ("total_bits", C.c_double * 4)]


def build(force=False):
    """Compile every HIP translation unit for gfx950 into turbo-range-coder_amd/libturborc_hip.so."""
    if force:
        subprocess.check_call(["make", "-s", "-C", PKG, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG])
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError("libturborc_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                               "there is no CPU fallback")
        # The process must end up with ONE HIP runtime.  PyTorch's wheel brings its own libamdhip64; if this library is
        # loaded first it pulls in /opt/rocm's copy, torch then loads its own, and device pointers of one runtime reach
        # launches of the other ("no ROCm-capable device is detected" on the first call).  With torch imported first the
        # library's dependency resolves to the runtime that is already there.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        l = C.CDLL(LIB)
        l.trc_last_error.restype = C.c_char_p
        l.trc_device_count.restype = C.c_int
        l.trc_set_chunk.restype = C.c_int; l.trc_set_chunk.argtypes = [C.c_uint32]
        l.trc_get_chunk.restype = C.c_uint32
        l.trc_round_chunk.restype = C.c_uint32; l.trc_round_chunk.argtypes = [C.c_int, _sz]
        l.trc_auto_chunk_codec.restype = C.c_uint32; l.trc_auto_chunk_codec.argtypes = [C.c_int, _sz]
        l.trc_work_bytes.restype = _sz; l.trc_work_bytes.argtypes = [C.c_int, _sz, C.c_uint32]
        l.trc_cdfini_dev.restype = C.c_int
        l.trc_cdfini_dev.argtypes = [_vp, _sz, _vp, C.c_uint, _vp, _vp, _vp]
        l.trc_hist_dev.restype = C.c_int; l.trc_hist_dev.argtypes = [_vp, _sz, _vp, _vp]
        l.trc_cdf_from_hist_dev.restype = C.c_int; l.trc_cdf_from_hist_dev.argtypes = [_vp, _sz, _vp, C.c_uint, _vp, _vp]
        l.trc_encode_dev.restype = C.c_int
        l.trc_encode_dev.argtypes = [C.c_int, _vp, _sz, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _sz, _vp]
        l.trc_tables_dev.restype = C.c_int
        l.trc_tables_dev.argtypes = [_vp, C.c_uint, _vp, _sz, _vp]
        l.trc_decode_dev.restype = C.c_int
        l.trc_decode_dev.argtypes = [C.c_int, _vp, _vp, _sz, C.c_uint32, _vp, C.c_uint, _vp, _vp, _sz, _vp]
        l.trc_range_work_bytes.restype = _sz; l.trc_range_work_bytes.argtypes = [C.c_int, _sz, C.c_uint32, _sz]
        l.trc_decode_range_dev.restype = C.c_int
        l.trc_decode_range_dev.argtypes = [C.c_int, _vp, _vp, _sz, C.c_uint32, _sz, _sz, _vp, C.c_uint, _vp, _vp, _sz, _vp]
        l.trc_container_range.restype = C.c_int
        l.trc_container_range.argtypes = [_vp, _sz, C.c_int, _sz, _sz, C.POINTER(Range)]
        l.trc_decode_range_host.restype = _sz
        l.trc_decode_range_host.argtypes = [C.c_int, _vp, _sz, _sz, _sz, _sz, _vp, _vp, C.c_uint]
        l.trc_planes_pitch.restype = _sz; l.trc_planes_pitch.argtypes = [_sz, C.c_uint]
        l.trc_planes_split_dev.restype = C.c_int; l.trc_planes_split_dev.argtypes = [_vp, _sz, C.c_uint, _vp, _sz, _vp, _vp]
        l.trc_planes_join_dev.restype = C.c_int; l.trc_planes_join_dev.argtypes = [_vp, _sz, _vp, _sz, C.c_uint, _vp, _vp]
        l.trc_planes_work_bytes.restype = _sz; l.trc_planes_work_bytes.argtypes = [C.c_int, _sz, C.c_uint, C.c_uint32]
        l.trc_planes_range_work_bytes.restype = _sz; l.trc_planes_range_work_bytes.argtypes = [C.c_int, _sz, C.c_uint, C.c_uint32, _sz]
        l.trc_encode_planes_dev.restype = C.c_int
        l.trc_encode_planes_dev.argtypes = [C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
        l.trc_decode_planes_dev.restype = C.c_int
        l.trc_decode_planes_dev.argtypes = [C.c_int, _vp, _vp, _vp, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _sz, _vp]
        l.trc_decode_planes_range_dev.restype = C.c_int
        l.trc_decode_planes_range_dev.argtypes = [C.c_int, _vp, _vp, _sz, C.c_uint, C.c_uint32, _sz, _sz, _vp, C.c_uint, _vp, _vp, _sz, _vp]
        l.trc_planes_bound.restype = _sz; l.trc_planes_bound.argtypes = [_sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_encode_planes_host.restype = _sz; l.trc_encode_planes_host.argtypes = [C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint]
        l.trc_decode_planes_host.restype = _sz; l.trc_decode_planes_host.argtypes = [_vp, _sz, _vp, _sz]
        l.trc_decode_planes_range_host.restype = _sz; l.trc_decode_planes_range_host.argtypes = [_vp, _sz, _sz, _sz, _vp]
        l.trc_planes_check.restype = C.c_int; l.trc_planes_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_split_filter_dev.restype = C.c_int
        l.trc_planes_split_filter_dev.argtypes = [C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, _vp, _vp]
        l.trc_planes_join_filter_dev.restype = C.c_int
        l.trc_planes_join_filter_dev.argtypes = [C.c_int, _vp, _sz, _vp, _sz, C.c_uint, C.c_uint32, _vp, _vp]
        l.trc_encode_fplanes_dev.restype = C.c_int; l.trc_encode_fplanes_dev.argtypes = [C.c_int, C.c_int] + l.trc_encode_planes_dev.argtypes[1:]
        l.trc_decode_fplanes_dev.restype = C.c_int; l.trc_decode_fplanes_dev.argtypes = [C.c_int, C.c_int] + l.trc_decode_planes_dev.argtypes[1:]
        l.trc_decode_fplanes_range_dev.restype = C.c_int
        l.trc_decode_fplanes_range_dev.argtypes = [C.c_int, C.c_int] + l.trc_decode_planes_range_dev.argtypes[1:]
        l.trc_fplanes_bound.restype = _sz; l.trc_fplanes_bound.argtypes = [_sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_encode_fplanes_host.restype = _sz; l.trc_encode_fplanes_host.argtypes = [C.c_int, C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint]
        l.trc_decode_fplanes_host.restype = _sz; l.trc_decode_fplanes_host.argtypes = [_vp, _sz, _vp, _sz]
        l.trc_decode_fplanes_range_host.restype = _sz; l.trc_decode_fplanes_range_host.argtypes = [_vp, _sz, _sz, _sz, _vp]
        l.trc_fplanes_check.restype = C.c_int; l.trc_fplanes_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_hist_bytes.restype = _sz; l.trc_planes_hist_bytes.argtypes = [C.c_uint]
        l.trc_planes_hist_dev.restype = C.c_int; l.trc_planes_hist_dev.argtypes = [C.c_uint, _vp, _sz, C.c_uint, C.c_uint32, _vp, _vp]
        l.trc_planes_advise.restype = C.c_int; l.trc_planes_advise.argtypes = [_vp, C.c_uint, C.c_uint, _sz, C.POINTER(PlanesAdvice)]
        l.trc_encode_aplanes_host.restype = _sz
        l.trc_encode_aplanes_host.argtypes = [C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint, C.POINTER(PlanesAdvice)]
        l.trc_decode_xplanes_host.restype = _sz; l.trc_decode_xplanes_host.argtypes = [_vp, _sz, _vp, _sz]
        l.trc_planes_split_sfilter_dev.restype = C.c_int
        l.trc_planes_split_sfilter_dev.argtypes = [C.c_int, C.c_int] + l.trc_planes_split_filter_dev.argtypes[1:]
        l.trc_planes_join_sfilter_dev.restype = C.c_int
        l.trc_planes_join_sfilter_dev.argtypes = [C.c_int, C.c_int] + l.trc_planes_join_filter_dev.argtypes[1:]
        l.trc_encode_splanes_dev.restype = C.c_int; l.trc_encode_splanes_dev.argtypes = [C.c_int, C.c_int, C.c_int] + l.trc_encode_planes_dev.argtypes[1:]
        l.trc_decode_splanes_dev.restype = C.c_int; l.trc_decode_splanes_dev.argtypes = [C.c_int, C.c_int, C.c_int] + l.trc_decode_planes_dev.argtypes[1:]
        l.trc_decode_splanes_range_dev.restype = C.c_int
        l.trc_decode_splanes_range_dev.argtypes = [C.c_int, C.c_int, C.c_int] + l.trc_decode_planes_range_dev.argtypes[1:]
        l.trc_planes_hist_stride_dev.restype = C.c_int
        l.trc_planes_hist_stride_dev.argtypes = [C.c_uint, C.c_int] + l.trc_planes_hist_dev.argtypes[1:]
        l.trc_splanes_bound.restype = _sz; l.trc_splanes_bound.argtypes = [_sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_encode_splanes_host.restype = _sz
        l.trc_encode_splanes_host.argtypes = [C.c_int, C.c_int, C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint]
        l.trc_decode_splanes_host.restype = _sz; l.trc_decode_splanes_host.argtypes = [_vp, _sz, _vp, _sz]
        l.trc_decode_splanes_range_host.restype = _sz; l.trc_decode_splanes_range_host.argtypes = [_vp, _sz, _sz, _sz, _vp]
        l.trc_splanes_check.restype = C.c_int; l.trc_splanes_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_split_ofilter_dev.restype = C.c_int; l.trc_planes_split_ofilter_dev.argtypes = l.trc_planes_split_sfilter_dev.argtypes
        l.trc_planes_join_ofilter_dev.restype = C.c_int; l.trc_planes_join_ofilter_dev.argtypes = l.trc_planes_join_sfilter_dev.argtypes
        l.trc_encode_oplanes_dev.restype = C.c_int; l.trc_encode_oplanes_dev.argtypes = l.trc_encode_splanes_dev.argtypes
        l.trc_decode_oplanes_dev.restype = C.c_int; l.trc_decode_oplanes_dev.argtypes = l.trc_decode_splanes_dev.argtypes
        l.trc_decode_oplanes_range_dev.restype = C.c_int; l.trc_decode_oplanes_range_dev.argtypes = l.trc_decode_splanes_range_dev.argtypes
        l.trc_planes_hist_order_bytes.restype = _sz; l.trc_planes_hist_order_bytes.argtypes = [C.c_uint]
        l.trc_planes_hist_order_dev.restype = C.c_int; l.trc_planes_hist_order_dev.argtypes = l.trc_planes_hist_stride_dev.argtypes
        l.trc_planes_advise_order.restype = C.c_int
        l.trc_planes_advise_order.argtypes = [_vp, C.c_uint, C.c_uint, _sz, C.POINTER(PlanesOrderAdvice)]
        l.trc_oplanes_bound.restype = _sz; l.trc_oplanes_bound.argtypes = [_sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_encode_oplanes_host.restype = _sz; l.trc_encode_oplanes_host.argtypes = l.trc_encode_splanes_host.argtypes
        l.trc_decode_oplanes_host.restype = _sz; l.trc_decode_oplanes_host.argtypes = [_vp, _sz, _vp, _sz]
        l.trc_decode_oplanes_range_host.restype = _sz; l.trc_decode_oplanes_range_host.argtypes = [_vp, _sz, _sz, _sz, _vp]
        l.trc_oplanes_check.restype = C.c_int; l.trc_oplanes_check.argtypes = [_vp, _sz, _sz]
        l.trc_encode_aoplanes_host.restype = _sz
        l.trc_encode_aoplanes_host.argtypes = [C.c_int, C.c_int, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint, C.POINTER(PlanesOrderAdvice)]
        l.trc_planes_split_base_dev.restype = C.c_int
        l.trc_planes_split_base_dev.argtypes = [C.c_int, _vp, _vp, _sz, C.c_uint, _vp, _sz, _vp, _vp]
        l.trc_planes_join_base_dev.restype = C.c_int
        l.trc_planes_join_base_dev.argtypes = [C.c_int, _vp, _sz, _vp, _vp, _sz, C.c_uint, _vp, _vp]
        l.trc_encode_bplanes_dev.restype = C.c_int
        l.trc_encode_bplanes_dev.argtypes = [C.c_int, C.c_int, _vp, _vp] + l.trc_encode_planes_dev.argtypes[2:]
        l.trc_decode_bplanes_dev.restype = C.c_int
        l.trc_decode_bplanes_dev.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp, _vp] + l.trc_decode_planes_dev.argtypes[4:]
        l.trc_decode_bplanes_range_dev.restype = C.c_int
        l.trc_decode_bplanes_range_dev.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp] + l.trc_decode_planes_range_dev.argtypes[3:]
        l.trc_planes_hist_base_dev.restype = C.c_int; l.trc_planes_hist_base_dev.argtypes = [C.c_uint, _vp, _vp, _sz, C.c_uint, _vp, _vp]
        l.trc_base_fingerprint_dev.restype = C.c_int; l.trc_base_fingerprint_dev.argtypes = [_vp, _sz, _vp, _vp]
        l.trc_base_fingerprint_host.restype = C.c_uint64; l.trc_base_fingerprint_host.argtypes = [_vp, _sz]
        l.trc_bplanes_bound.restype = _sz; l.trc_bplanes_bound.argtypes = [_sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_encode_bplanes_host.restype = _sz
        l.trc_encode_bplanes_host.argtypes = [C.c_int, C.c_int, _vp, _vp, _sz, C.c_uint, C.c_uint32, _vp, _sz, C.c_uint]
        l.trc_decode_bplanes_host.restype = _sz; l.trc_decode_bplanes_host.argtypes = [_vp, _sz, _vp, _sz, _vp, _sz]
        l.trc_decode_bplanes_range_host.restype = _sz; l.trc_decode_bplanes_range_host.argtypes = [_vp, _sz, _vp, _sz, _sz, _sz, _vp]
        l.trc_bplanes_check.restype = C.c_int; l.trc_bplanes_check.argtypes = [_vp, _sz, _sz]
        _it = C.POINTER(PlanesItem)
        l.trc_planes_batch_plan_host.restype = C.c_int
        l.trc_planes_batch_plan_host.argtypes = [_it, _sz, C.c_uint, C.c_uint32, C.POINTER(PlanesBatchPlan), C.POINTER(C.c_uint64)]
        l.trc_planes_batch_work_bytes.restype = _sz; l.trc_planes_batch_work_bytes.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32]
        l.trc_planes_batch_range_work_bytes.restype = _sz
        l.trc_planes_batch_range_work_bytes.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, _sz, _sz]
        l.trc_planes_batch_table_bytes.restype = _sz; l.trc_planes_batch_table_bytes.argtypes = [_sz, C.c_uint64]
        l.trc_planes_split_batch_dev.restype = C.c_int
        l.trc_planes_split_batch_dev.argtypes = [_it, _sz, C.c_uint, C.c_uint32, _vp, _sz, _vp, _sz, _vp]
        l.trc_planes_join_batch_dev.restype = C.c_int
        l.trc_planes_join_batch_dev.argtypes = [_vp, _sz, _it, _sz, _sz, _sz, C.c_uint, C.c_uint32, _vp, _sz, _vp]
        l.trc_encode_planes_batch_dev.restype = C.c_int
        l.trc_encode_planes_batch_dev.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
        l.trc_decode_planes_batch_dev.restype = C.c_int
        l.trc_decode_planes_batch_dev.argtypes = [C.c_int, _vp, _vp, _it, _sz, _sz, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _sz, _vp]
        _fl = C.POINTER(C.c_uint8)                  # the per-item filters of the filtered batch calls: a host array, or None
        l.trc_planes_split_fbatch_dev.restype = C.c_int
        l.trc_planes_split_fbatch_dev.argtypes = [_it, _fl] + l.trc_planes_split_batch_dev.argtypes[1:]
        l.trc_planes_join_fbatch_dev.restype = C.c_int
        l.trc_planes_join_fbatch_dev.argtypes = [_vp, _sz, _it, _fl] + l.trc_planes_join_batch_dev.argtypes[3:]
        l.trc_encode_fplanes_batch_dev.restype = C.c_int
        l.trc_encode_fplanes_batch_dev.argtypes = [C.c_int, _it, _fl] + l.trc_encode_planes_batch_dev.argtypes[2:]
        l.trc_decode_fplanes_batch_dev.restype = C.c_int
        l.trc_decode_fplanes_batch_dev.argtypes = [C.c_int, _vp, _vp, _it, _fl] + l.trc_decode_planes_batch_dev.argtypes[4:]
        _bs = C.POINTER(C.c_void_p)                 # the per-item bases of the batch calls against a base: a host array, or None
        l.trc_planes_split_bbatch_dev.restype = C.c_int
        l.trc_planes_split_bbatch_dev.argtypes = [_it, _bs, _fl] + l.trc_planes_split_batch_dev.argtypes[1:]
        l.trc_planes_join_bbatch_dev.restype = C.c_int
        l.trc_planes_join_bbatch_dev.argtypes = [_vp, _sz, _it, _bs, _fl] + l.trc_planes_join_batch_dev.argtypes[3:]
        l.trc_planes_bbatch_table_bytes.restype = _sz; l.trc_planes_bbatch_table_bytes.argtypes = [_sz, C.c_uint64]
        l.trc_planes_bbatch_work_bytes.restype = _sz; l.trc_planes_bbatch_work_bytes.argtypes = l.trc_planes_batch_work_bytes.argtypes
        l.trc_planes_bbatch_range_work_bytes.restype = _sz
        l.trc_planes_bbatch_range_work_bytes.argtypes = l.trc_planes_batch_range_work_bytes.argtypes
        l.trc_encode_bplanes_batch_dev.restype = C.c_int
        l.trc_encode_bplanes_batch_dev.argtypes = [C.c_int, _it, _bs, _fl] + l.trc_encode_planes_batch_dev.argtypes[2:]
        l.trc_decode_bplanes_batch_dev.restype = C.c_int
        l.trc_decode_bplanes_batch_dev.argtypes = [C.c_int, _vp, _vp, _it, _bs, _fl] + l.trc_decode_planes_batch_dev.argtypes[4:]
        _ad = C.POINTER(PlanesAdvice)               # the batch advisor: advice per item, or None
        l.trc_planes_hist_batch_bytes.restype = _sz; l.trc_planes_hist_batch_bytes.argtypes = [_sz, C.c_uint]
        l.trc_planes_hist_batch_dev.restype = C.c_int
        l.trc_planes_hist_batch_dev.argtypes = [C.c_uint, _it, _sz, _sz, _sz, C.c_uint, C.c_uint32, _vp, _vp, _sz, _vp]
        l.trc_planes_advise_batch.restype = C.c_int
        l.trc_planes_advise_batch.argtypes = [_vp, C.c_uint, C.c_uint, _it, _sz, _fl, _ad]
        l.trc_planes_advise_batch_work_bytes.restype = _sz; l.trc_planes_advise_batch_work_bytes.argtypes = [_it, _sz, C.c_uint, C.c_uint32]
        l.trc_planes_advise_batch_dev.restype = C.c_int
        l.trc_planes_advise_batch_dev.argtypes = [C.c_uint, _it, _sz, C.c_uint, C.c_uint32, _fl, _ad, _vp, _sz, _vp]
        l.trc_planes_split_sbatch_dev.restype = C.c_int        # ... and the per-item strides behind them: a host array, or None
        l.trc_planes_split_sbatch_dev.argtypes = [_it, _fl, _fl] + l.trc_planes_split_batch_dev.argtypes[1:]
        l.trc_planes_join_sbatch_dev.restype = C.c_int
        l.trc_planes_join_sbatch_dev.argtypes = [_vp, _sz, _it, _fl, _fl] + l.trc_planes_join_batch_dev.argtypes[3:]
        l.trc_encode_splanes_batch_dev.restype = C.c_int
        l.trc_encode_splanes_batch_dev.argtypes = [C.c_int, _it, _fl, _fl] + l.trc_encode_planes_batch_dev.argtypes[2:]
        l.trc_decode_splanes_batch_dev.restype = C.c_int
        l.trc_decode_splanes_batch_dev.argtypes = [C.c_int, _vp, _vp, _it, _fl, _fl] + l.trc_decode_planes_batch_dev.argtypes[4:]
        l.trc_planes_hist_sbatch_dev.restype = C.c_int
        l.trc_planes_hist_sbatch_dev.argtypes = [C.c_uint, _it, _fl] + l.trc_planes_hist_batch_dev.argtypes[2:]
        l.trc_planes_advise_sbatch_dev.restype = C.c_int
        l.trc_planes_advise_sbatch_dev.argtypes = [C.c_uint, _it, _fl] + l.trc_planes_advise_batch_dev.argtypes[2:]
        l.trc_planes_sbatch_bound.restype = _sz; l.trc_planes_sbatch_bound.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, C.c_uint]
        # ... and the per-item predictor orders behind the strides: a host array, or None
        l.trc_planes_split_obatch_dev.restype = C.c_int
        l.trc_planes_split_obatch_dev.argtypes = [_it, _fl, _fl, _fl] + l.trc_planes_split_batch_dev.argtypes[1:]
        l.trc_planes_join_obatch_dev.restype = C.c_int
        l.trc_planes_join_obatch_dev.argtypes = [_vp, _sz, _it, _fl, _fl, _fl] + l.trc_planes_join_batch_dev.argtypes[3:]
        l.trc_encode_oplanes_batch_dev.restype = C.c_int
        l.trc_encode_oplanes_batch_dev.argtypes = [C.c_int, _it, _fl, _fl, _fl] + l.trc_encode_planes_batch_dev.argtypes[2:]
        l.trc_decode_oplanes_batch_dev.restype = C.c_int
        l.trc_decode_oplanes_batch_dev.argtypes = [C.c_int, _vp, _vp, _it, _fl, _fl, _fl] + l.trc_decode_planes_batch_dev.argtypes[4:]
        l.trc_planes_hist_obatch_bytes.restype = _sz; l.trc_planes_hist_obatch_bytes.argtypes = [_sz, C.c_uint]
        l.trc_planes_hist_obatch_dev.restype = C.c_int
        l.trc_planes_hist_obatch_dev.argtypes = [C.c_uint, _it, _fl] + l.trc_planes_hist_batch_dev.argtypes[2:]
        l.trc_planes_advise_obatch.restype = C.c_int
        l.trc_planes_advise_obatch.argtypes = [_vp, C.c_uint, C.c_uint, _it, _sz, _fl, _fl, C.POINTER(PlanesOrderAdvice)]
        l.trc_planes_advise_obatch_work_bytes.restype = _sz
        l.trc_planes_advise_obatch_work_bytes.argtypes = l.trc_planes_advise_batch_work_bytes.argtypes
        l.trc_planes_advise_obatch_dev.restype = C.c_int
        l.trc_planes_advise_obatch_dev.argtypes = [C.c_uint, _it, _fl, _sz, C.c_uint, C.c_uint32, _fl, _fl, C.POINTER(PlanesOrderAdvice), _vp, _sz, _vp]
        l.trc_planes_obatch_bound.restype = _sz; l.trc_planes_obatch_bound.argtypes = l.trc_planes_sbatch_bound.argtypes
        l.trc_planes_obatch_check.restype = C.c_int; l.trc_planes_obatch_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_obatch_info.restype = C.c_int
        l.trc_planes_obatch_info.argtypes = [_vp, _sz, C.POINTER(PlanesBatchHdr), C.POINTER(C.c_uint64), _fl, _fl, _fl, _sz]
        l.trc_planes_obatch_pack_dev.restype = C.c_int
        l.trc_planes_obatch_pack_dev.argtypes = [C.c_int, _it, _fl, _fl, _fl, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
        l.trc_planes_sbatch_check.restype = C.c_int; l.trc_planes_sbatch_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_sbatch_info.restype = C.c_int
        l.trc_planes_sbatch_info.argtypes = [_vp, _sz, C.POINTER(PlanesBatchHdr), C.POINTER(C.c_uint64), _fl, _fl, _sz]
        l.trc_planes_sbatch_pack_dev.restype = C.c_int
        l.trc_planes_sbatch_pack_dev.argtypes = [C.c_int, _it, _fl, _fl, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
        l.trc_decode_splanes_batch_packed_dev.restype = C.c_int
        l.trc_decode_splanes_batch_packed_dev.argtypes = [C.c_int, _vp, _sz, _it, _fl, _fl, _sz, _sz, _sz, C.c_uint, C.c_uint32, C.c_uint,
                                                          C.POINTER(C.c_uint64), _vp, _sz, _vp]
        l.trc_encode_splanes_batch_host.restype = _sz
        l.trc_encode_splanes_batch_host.argtypes = [C.c_int, _it, _fl, _fl, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz]
        l.trc_decode_splanes_batch_host.restype = _sz
        l.trc_decode_splanes_batch_host.argtypes = [_vp, _sz, _it, _sz, _sz, _sz, C.c_int]
        l.trc_decode_oplanes_batch_packed_dev.restype = C.c_int
        l.trc_decode_oplanes_batch_packed_dev.argtypes = [C.c_int, _vp, _sz, _it, _fl, _fl, _fl, _sz, _sz, _sz, C.c_uint, C.c_uint32, C.c_uint,
                                                          C.POINTER(C.c_uint64), _vp, _sz, _vp]
        l.trc_encode_oplanes_batch_host.restype = _sz
        l.trc_encode_oplanes_batch_host.argtypes = [C.c_int, _it, _fl, _fl, _fl, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz]
        l.trc_decode_oplanes_batch_host.restype = _sz
        l.trc_decode_oplanes_batch_host.argtypes = [_vp, _sz, _it, _sz, _sz, _sz, C.c_int]
        l.trc_encode_aoplanes_batch_host.restype = _sz
        l.trc_encode_aoplanes_batch_host.argtypes = [C.c_int, _it, _fl, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz, _fl, _fl]
        l.trc_base_fingerprint_batch_table_bytes.restype = _sz; l.trc_base_fingerprint_batch_table_bytes.argtypes = [_sz]
        l.trc_base_fingerprint_batch_dev.restype = C.c_int
        l.trc_base_fingerprint_batch_dev.argtypes = [_it, _bs, _fl, _sz, _sz, _sz, _vp, _vp, _sz, _vp]
        l.trc_base_verify_batch_dev.restype = C.c_int
        l.trc_base_verify_batch_dev.argtypes = [_vp, _it, _bs, _fl, _sz, _sz, _sz, _vp, _vp, _sz, _vp]
        l.trc_planes_bbatch_bound.restype = _sz; l.trc_planes_bbatch_bound.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_planes_bbatch_check.restype = C.c_int; l.trc_planes_bbatch_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_bbatch_info.restype = C.c_int
        l.trc_planes_bbatch_info.argtypes = [_vp, _sz, C.POINTER(PlanesBatchHdr), C.POINTER(C.c_uint64), _fl, C.POINTER(C.c_uint64), _sz]
        l.trc_planes_bbatch_pack_dev.restype = C.c_int
        l.trc_planes_bbatch_pack_dev.argtypes = [C.c_int, _it, _bs, _fl, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp]
        l.trc_decode_bplanes_batch_packed_dev.restype = C.c_int
        l.trc_decode_bplanes_batch_packed_dev.argtypes = [C.c_int, _vp, _sz, _it, _bs, _fl, _sz, _sz, _sz, C.c_uint, C.c_uint32, C.c_uint,
                                                          C.POINTER(C.c_uint64), _vp, _sz, _vp]
        l.trc_planes_hist_bbatch_dev.restype = C.c_int
        l.trc_planes_hist_bbatch_dev.argtypes = [C.c_uint, _it, _bs] + l.trc_planes_hist_batch_dev.argtypes[2:]
        l.trc_planes_advise_bbatch.restype = C.c_int
        l.trc_planes_advise_bbatch.argtypes = [_vp, C.c_uint, C.c_uint, _it, _bs, _sz, _fl, _ad]
        l.trc_planes_advise_bbatch_dev.restype = C.c_int
        l.trc_planes_advise_bbatch_dev.argtypes = [C.c_uint, _it, _bs] + l.trc_planes_advise_batch_dev.argtypes[2:]
        l.trc_encode_bplanes_batch_host.restype = _sz
        l.trc_encode_bplanes_batch_host.argtypes = [C.c_int, _it, _bs, _fl, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz]
        l.trc_encode_abplanes_batch_host.restype = _sz
        l.trc_encode_abplanes_batch_host.argtypes = [C.c_int, _it, _bs, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz, _fl]
        l.trc_decode_bplanes_batch_host.restype = _sz
        l.trc_decode_bplanes_batch_host.argtypes = [_vp, _sz, _it, _bs, _sz, _sz, _sz, C.c_int]
        l.trc_planes_batch_auto_chunk.restype = C.c_uint32; l.trc_planes_batch_auto_chunk.argtypes = [C.c_int, _it, _sz, C.c_uint]
        l.trc_planes_batch_bound.restype = _sz; l.trc_planes_batch_bound.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, C.c_uint]
        l.trc_planes_batch_layout_host.restype = C.c_int
        l.trc_planes_batch_layout_host.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, C.c_uint, C.POINTER(C.c_uint64), C.POINTER(PlanesBatchLayout)]
        l.trc_planes_batch_check.restype = C.c_int; l.trc_planes_batch_check.argtypes = [_vp, _sz, _sz]
        l.trc_planes_batch_info.restype = C.c_int
        l.trc_planes_batch_info.argtypes = [_vp, _sz, C.POINTER(PlanesBatchHdr), C.POINTER(C.c_uint64), _fl, _sz]
        l.trc_planes_batch_pack_dev.restype = C.c_int
        l.trc_planes_batch_pack_dev.argtypes = [C.c_int, _it, _fl, _sz, C.c_uint, C.c_uint32, _vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
        l.trc_decode_planes_batch_packed_dev.restype = C.c_int
        l.trc_decode_planes_batch_packed_dev.argtypes = [C.c_int, _vp, _sz, _it, _fl, _sz, _sz, _sz, C.c_uint, C.c_uint32, C.c_uint,
                                                         C.POINTER(C.c_uint64), _vp, _sz, _vp]
        l.trc_encode_planes_batch_host.restype = _sz
        l.trc_encode_planes_batch_host.argtypes = [C.c_int, _it, _fl, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz]
        l.trc_encode_aplanes_batch_host.restype = _sz
        l.trc_encode_aplanes_batch_host.argtypes = [C.c_int, _it, _sz, C.c_uint, C.c_uint32, C.c_uint, C.c_int, _vp, _sz, _fl]
        l.trc_decode_planes_batch_host.restype = _sz
        l.trc_decode_planes_batch_host.argtypes = [_vp, _sz, _it, _sz, _sz, _sz, C.c_int]
        l.trc_encode_host.restype = _sz; l.trc_encode_host.argtypes = [C.c_int, _vp, _sz, C.c_uint32, _vp, _sz, _vp, C.c_uint]
        l.trc_decode_host.restype = _sz; l.trc_decode_host.argtypes = [C.c_int, _vp, _sz, _vp, _sz, _vp, C.c_uint]
        l.trc_container_bound.restype = _sz; l.trc_container_bound.argtypes = [_sz, C.c_uint32]
        l.trc_container_check.restype = C.c_int; l.trc_container_check.argtypes = [_vp, _sz, C.c_int, _sz]
        l.trc_host_plan.restype = C.c_int
        l.trc_host_plan.argtypes = [C.c_int, _sz, C.c_uint32, C.c_int, C.c_int, C.POINTER(_sz), C.c_int, C.POINTER(C.c_uint32)]
        l.trc_host_pin.restype = C.c_int; l.trc_host_pin.argtypes = [_vp, _sz]
        l.trc_host_unpin.restype = C.c_int; l.trc_host_unpin.argtypes = [_vp]
        l.trc_timing_enable.restype = C.c_int; l.trc_timing_enable.argtypes = [C.c_int]
        l.trc_timing_pause.restype = C.c_int; l.trc_timing_pause.argtypes = [C.c_int]
        l.trc_timing_read.restype = C.c_int
        l.trc_timing_read.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        l.trc_kernel_name.restype = C.c_char_p; l.trc_kernel_name.argtypes = [C.c_int, C.c_int]
        l.trc_set_devices.restype = C.c_int; l.trc_set_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
        l.trc_get_devices.restype = C.c_int; l.trc_get_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
        _lib = l
    return _lib


class TrcError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise TrcError("libturborc_hip rc=%d: %s" % (rc, lib().trc_last_error().decode()))


def timing_enable(on=True):
    _chk(lib().trc_timing_enable(1 if on else 0))


def timing_pause(paused=True):
    """suspend / resume the event pairs without resetting what has been collected"""
    _chk(lib().trc_timing_pause(1 if paused else 0))


def timing_read(decode):
    """-> (total_ms, launches) of the coder kernels since timing_enable(); decode = 2: the encode path's scan + gather kernels"""
    ms, cnt = C.c_double(0), C.c_int(0)
    _chk(lib().trc_timing_read(2 if decode == 2 else 1 if decode else 0, C.byref(ms), C.byref(cnt)))
    return ms.value, cnt.value


def ss_prm(prm):
    """TRC_SS_PRM(prm0, prm1) of include/trc_hip.h: the `cdfnum` of an "ss" coder's call"""
    return int(prm[0]) | int(prm[1]) << 8


def _cdfnum(codec, cdfnum, prm):
    """what a call passes as cdfnum: the alphabet size (static coders), the two parameters (ss coders), else 0"""
    return cdfnum if codec in STATIC else ss_prm(prm) if codec in SSBIT else 0


def nchunks(n, chunk):
    return (n + chunk - 1) // chunk


def range_work_bytes(codec, n, chunk, count):
    """bytes of the workspace trc_decode_range_dev needs for `count` chunks of an (n, chunk) container; 0: bad arguments"""
    return lib().trc_range_work_bytes(codec, n, chunk, count)


# ---------------------------------------------------------------- device-resident layer (torch) ---
class DeviceCoder:
    """Pre-allocated HBM buffers for repeated encode/decode of up to `n` bytes on the current device."""

    def __init__(self, codec, n, chunk=4096, device="cuda"):
        import torch
        self.torch = torch
        self.codec, self.n, self.chunk = codec, n, chunk
        self.nch = nchunks(n, chunk)
        self.dev = torch.device(device)
        u8 = torch.uint8
        self.work_bytes = lib().trc_work_bytes(codec, n, chunk)
        if self.work_bytes == 0:
            raise TrcError("bad (codec, n, chunk)")
        self.work = torch.empty(self.work_bytes + PAD, dtype=u8, device=self.dev)
        self.clen = torch.zeros(max(self.nch, 1) + 64, dtype=torch.int32, device=self.dev)
        self.payload = torch.zeros(n + PAD + 64, dtype=u8, device=self.dev)
        self.total = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.cdf = torch.zeros(264, dtype=torch.int16, device=self.dev)
        self.status = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self.cdfnum = 0
        self.tables_ready = 0                                  # TABLES_READY once trc_tables_dev ran for the current CDF
        self.range_work, self.range_work_bytes = None, 0       # decode_range's own workspace, made at its first call
        self.range_tables = 0                                  # ... and TABLES_READY for it

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _tables(self):
        """derive the coder tables from the current CDF once (enqueued), instead of at every encode/decode"""
        if self.codec in STATIC:
            _chk(lib().trc_tables_dev(self.cdf.data_ptr(), self.cdfnum, self.work.data_ptr(), self.work_bytes, self._stream()))
            self.tables_ready = TABLES_READY
            self.range_tables = 0

    def set_cdf(self, cdf_np, cdfnum):
        t = self.torch.from_numpy(np.ascontiguousarray(cdf_np[:cdfnum + 1]).view(np.int16))
        self.cdf[:cdfnum + 1].copy_(t)
        self.cdfnum = cdfnum
        self._tables()

    def cdfini(self, d_in, n, cdfnum):
        """Device cdfini: histogram of d_in[:n] -> self.cdf (stays on device)."""
        _chk(lib().trc_cdfini_dev(d_in.data_ptr(), n, self.cdf.data_ptr(), cdfnum, self.status.data_ptr(),
                                  self.work.data_ptr(), self._stream()))
        self.cdfnum = cdfnum
        self._tables()

    def hist(self, d_in, n, d_hist):
        """byte histogram of d_in[:n] into d_hist (int64[256] device tensor)"""
        _chk(lib().trc_hist_dev(d_in.data_ptr(), n, d_hist.data_ptr(), self._stream()))

    def cdf_from_hist(self, d_hist, n_total, cdfnum):
        _chk(lib().trc_cdf_from_hist_dev(d_hist.data_ptr(), n_total, self.cdf.data_ptr(), cdfnum, self.status.data_ptr(), self._stream()))
        self.cdfnum = cdfnum
        self._tables()

    def encode(self, d_in, n=None, prm=(5, 6)):
        """Enqueue encode of d_in[:n]; results in self.clen / self.payload / self.total (device).  prm: the two shift
        parameters of an "ss" coder (SSBIT), unused by every other one."""
        n = self.n if n is None else n
        st = self.codec in STATIC
        _chk(lib().trc_encode_dev(self.codec | self.tables_ready, d_in.data_ptr(), n, self.chunk,
                                  self.cdf.data_ptr() if st else None, _cdfnum(self.codec, self.cdfnum, prm),
                                  self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(),
                                  self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode(self, d_out, n=None, clen=None, payload=None, dir_ready=False, prm=(5, 6)):
        """dir_ready: the workspace still holds the group sums of `clen` (the encode or decode just before this call
        was for the same directory): TRC_DIR_READY, include/trc_hip.h"""
        n = self.n if n is None else n
        st = self.codec in STATIC
        clen = self.clen if clen is None else clen
        payload = self.payload if payload is None else payload
        _chk(lib().trc_decode_dev(self.codec | self.tables_ready | (DIR_READY if dir_ready else 0), clen.data_ptr(), payload.data_ptr(), n, self.chunk,
                                  self.cdf.data_ptr() if st else None, _cdfnum(self.codec, self.cdfnum, prm),
                                  d_out.data_ptr(), self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode_range(self, d_out, first, count, n=None, clen=None, payload=None, dir_ready=False, prm=(5, 6)):
        """Enqueue the decode of chunks [first, first + count) of the container (clen, payload, n) to d_out[0:], in a workspace
        of its own (trc_range_work_bytes; it grows with the largest count seen).  dir_ready: the decode_range before this one
        was for the same n and an unchanged clen, any first and count (TRC_DIR_READY, include/trc_hip.h); dropped when the
        workspace has just grown and the index with it."""
        n = self.n if n is None else n
        st = self.codec in STATIC
        clen = self.clen if clen is None else clen
        payload = self.payload if payload is None else payload
        need = lib().trc_range_work_bytes(self.codec, n, self.chunk, count)
        if need > self.range_work_bytes:
            self.range_work = self.torch.empty(need + PAD, dtype=self.torch.uint8, device=self.dev)
            self.range_work_bytes, self.range_tables, dir_ready = need, 0, False
        if st and not self.range_tables and self.range_work is not None:
            _chk(lib().trc_tables_dev(self.cdf.data_ptr(), self.cdfnum, self.range_work.data_ptr(), self.range_work_bytes, self._stream()))
            self.range_tables = TABLES_READY
        _chk(lib().trc_decode_range_dev(self.codec | self.range_tables | (DIR_READY if dir_ready else 0), clen.data_ptr(), payload.data_ptr(),
                                        n, self.chunk, first, count, self.cdf.data_ptr() if st else None, _cdfnum(self.codec, self.cdfnum, prm),
                                        d_out.data_ptr(), self.range_work.data_ptr() if self.range_work is not None else None,
                                        self.range_work_bytes, self._stream()))

    def result(self, n=None):
        """Synchronise and fetch (clen[nchunks] u32, payload bytes) to the host."""
        n = self.n if n is None else n
        nch = nchunks(n, self.chunk)
        self.torch.cuda.synchronize(self.dev)
        tot = int(self.total[0].item())
        clen = self.clen[:nch].cpu().numpy().view(np.uint32).copy()
        payload = self.payload[:tot].cpu().numpy().copy()
        return clen, payload


# ------------------------------------------------------------------- byte planes (include/trc_hip.h) ---
PLANES_MAGIC = 0x50435254                                      # "TRCP"
PLANES_CDF_STRIDE = 264
PLANES_HDR = 32


def planes_pitch(n, esize):
    """bytes from plane k to plane k + 1 in the coded planar calls: n // esize + PAD rounded up to 256; 0: bad arguments"""
    return lib().trc_planes_pitch(n, esize)


def _cur_stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def planes_split(d_in, n, esize, d_planes, pitch, d_tail=None):
    """enqueue trc_planes_split_dev: d_in[:n] (uint8 tensor) -> plane k at d_planes[k * pitch:], the n % esize tail bytes to d_tail"""
    _chk(lib().trc_planes_split_dev(d_in.data_ptr(), n, esize, d_planes.data_ptr(), pitch,
                                    d_tail.data_ptr() if d_tail is not None else None, _cur_stream(d_in)))


def planes_join(d_planes, pitch, d_tail, n, esize, d_out):
    """enqueue trc_planes_join_dev, the inverse of planes_split"""
    _chk(lib().trc_planes_join_dev(d_planes.data_ptr(), pitch, d_tail.data_ptr() if d_tail is not None else None, n, esize,
                                   d_out.data_ptr(), _cur_stream(d_out)))


class PlanesCoder:
    """Pre-allocated HBM buffers for the planar calls on up to n bytes of esize-byte elements: plane k's directory at
    self.clen[k * nch:], its payload at self.payload[k * pitch:], its size in self.total[k], its CDF (static coders, built by
    encode) at self.cdf[k * PLANES_CDF_STRIDE:], the tail bytes in self.tail."""
    _ENC, _DEC, _DEC_RANGE = "trc_encode_planes_dev", "trc_decode_planes_dev", "trc_decode_planes_range_dev"

    def __init__(self, codec, n, esize, chunk=4096, device="cuda", cdfnum=256, prm=(5, 6), guard=0):
        """guard: that many bytes of 0xA5 behind every buffer and its TRC_PAD slack; guards_ok() tells whether they survived"""
        import torch
        self.torch = torch
        self.codec, self.n, self.esize, self.chunk = codec, n, esize, chunk
        self.m = n // esize
        self.nch = nchunks(self.m, chunk)
        self.pitch = planes_pitch(n, esize)
        self.dev = torch.device(device)
        self.cdfnum = _cdfnum(codec, cdfnum, prm)
        self.work_bytes = lib().trc_planes_work_bytes(codec, n, esize, chunk)
        if self.work_bytes == 0:
            raise TrcError("bad (codec, n, esize, chunk)")
        self.guard, self._guards = guard, []
        self.work = self._buf(self.work_bytes)
        self.clen = self._buf(4 * esize * self.nch)
        self.payload = self._buf(esize * self.pitch)
        self.total = self._buf(8 * esize)
        self.tail = self._buf(8)
        self.cdf = self._buf(2 * esize * PLANES_CDF_STRIDE)
        self.status = self._buf(4 * esize)
        self.range_work, self.range_work_bytes = None, 0

    def _lead(self):
        """what the calls take between the codec and the first pointer"""
        return ()

    def _buf(self, nbytes):
        """nbytes + PAD zero bytes on the device (uint8), followed by the guard"""
        t = self.torch.zeros(nbytes + PAD + self.guard, dtype=self.torch.uint8, device=self.dev)
        if self.guard:
            t[nbytes + PAD:] = 0xA5
            self._guards.append(t[nbytes + PAD:])
        return t

    def guards_ok(self):
        self.torch.cuda.synchronize(self.dev)
        return all(bool((g == 0xA5).all().item()) for g in self._guards)

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def encode(self, d_in, n=None, flags=0):
        n = self.n if n is None else n
        st = self.codec in STATIC
        _chk(getattr(lib(), self._ENC)(self.codec | flags, *self._lead(), d_in.data_ptr(), n, self.esize, self.chunk,
                                       self.cdf.data_ptr() if st else None, self.cdfnum, self.status.data_ptr() if st else None,
                                       self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(), self.tail.data_ptr(),
                                       self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode(self, d_out, n=None, flags=0):
        n = self.n if n is None else n
        _chk(getattr(lib(), self._DEC)(self.codec | flags, *self._lead(), self.clen.data_ptr(), self.payload.data_ptr(), self.tail.data_ptr(),
                                       n, self.esize, self.chunk, self.cdf.data_ptr() if self.codec in STATIC else None, self.cdfnum,
                                       d_out.data_ptr(), self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode_range(self, d_out, first, count, n=None, flags=0):
        """elements [first * chunk, min(m, (first + count) * chunk)) to d_out[0:], in a workspace of its own that grows with count"""
        n = self.n if n is None else n
        need = lib().trc_planes_range_work_bytes(self.codec, n, self.esize, self.chunk, count)
        if need > self.range_work_bytes:
            self.range_work, self.range_work_bytes = self._buf(need), need
        if self.range_work is None:                            # nothing to size a workspace by: the call rejects these arguments itself
            self.range_work = self._buf(0)
        _chk(getattr(lib(), self._DEC_RANGE)(self.codec | flags, *self._lead(), self.clen.data_ptr(), self.payload.data_ptr(), n, self.esize,
                                             self.chunk, first, count, self.cdf.data_ptr() if self.codec in STATIC else None, self.cdfnum,
                                             d_out.data_ptr(), self.range_work.data_ptr(), self.range_work_bytes, self._stream()))

    def cdf_of(self, k):
        """Synchronise and fetch plane k's CDF (uint16[cdfnum + 1]) and cdfini status, as encode left them (static coders)"""
        self.torch.cuda.synchronize(self.dev)
        cdf = self.cdf[:2 * self.esize * PLANES_CDF_STRIDE].cpu().numpy().view("<u2")
        status = self.status[:4 * self.esize].cpu().numpy().view("<i4")
        return cdf[k * PLANES_CDF_STRIDE:k * PLANES_CDF_STRIDE + self.cdfnum + 1].copy(), int(status[k])

    def result(self, k):
        """Synchronise and fetch plane k's (clen[nch] u32, payload bytes, total) to the host."""
        self.torch.cuda.synchronize(self.dev)
        tot = int(self.total[:8 * self.esize].cpu().numpy().view("<u8")[k])
        clen = self.clen[4 * k * self.nch:4 * (k + 1) * self.nch].cpu().numpy().view(np.uint32).copy()
        payload = self.payload[k * self.pitch:k * self.pitch + tot].cpu().numpy().copy()
        return clen, payload, tot


# ------------------------------------------------------- batched byte planes (include/trc_hip.h) ---
PLANES_BATCH_MAX = 1 << 20


def planes_items(pairs):
    """a trc_planes_item array (host) of (device address or None, bytes) pairs"""
    arr = (PlanesItem * max(len(pairs), 1))()
    for i, (ptr, n) in enumerate(pairs):
        arr[i].d_ptr, arr[i].n = ptr, n
    return arr


def planes_batch_plan(items, count, esize, chunk):
    """trc_planes_batch_plan_host (needs no device) -> (dict of the plan's fields, first_chunk: list of count + 1)"""
    p = PlanesBatchPlan()
    first = (C.c_uint64 * (count + 1))()
    _chk(lib().trc_planes_batch_plan_host(items, count, esize, chunk, C.byref(p), first))
    return {f: int(getattr(p, f)) for f, _ in PlanesBatchPlan._fields_}, list(first)


def planes_split_batch(items, count, esize, chunk, d_planes, pitch, d_table, table_bytes):
    """enqueue trc_planes_split_batch_dev: the planes of the items' virtual buffer, plane k at d_planes[k * pitch:]"""
    _chk(lib().trc_planes_split_batch_dev(items, count, esize, chunk, d_planes.data_ptr(), pitch, d_table.data_ptr(), table_bytes,
                                          _cur_stream(d_planes)))


def planes_join_batch(d_planes, offset, pitch, items, count, first_item, item_count, esize, chunk, d_table, table_bytes):
    """enqueue trc_planes_join_batch_dev from d_planes[offset:] (offset = first_chunk[first_item] * chunk into a whole batch's planes)"""
    _chk(lib().trc_planes_join_batch_dev(d_planes.data_ptr() + offset, pitch, items, count, first_item, item_count, esize, chunk,
                                         d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def _byte_per_item(what, values, count):
    """None, one int for every item or a sequence of `count` ints as the host array of bytes the batch calls take"""
    if values is None:
        return None
    v = [values] * count if isinstance(values, int) else [int(x) for x in values]
    if len(v) != count or any(not 0 <= x <= 255 for x in v):
        raise TrcError("%s: one byte per item of the batch" % what)
    return (C.c_uint8 * max(count, 1))(*v)


def planes_filters(filters, count):
    """the per-item filters of a batch as the host array the filtered batch calls take: None (no filter), one int for every item,
    or a sequence of `count` ints.  Values are not judged here: the library does that."""
    return _byte_per_item("filters", filters, count)


def planes_split_fbatch(items, filters, count, esize, chunk, d_planes, pitch, d_table, table_bytes):
    """enqueue trc_planes_split_fbatch_dev: planes_split_batch of the items filtered one by one (filters: see planes_filters)"""
    _chk(lib().trc_planes_split_fbatch_dev(items, planes_filters(filters, count), count, esize, chunk, d_planes.data_ptr(), pitch,
                                           d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_join_fbatch(d_planes, offset, pitch, items, filters, count, first_item, item_count, esize, chunk, d_table, table_bytes):
    """enqueue trc_planes_join_fbatch_dev from d_planes[offset:], the inverse of planes_split_fbatch (filters: those of the whole batch)"""
    _chk(lib().trc_planes_join_fbatch_dev(d_planes.data_ptr() + offset, pitch, items, planes_filters(filters, count), count, first_item,
                                          item_count, esize, chunk, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_strides(strides, count):
    """the per-item strides of a batch as the host array the strided batch calls take: None (stride 1), one int for every item, or a
    sequence of `count` ints.  Values are not judged here: the library does that."""
    return _byte_per_item("strides", strides, count)


def planes_split_sbatch(items, filters, strides, count, esize, chunk, d_planes, pitch, d_table, table_bytes):
    """enqueue trc_planes_split_sbatch_dev: planes_split_fbatch with item i predicted from the element strides[i] back"""
    _chk(lib().trc_planes_split_sbatch_dev(items, planes_filters(filters, count), planes_strides(strides, count), count, esize, chunk,
                                           d_planes.data_ptr(), pitch, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_join_sbatch(d_planes, offset, pitch, items, filters, strides, count, first_item, item_count, esize, chunk, d_table, table_bytes):
    """enqueue trc_planes_join_sbatch_dev from d_planes[offset:], the inverse of planes_split_sbatch (filters, strides: the whole batch's)"""
    _chk(lib().trc_planes_join_sbatch_dev(d_planes.data_ptr() + offset, pitch, items, planes_filters(filters, count), planes_strides(strides, count),
                                          count, first_item, item_count, esize, chunk, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_orders(orders, count):
    """the per-item predictor orders of a batch as the host array the ordered batch calls take: None (order 1), one int for every
    item, or a sequence of `count` ints.  Values are not judged here: the library does that."""
    return _byte_per_item("orders", orders, count)


def planes_split_obatch(items, filters, strides, orders, count, esize, chunk, d_planes, pitch, d_table, table_bytes):
    """enqueue trc_planes_split_obatch_dev: planes_split_sbatch with a zigzag-delta item i behind the predictor of order orders[i]"""
    _chk(lib().trc_planes_split_obatch_dev(items, planes_filters(filters, count), planes_strides(strides, count), planes_orders(orders, count), count,
                                           esize, chunk, d_planes.data_ptr(), pitch, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_join_obatch(d_planes, offset, pitch, items, filters, strides, orders, count, first_item, item_count, esize, chunk, d_table, table_bytes):
    """enqueue trc_planes_join_obatch_dev from d_planes[offset:], the inverse of planes_split_obatch (filters, strides, orders: the whole batch's)"""
    _chk(lib().trc_planes_join_obatch_dev(d_planes.data_ptr() + offset, pitch, items, planes_filters(filters, count), planes_strides(strides, count),
                                          planes_orders(orders, count), count, first_item, item_count, esize, chunk, d_table.data_ptr(), table_bytes,
                                          _cur_stream(d_planes)))


def planes_bases(bases, count):
    """the per-item bases of a batch as the host array the bbatch calls take: None, or a sequence of `count` device tensors,
    addresses or None.  Values are not judged here: the library does that."""
    if bases is None:
        return None
    b = [x.data_ptr() if hasattr(x, "data_ptr") else x for x in bases]
    if len(b) != count:
        raise TrcError("bases: one entry per item of the batch")
    return (C.c_void_p * max(count, 1))(*b)


def planes_split_bbatch(items, bases, filters, count, esize, chunk, d_planes, pitch, d_table, table_bytes):
    """enqueue trc_planes_split_bbatch_dev: planes_split_batch of the items, item i filtered against bases[i] (see planes_bases)"""
    _chk(lib().trc_planes_split_bbatch_dev(items, planes_bases(bases, count), planes_filters(filters, count), count, esize, chunk,
                                           d_planes.data_ptr(), pitch, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


def planes_join_bbatch(d_planes, offset, pitch, items, bases, filters, count, first_item, item_count, esize, chunk, d_table, table_bytes):
    """enqueue trc_planes_join_bbatch_dev from d_planes[offset:], the inverse of planes_split_bbatch (bases, filters: the whole batch's)"""
    _chk(lib().trc_planes_join_bbatch_dev(d_planes.data_ptr() + offset, pitch, items, planes_bases(bases, count), planes_filters(filters, count),
                                          count, first_item, item_count, esize, chunk, d_table.data_ptr(), table_bytes, _cur_stream(d_planes)))


class PlanesBatchCoder:
    """The coded buffers of one batch of device tensors of one element size (bf16 / fp16: 2, fp32: 4, fp64 / int64: 8), coded by
    trc_encode_planes_batch_dev as the planes of their virtual buffer: self.clen / payload / total / cdf / status are laid out as
    PlanesCoder's for n = plan["n_virtual"].  decode(first_item, item_count) writes those items back into the tensors given (the
    encoded ones by default).  filters (None, one FILTER_* for all items, or one per item) puts a predictor filter in front of
    each item's planes: the trc_*_fplanes_batch_dev calls, and decode() passes the same filters on.  filters="auto": encode() first
    asks the batch advisor (planes_advise_batch_dev, which waits for the stream) about the tensors' current contents, leaves its
    choice in self.filters and what decided in self.advice, and codes exactly as if that list had been given.  strides (None, one
    int for all items, or one per item, each 1 .. 8) predicts a filtered item from the element that many back -- rows of K fields,
    interleaved channels: the trc_*_splanes_batch_dev calls where an item with a filter has a stride above 1, today's calls
    otherwise; with filters="auto" the advisor chooses under these strides.  bases (a list of one tensor or None per item):
    filters[i] then means "against bases[i]" -- the trc_*_bplanes_batch_dev calls; decode(bases=...) may be given other bases (the
    output tensors themselves: in place).  It cannot be combined with strides or filters="auto", and pack() raises: the TRCB
    container has no place for a base.  orders (None, one int for all items, or one per item, each 1 .. 3) puts a zigzag-delta item
    behind the polynomial predictor of that order: the trc_*_oplanes_batch_dev calls and the TRCU container where such an item has an
    order above 1 (ordered()), the calls above otherwise.  orders="auto": encode() first asks the order advisor
    (planes_advise_obatch_dev, which waits for the stream) under the coder's strides, leaves its choice in self.filters and
    self.orders and what decided in self.advice; filters must then be None.  Orders cannot be combined with bases.  Plumbing only."""

    def __init__(self, codec, tensors, chunk=4096, cdfnum=256, prm=(5, 6), guard=0, esize=None, filters=None, strides=None, bases=None, orders=None):
        """esize: the element size where the tensors do not say it themselves (uint8 tensors of whole elements)"""
        import torch
        self.torch = torch
        tensors = list(tensors)
        if not tensors or any(not t.is_cuda or not t.is_contiguous() or t.element_size() != tensors[0].element_size() for t in tensors):
            raise TrcError("a batch is a non-empty list of contiguous device tensors of one element size")
        self.codec, self.chunk, self.esize, self.count = codec, chunk, esize or tensors[0].element_size(), len(tensors)
        self.dev = tensors[0].device
        self.sizes = [t.numel() * t.element_size() for t in tensors]
        self.items = self._items(tensors)
        self.auto, self.advice = isinstance(filters, str) and filters == "auto", None
        self.filters = None if self.auto else planes_filters(filters, self.count)
        self.strides = planes_strides(strides, self.count)
        self.auto_orders = isinstance(orders, str) and orders == "auto"
        self.orders = None if self.auto_orders else planes_orders(orders, self.count)
        if self.auto_orders and filters is not None:
            raise ValueError("orders=\"auto\" chooses the filters as well: filters must be None")
        if bases is not None and (strides is not None or self.auto or orders is not None):
            raise ValueError("bases cannot be combined with strides, orders or filters=\"auto\": a filter id then means \"against bases[i]\"")
        self._bases = None if bases is None else list(bases)   # (kept alive: the array below holds addresses only)
        self.bases = planes_bases(self._bases, self.count)
        self.plan, self.first = planes_batch_plan(self.items, self.count, self.esize, chunk)
        self.nch, self.pitch = self.plan["chunks"], self.plan["pitch"]
        self.cdfnum = _cdfnum(codec, cdfnum, prm)
        self.work_bytes = (lib().trc_planes_bbatch_work_bytes if self.bases is not None else lib().trc_planes_batch_work_bytes)(
            codec, self.items, self.count, self.esize, chunk)
        if self.work_bytes == 0:
            raise TrcError("bad (codec, tensors, chunk)")
        self.guard, self._guards = guard, []
        self.work = self._buf(self.work_bytes)
        self.clen = self._buf(4 * self.esize * self.nch)
        self.payload = self._buf(self.esize * self.pitch)
        self.total = self._buf(8 * self.esize)
        self.cdf = self._buf(2 * self.esize * PLANES_CDF_STRIDE)
        self.status = self._buf(4 * self.esize)
        self.range_work, self.range_work_bytes = None, 0
        self._tensors = tensors

    _buf = PlanesCoder._buf
    guards_ok = PlanesCoder.guards_ok
    _stream = PlanesCoder._stream
    cdf_of = PlanesCoder.cdf_of
    result = PlanesCoder.result

    def _items(self, tensors):
        """tensors of the batch's sizes; None where decode is not to look"""
        if len(tensors) != self.count or any(t is not None and t.numel() * t.element_size() != n for t, n in zip(tensors, self.sizes)):
            raise TrcError("the tensors do not have the batch's sizes")
        return planes_items([(t.data_ptr() if t is not None else None, n) for t, n in zip(tensors, self.sizes)])

    def encode(self, flags=0):
        if self.auto_orders:                                   # the order advisor on what the tensors hold now, under the coder's strides
            f, o, self.advice = planes_advise_obatch_dev(self.items, self.esize, self.chunk, 15, self.count, self.dev, strides=self.strides)
            self.filters, self.orders = planes_filters(f, self.count), planes_orders(o, self.count)
        if self.auto:                                          # the advisor on what the tensors hold now; then as if that list had been given
            chosen, self.advice = planes_advise_batch_dev(self.items, self.esize, self.chunk, 7, self.count, self.dev, strides=self.strides)
            self.filters = planes_filters(chosen, self.count)
        st = self.codec in STATIC
        tail = (self.count, self.esize, self.chunk, self.cdf.data_ptr() if st else None, self.cdfnum, self.status.data_ptr() if st else None,
                self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(), self.work.data_ptr(), self.work_bytes, self._stream())
        fam, lead = self._family()
        _chk(getattr(lib(), "trc_encode_%splanes_batch_dev" % fam)(self.codec | flags, self.items, *lead, *tail))

    def _family(self, bases=None):
        """which calls the coder's bases, filters and strides select as they stand -- "b", "" (no filter), "s" or "f", the letter in
        front of "planes" in their names -- and what those take between the items and `count`.  bases: others than the coder's"""
        if self.bases is not None:
            return "b", (self.bases if bases is None else planes_bases(list(bases), self.count), self.filters)
        if self.filters is None:
            return "", ()
        if self.ordered():
            return "o", (self.filters, self.strides, self.orders)
        return ("s", (self.filters, self.strides)) if self.strided() else ("f", (self.filters,))

    def _packed_family(self):
        """the same for the container calls, which come ordered ("o"), strided ("s") or not ("") and always take the filters, None included"""
        if self.ordered():
            return "o", (self.filters, self.strides, self.orders)
        return ("s", (self.filters, self.strides)) if self.strided() else ("", (self.filters,))

    def ordered(self):
        """whether a zigzag-delta item has an order above 1: the ordered calls and the TRCU container; else the others"""
        return self.filters is not None and self.orders is not None and \
            any(f == FILTER_ZDELTA and o > 1 for f, o in zip(self.filters[:self.count], self.orders[:self.count]))

    def strided(self):
        """whether an item with a filter has a stride above 1: the strided calls; else today's"""
        return self.filters is not None and self.strides is not None and \
            any(f != FILTER_NONE and s > 1 for f, s in zip(self.filters[:self.count], self.strides[:self.count]))

    def decode(self, first_item=0, item_count=None, out=None, flags=0, bases=None):
        """items [first_item, first_item + item_count) into out[i] (a list of count tensors, None outside the range; default: the
        encoded tensors), in a workspace of its own that grows with the requested chunks.  bases (a coder with bases): the bases
        to decode against instead of the coder's own, one per item, None outside the range"""
        item_count = self.count - first_item if item_count is None else item_count
        items = self.items if out is None else self._items(list(out))
        range_bytes = lib().trc_planes_bbatch_range_work_bytes if self.bases is not None else lib().trc_planes_batch_range_work_bytes
        need = range_bytes(self.codec, items, self.count, self.esize, self.chunk, first_item, item_count)
        if need > self.range_work_bytes:
            self.range_work, self.range_work_bytes = self._buf(need), need
        if self.range_work is None:                            # nothing to size a workspace by: the call rejects or ignores these arguments itself
            self.range_work = self._buf(0)
        tail = (self.count, first_item, item_count, self.esize, self.chunk, self.cdf.data_ptr() if self.codec in STATIC else None, self.cdfnum,
                self.range_work.data_ptr(), self.range_work_bytes, self._stream())
        fam, lead = self._family(bases)
        _chk(getattr(lib(), "trc_decode_%splanes_batch_dev" % fam)(self.codec | flags, self.clen.data_ptr(), self.payload.data_ptr(), items, *lead, *tail))

    def pack(self, guard=0):
        """enqueue trc_planes_batch_pack_dev (strided(): trc_planes_sbatch_pack_dev, the TRCT container, sized by trc_planes_sbatch_bound;
        ordered(): trc_planes_obatch_pack_dev, the TRCU container, sized by trc_planes_obatch_bound)
        on what encode() left, then synchronise to read the size -> (the TRCB container: a uint8
        device tensor trimmed to its size, with what remains of the planes_batch_bound bytes readable behind it; the size).  guard:
        0xA5 from the container's start through to the bound and that many bytes past it; self.pack_guard = the tensor's bytes behind
        the container, which must still be 0xA5.  The full buffer stays in self.packed."""
        if self.bases is not None:
            raise TrcError("pack: the TRCB container has no place for a base; a batch against bases has no container")
        st = self.codec in STATIC
        fam, lead = self._packed_family()
        bound = getattr(lib(), "trc_planes_%sbatch_bound" % fam)(self.codec, self.items, self.count, self.esize, self.chunk, self.cdfnum)
        if bound == 0:
            raise TrcError("bad (codec, tensors, chunk, cdfnum)")
        buf = self.torch.full((bound + guard,), 0xA5 if guard else 0, dtype=self.torch.uint8, device=self.dev)
        d_size = self.torch.zeros(1, dtype=self.torch.int64, device=self.dev)
        tail = (self.count, self.esize, self.chunk, self.cdf.data_ptr() if st else None, self.cdfnum, self.status.data_ptr() if st else None,
                self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(), buf.data_ptr(), bound, d_size.data_ptr(), self._stream())
        _chk(getattr(lib(), "trc_planes_%sbatch_pack_dev" % fam)(self.codec, self.items, *lead, *tail))
        size = int(d_size.item())
        self.packed, self.pack_guard = buf, buf[size:]
        return buf[:size], size

    def decode_packed(self, d_cont, total, first_item=0, item_count=None, out=None, cont_bytes=None, work_bytes=None):
        """the inverse of pack(): items [first_item, first_item + item_count) straight from the container d_cont (a uint8 device tensor;
        `total`: the planes' payload sizes, as parse_planes_batch gives them) into out[i] (default: the encoded tensors).  cont_bytes /
        work_bytes: what the call is told instead of the truth (the tests' argument errors)"""
        item_count = self.count - first_item if item_count is None else item_count
        items = self.items if out is None else self._items(list(out))
        need = lib().trc_planes_batch_range_work_bytes(self.codec, items, self.count, self.esize, self.chunk, first_item, item_count)
        if need > self.range_work_bytes:
            self.range_work, self.range_work_bytes = self._buf(need), need
        if self.range_work is None:
            self.range_work = self._buf(0)
        tot = (C.c_uint64 * 8)(*[int(x) for x in total])
        tail = (self.count, first_item, item_count, self.esize, self.chunk, self.cdfnum, tot, self.range_work.data_ptr(),
                need if work_bytes is None else work_bytes, self._stream())
        fam, lead = self._packed_family()                      # ("s": d_cont is the TRCT container pack() gave)
        _chk(getattr(lib(), "trc_decode_%splanes_batch_packed_dev" % fam)(self.codec, d_cont.data_ptr(), d_cont.numel() if cont_bytes is None else cont_bytes,
                                                                         items, *lead, *tail))

    def stored_bytes(self):
        """Synchronise: payload + directory (+ CDFs of a static coder) of all planes"""
        self.torch.cuda.synchronize(self.dev)
        tot = self.total[:8 * self.esize].cpu().numpy().view("<u8")
        return int(tot.sum()) + self.esize * (4 * self.nch + (2 * (self.cdfnum + 1) if self.codec in STATIC else 0))


class BasePlanesBatchCoder(PlanesBatchCoder):
    """PlanesBatchCoder for a batch against bases (required: one tensor or None per item) with the TRCE container, which names every
    base by its fingerprint: pack() -> the container, decode_packed(..., bases=None) decodes from it against the coder's bases or the
    ones given (the output tensors themselves: in place), verify(d_cont, bases=None) -> the lowest item index whose base does not
    have the container's fingerprint, or -1.  filters="auto": encode() first asks the advisor against the bases
    (planes_advise_batch_dev(bases=...), which waits for the stream; an item without a base is never given a filter) and leaves
    self.filters / self.advice as the parent does.  Where no filter is chosen anywhere the batch is a TRCB container: pack() raises
    as the library does.  No strides."""

    def __init__(self, codec, tensors, chunk=4096, cdfnum=256, prm=(5, 6), guard=0, esize=None, filters=None, bases=None):
        if bases is None:
            raise ValueError("BasePlanesBatchCoder codes against bases: one tensor or None per item")
        auto = isinstance(filters, str) and filters == "auto"
        super().__init__(codec, tensors, chunk, cdfnum=cdfnum, prm=prm, guard=guard, esize=esize, filters=None if auto else filters, bases=bases)
        self.auto_bases = auto                                 # (self.auto stays False: the parent's advisor knows no bases)
        self.table_bytes = lib().trc_base_fingerprint_batch_table_bytes(self.count)
        self.table = self._buf(self.table_bytes)

    def encode(self, flags=0):
        if self.auto_bases:                                    # the advisor against the bases on what the tensors hold now
            chosen, self.advice = planes_advise_batch_dev(self.items, self.esize, self.chunk, 7, self.count, self.dev, bases=self._bases)
            self.filters = planes_filters(chosen, self.count)
        super().encode(flags)

    def pack(self, guard=0):
        """enqueue trc_planes_bbatch_pack_dev on what encode() left, then synchronise to read the size -> (the TRCE container: a uint8
        device tensor trimmed to its size; the size).  guard, self.packed and self.pack_guard as in the parent"""
        st = self.codec in STATIC
        bound = lib().trc_planes_bbatch_bound(self.codec, self.items, self.count, self.esize, self.chunk, self.cdfnum)
        if bound == 0:
            raise TrcError("bad (codec, tensors, chunk, cdfnum)")
        buf = self.torch.full((bound + guard,), 0xA5 if guard else 0, dtype=self.torch.uint8, device=self.dev)
        d_size = self.torch.zeros(1, dtype=self.torch.int64, device=self.dev)
        _chk(lib().trc_planes_bbatch_pack_dev(self.codec, self.items, self.bases, self.filters, self.count, self.esize, self.chunk,
                                              self.cdf.data_ptr() if st else None, self.cdfnum, self.status.data_ptr() if st else None,
                                              self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(), buf.data_ptr(), bound,
                                              d_size.data_ptr(), self.table.data_ptr(), self.table_bytes, self._stream()))
        size = int(d_size.item())
        self.packed, self.pack_guard = buf, buf[size:]
        return buf[:size], size

    def decode_packed(self, d_cont, total, first_item=0, item_count=None, out=None, cont_bytes=None, work_bytes=None, bases=None):
        """the inverse of pack(): trc_decode_bplanes_batch_packed_dev from the TRCE container d_cont (`total` as parse_planes_bbatch
        gives it) into out[i] (default: the encoded tensors) against `bases` (default: the coder's); it does not verify them"""
        item_count = self.count - first_item if item_count is None else item_count
        items = self.items if out is None else self._items(list(out))
        need = lib().trc_planes_bbatch_range_work_bytes(self.codec, items, self.count, self.esize, self.chunk, first_item, item_count)
        if need > self.range_work_bytes:
            self.range_work, self.range_work_bytes = self._buf(need), need
        if self.range_work is None:
            self.range_work = self._buf(0)
        tot = (C.c_uint64 * 8)(*[int(x) for x in total])
        _chk(lib().trc_decode_bplanes_batch_packed_dev(self.codec, d_cont.data_ptr(), d_cont.numel() if cont_bytes is None else cont_bytes, items,
                                                       *self._family(bases)[1], self.count, first_item, item_count, self.esize, self.chunk, self.cdfnum, tot,
                                                       self.range_work.data_ptr(), need if work_bytes is None else work_bytes, self._stream()))

    def verify(self, d_cont, bases=None, first_item=0, item_count=None):
        """trc_base_verify_batch_dev, then synchronise -> the lowest index in [first_item, first_item + item_count) whose base (the
        coder's, or the one given) does not have the fingerprint the container holds, or -1"""
        item_count = self.count - first_item if item_count is None else item_count
        d_bad = self.torch.full((1,), -2, dtype=self.torch.int64, device=self.dev)
        _chk(lib().trc_base_verify_batch_dev(d_cont.data_ptr(), self.items, *self._family(bases)[1], self.count, first_item, item_count,
                                             d_bad.data_ptr(), self.table.data_ptr(), self.table_bytes, self._stream()))
        return int(d_bad.item())


def base_fingerprint_batch(items, bases, filters, count, first_item, item_count, d_fp, d_table, table_bytes):
    """enqueue trc_base_fingerprint_batch_dev: the fingerprints of the bases of items [first_item, first_item + item_count) with a
    filter into d_fp (8 bytes per item of the range, 0 where the filter is NONE); does not wait"""
    _chk(lib().trc_base_fingerprint_batch_dev(items, planes_bases(bases, count), planes_filters(filters, count), count, first_item, item_count,
                                              d_fp.data_ptr(), d_table.data_ptr(), table_bytes, _cur_stream(d_fp)))


# ------------------------------------------------------ reference-signature layer (host pointers) ---
_HOST_ENC = {ANS4S: "anscdf4senc", RCS1: "rccdfsenc", RCS2: "rccdfs2enc", RCA: "rccdfenc", ANSA: "anscdfenc", RCB: "rcsenc", RCAI: "rccdfienc",
             RCA4: "rccdf4enc", RCAI4: "rccdf4ienc", ANSA4: "anscdf4enc", RCSM: "rccdfsmenc", ANSO1: "anscdf1enc", ANSB: "ansbc",
             VLCU16: "rccdfuenc16", VLCU32: "rccdfuenc32", VLCV16: "rccdfvenc16", VLCV32: "rccdfvenc32", VLCVZ16: "rccdfvzenc16", VLCVZ32: "rccdfvzenc32",
             VLAU16: "anscdfuenc16", VLAUZ16: "anscdfuzenc16", VLAV16: "anscdfvenc16", VLAVZ16: "anscdfvzenc16", VLAV32: "anscdfvenc32", VLAVZ32: "anscdfvzenc32",
             RCV8: "rccdfenc8", RCVI8: "rccdfienc8", RCC1: "rccsenc", RCX1: "rcxsenc",
             RCG8: "rcgsenc8", RCG16: "rcgsenc16", RCG32: "rcgsenc32", RCGZ8: "rcgzsenc8", RCGZ16: "rcgzsenc16", RCGZ32: "rcgzsenc32",
             RCR8: "rcrsenc8", RCR16: "rcrsenc16", RCR32: "rcrsenc32", RCRZ8: "rcrzsenc8", RCRZ16: "rcrzsenc16", RCRZ32: "rcrzsenc32",
             RCBV16: "rcvsenc16", RCBV32: "rcvsenc32", RCBVZ16: "rcvzsenc16", RCBVZ32: "rcvzsenc32",
             RCBVG16: "rcvgsenc16", RCBVG32: "rcvgsenc32", RCBVGZ16: "rcvgzsenc16", RCBVGZ32: "rcvgzsenc32",
             RCW16: "rcsenc16", RCW32: "rcsenc32", RCCW32: "rccsenc32", RCC2W32: "rcc2senc32",
             RC4: "rc4senc", RC4C: "rc4csenc", RCU3: "rcu3senc",
             RCSS: "rcssenc", RC4SS: "rc4ssenc", RC4CSS: "rc4cssenc", RCU3SS: "rcu3ssenc"}
_HOST_DEC = {ANS4S: "anscdf4sdec", RCS1: "rccdfsbdec", RCS2: "rccdfsb2dec", RCA: "rccdfdec", ANSA: "anscdfdec", RCB: "rcsdec", RCAI: "rccdfidec",
             RCA4: "rccdf4dec", RCAI4: "rccdf4idec", ANSA4: "anscdf4dec", RCSM: "rccdfsmbdec", ANSO1: "anscdf1dec", ANSB: "ansbd",
             VLCU16: "rccdfudec16", VLCU32: "rccdfudec32", VLCV16: "rccdfvdec16", VLCV32: "rccdfvdec32", VLCVZ16: "rccdfvzdec16", VLCVZ32: "rccdfvzdec32",
             VLAU16: "anscdfudec16", VLAUZ16: "anscdfuzdec16", VLAV16: "anscdfvdec16", VLAVZ16: "anscdfvzdec16", VLAV32: "anscdfvdec32", VLAVZ32: "anscdfvzdec32",
             RCV8: "rccdfdec8", RCVI8: "rccdfidec8", RCC1: "rccsdec", RCX1: "rcxsdec",
             RCG8: "rcgsdec8", RCG16: "rcgsdec16", RCG32: "rcgsdec32", RCGZ8: "rcgzsdec8", RCGZ16: "rcgzsdec16", RCGZ32: "rcgzsdec32",
             RCR8: "rcrsdec8", RCR16: "rcrsdec16", RCR32: "rcrsdec32", RCRZ8: "rcrzsdec8", RCRZ16: "rcrzsdec16", RCRZ32: "rcrzsdec32",
             RCBV16: "rcvsdec16", RCBV32: "rcvsdec32", RCBVZ16: "rcvzsdec16", RCBVZ32: "rcvzsdec32",
             RCBVG16: "rcvgsdec16", RCBVG32: "rcvgsdec32", RCBVGZ16: "rcvgzsdec16", RCBVGZ32: "rcvgzsdec32",
             RCW16: "rcsdec16", RCW32: "rcsdec32", RCCW32: "rccsdec32", RCC2W32: "rcc2sdec32",
             RC4: "rc4sdec", RC4C: "rc4csdec", RCU3: "rcu3sdec",
             RCSS: "rcssdec", RC4SS: "rc4ssdec", RC4CSS: "rc4cssdec", RCU3SS: "rcu3ssdec"}


def _host_fn(name, codec):
    f = getattr(lib(), name)
    f.restype = _sz
    if codec == ANS4S:
        f.argtypes = [_u8p, _sz, _u8p, _u16p]
    elif codec in (RCS1, RCS2, RCSM):
        f.argtypes = [_u8p, _sz, _u8p, _u16p, C.c_uint]
    elif codec in SSBIT:
        f.argtypes = [_u8p, _sz, _u8p, C.c_uint, C.c_uint]
    else:
        f.argtypes = [_u8p, _sz, _u8p]
    return f


def _host_args(codec, cdf, cdfnum, prm):
    """what a reference-named call takes behind (in, n, out): the values for the prototype _host_fn sets"""
    if codec == ANS4S:
        return (cdf.ctypes.data_as(_u16p),)
    if codec in (RCS1, RCS2, RCSM):
        return (cdf.ctypes.data_as(_u16p), cdfnum)
    if codec in SSBIT:
        return (prm[0], prm[1])
    return ()


def host_encode(codec, data, cdf=None, cdfnum=256, name=None, prm=(5, 6)):
    """Call the reference-named encoder with host pointers -> np.uint8 array of the returned length."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    out = np.zeros(n + n // 3 + 1024, dtype=np.uint8)          # the harness's OSIZE (turborc.c:418)
    f = _host_fn(name or _HOST_ENC[codec], codec)
    l = f(data.ctypes.data_as(_u8p), n, out.ctypes.data_as(_u8p), *_host_args(codec, cdf, cdfnum, prm))
    if l == 0 and n != 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def host_decode(codec, comp, n, cdf=None, cdfnum=256, name=None, prm=(5, 6)):
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    if comp.size == n:
        return comp.copy()                                      # CCPY rule (turborc.c:434)
    src = np.zeros(comp.size + 1024, dtype=np.uint8); src[:comp.size] = comp
    out = np.full(n + 64, 0xA5, dtype=np.uint8)
    f = _host_fn(name or _HOST_DEC[codec], codec)
    l = f(src.ctypes.data_as(_u8p), n, out.ctypes.data_as(_u8p), *_host_args(codec, cdf, cdfnum, prm))
    if l != n:
        raise TrcError(lib().trc_last_error().decode())
    return out[:n].copy()


def container_range(buf, offset, length):
    """trc_container_range on a container in host memory (needs no device) -> dict of the six trc_range fields"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    r = Range()
    _chk(lib().trc_container_range(buf.ctypes.data, buf.size, 0, offset, length, C.byref(r)))
    return {f: int(getattr(r, f)) for f, _ in Range._fields_}


def host_decode_range(codec, comp, n, offset, length, cdf=None, cdfnum=256, prm=None):
    """bytes [offset, offset + length) of what `comp` (a host-pointer encoder's result for n bytes) holds: trc_decode_range_host.
    prm: an "ss" coder's parameters, None = those of the container's header"""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    out = np.full(length + 64, 0xA5, dtype=np.uint8)
    st = codec in STATIC
    l = lib().trc_decode_range_host(codec, comp.ctypes.data, comp.size, n, offset, length, out.ctypes.data,
                                    cdf.ctypes.data if st else None, _cdfnum(codec, cdfnum, prm) if prm or st else 0)
    if l != length or not (out[length:] == 0xA5).all():
        raise TrcError(lib().trc_last_error().decode() if l != length else "trc_decode_range_host wrote past its output")
    return out[:length].copy()


def set_devices(devs):
    """devices of the host-pointer calls ([] = the caller's current device; an entry may repeat: include/trc_hip.h)"""
    arr = (C.c_int * max(len(devs), 1))(*devs)
    _chk(lib().trc_set_devices(arr, len(devs)))


def host_cdfini(data, cdfnum=None):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if cdfnum is None:
        cdfnum = int(data.max()) + 1
    cdf = np.zeros(257, dtype=np.uint16)
    f = lib().cdfini
    f.restype = C.c_int; f.argtypes = [_u8p, _sz, _u16p, C.c_uint]
    r = f(data.ctypes.data_as(_u8p), data.size, cdf.ctypes.data_as(_u16p), cdfnum)
    return r, cdf, cdfnum


def parse_container(buf):
    """-> dict(hdr fields), clen (u32 array), payload (u8 array)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    magic, codec, ver, cdfnum, chunk, nch = np.frombuffer(buf[:16].tobytes(), dtype="<u4,u1,u1,<u2,<u4,<u4")[0]
    n, pay = np.frombuffer(buf[16:32].tobytes(), dtype="<u8")
    clen = buf[HDR:HDR + 4 * int(nch)].view("<u4").copy()
    payload = buf[HDR + 4 * int(nch):HDR + 4 * int(nch) + int(pay)].copy()
    return dict(magic=int(magic), codec=int(codec), version=int(ver), cdfnum=int(cdfnum), chunk=int(chunk),
                nchunks=int(nch), n=int(n), payload=int(pay)), clen, payload


def planes_bound(n, esize, chunk=0, cdfnum=0):
    return lib().trc_planes_bound(n, esize, chunk, cdfnum)


def host_encode_planes(codec, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_planes_host -> the TRCP container (np.uint8); chunk 0 = automatic"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(planes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    l = lib().trc_encode_planes_host(codec, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def _host_decode_guarded(name, comp, length, offset=None):
    """the host call `name` for `length` bytes (of the whole container, or from `offset` where given) into an output with 64 bytes
    of 0xA5 behind it, which must survive"""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    out = np.full(length + 64, 0xA5, dtype=np.uint8)
    f = getattr(lib(), name)
    if offset is None:
        l = f(comp.ctypes.data, comp.size, out.ctypes.data, length)
    else:
        l = f(comp.ctypes.data, comp.size, offset, length, out.ctypes.data)
    if l != length or not (out[length:] == 0xA5).all():
        raise TrcError(lib().trc_last_error().decode() if l != length else name + " wrote past its output")
    return out[:length].copy()


def host_decode_planes(comp, n):
    return _host_decode_guarded("trc_decode_planes_host", comp, n)


def host_decode_planes_range(comp, offset, length):
    return _host_decode_guarded("trc_decode_planes_range_host", comp, length, offset)


def planes_check(buf, outlen=None):
    """trc_planes_check on a TRCP container in host memory (needs no device); raises TrcError with the library's reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_planes_check(buf.ctypes.data, buf.size, (1 << 64) - 1 if outlen is None else outlen))


def parse_planes(buf):
    """-> dict(hdr fields, off=[...]), sections: per plane (cdf u16 array or None, the TRC1 container of the plane as u8 array), tail"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    magic, codec, ver, esize, tail, chunk, cdfnum = np.frombuffer(buf[:16].tobytes(), dtype="<u4,u1,u1,u1,u1,<u4,<u4")[0]
    n, size = (int(x) for x in np.frombuffer(buf[16:32].tobytes(), dtype="<u8"))
    esize, tail, cdfnum, codec = int(esize), int(tail), int(cdfnum), int(codec)
    off = [int(x) for x in np.frombuffer(buf[PLANES_HDR:PLANES_HDR + 8 * esize].tobytes(), dtype="<u8")]
    cdfb = (2 * (cdfnum + 1) + 7) & ~7 if codec in STATIC else 0
    sections = []
    for k in range(esize):
        sec = buf[off[k]:(off[k + 1] if k + 1 < esize else size - tail)]
        hdr, _, _ = parse_container(sec[cdfb:])
        used = HDR + 4 * hdr["nchunks"] + hdr["payload"]
        sections.append((sec[:2 * (cdfnum + 1)].view("<u2").copy() if cdfb else None, sec[cdfb:cdfb + used].copy()))
    return dict(magic=int(magic), codec=codec, version=int(ver), esize=esize, tail=tail, chunk=int(chunk), cdfnum=cdfnum,
                n=n, size=size, off=off), sections, buf[size - tail:size].copy()


# ------------------------------------------------------------ byte planes behind a filter (include/trc_hip.h) ---
FILTER_NONE, FILTER_ZDELTA, FILTER_XOR = 0, 1, 2
FPLANES_MAGIC = 0x46435254                                     # "TRCF"
FPLANES_HDR = 16


def planes_split_filter(filt, d_in, n, esize, seg, d_planes, pitch, d_tail=None):
    """enqueue trc_planes_split_filter_dev: planes_split of the zigzag-delta / xor filtered elements, restarting every seg elements"""
    _chk(lib().trc_planes_split_filter_dev(filt, d_in.data_ptr(), n, esize, seg, d_planes.data_ptr(), pitch,
                                           d_tail.data_ptr() if d_tail is not None else None, _cur_stream(d_in)))


def planes_join_filter(filt, d_planes, pitch, d_tail, n, esize, seg, d_out):
    """enqueue trc_planes_join_filter_dev, the inverse of planes_split_filter"""
    _chk(lib().trc_planes_join_filter_dev(filt, d_planes.data_ptr(), pitch, d_tail.data_ptr() if d_tail is not None else None, n, esize,
                                          seg, d_out.data_ptr(), _cur_stream(d_out)))


class FilteredPlanesCoder(PlanesCoder):
    """PlanesCoder through the trc_*_fplanes_dev calls: the same buffers and results, of the filtered elements (restart = chunk).
    filter=FILTER_NONE is the unfiltered coder."""
    _ENC, _DEC, _DEC_RANGE = "trc_encode_fplanes_dev", "trc_decode_fplanes_dev", "trc_decode_fplanes_range_dev"

    def __init__(self, codec, n, esize, chunk=4096, device="cuda", cdfnum=256, prm=(5, 6), guard=0, filter=FILTER_NONE):
        super().__init__(codec, n, esize, chunk, device, cdfnum=cdfnum, prm=prm, guard=guard)
        self.filter = filter

    def _lead(self):
        return (self.filter,)


def fplanes_bound(n, esize, chunk=0, cdfnum=0):
    return lib().trc_fplanes_bound(n, esize, chunk, cdfnum)


def host_encode_fplanes(codec, filt, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_fplanes_host -> the TRCF container (np.uint8): 16 bytes, then the TRCP container of the filtered data"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(fplanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    l = lib().trc_encode_fplanes_host(codec, filt, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def host_decode_fplanes(comp, n):
    return _host_decode_guarded("trc_decode_fplanes_host", comp, n)


def host_decode_fplanes_range(comp, offset, length):
    return _host_decode_guarded("trc_decode_fplanes_range_host", comp, length, offset)


def fplanes_check(buf, outlen=None):
    """trc_fplanes_check on a TRCF container in host memory (needs no device); raises TrcError with the library's reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_fplanes_check(buf.ctypes.data, buf.size, (1 << 64) - 1 if outlen is None else outlen))


# ------------------------------------------------------------------- the planes advisor (include/trc_hip.h) ---
def planes_hist_bytes(esize):
    return lib().trc_planes_hist_bytes(esize)


def planes_hist(filters, d_in, n, esize, seg, d_hist):
    """enqueue trc_planes_hist_dev: the byte histograms of the planes of d_in[:n] under every filter of the bit set `filters`,
    into d_hist (3 * esize * 256 uint64 as a device tensor; zeroed by the call)"""
    _chk(lib().trc_planes_hist_dev(filters, d_in.data_ptr(), n, esize, seg, d_hist.data_ptr(), _cur_stream(d_in)))


def _advice_dict(a):
    return dict(filter=int(a.filter), esize=int(a.esize), filters=int(a.filters), m=int(a.m),
                bits=np.array([list(r) for r in a.bits], dtype=np.float64), total_bits=np.array(list(a.total_bits), dtype=np.float64))


def planes_advise(hist, filters, esize, m):
    """trc_planes_advise on histograms in host memory (uint64 [3 * esize * 256]; needs no device) -> dict of the advice's fields"""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    if hist.size < 3 * esize * 256:                                # (a bad esize is the library's to refuse: give it something to read)
        hist = np.concatenate([hist.reshape(-1), np.zeros(3 * 8 * 256, dtype=np.uint64)])
    a = PlanesAdvice()
    _chk(lib().trc_planes_advise(hist.ctypes.data, filters, esize, m, C.byref(a)))
    return _advice_dict(a)


def planes_hist_batch_bytes(item_count, esize):
    return lib().trc_planes_hist_batch_bytes(item_count, esize)


def planes_hist_batch(filters, items, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes):
    """enqueue trc_planes_hist_batch_dev: slice j of d_hist (3 * esize * 256 uint64 each; zeroed by the call) = the histograms
    planes_hist would leave for item first_item + j of the batch alone, with seg = chunk"""
    _chk(lib().trc_planes_hist_batch_dev(filters, items, count, first_item, item_count, esize, chunk, d_hist.data_ptr(),
                                         d_table.data_ptr(), table_bytes, _cur_stream(d_hist)))


def planes_hist_sbatch(filters, items, strides, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes):
    """enqueue trc_planes_hist_sbatch_dev: planes_hist_batch with item i's predicted rows counted against the element strides[i] back
    (strides: see planes_strides) -- slice j is what planes_hist_stride leaves for item first_item + j alone at its stride"""
    _chk(lib().trc_planes_hist_sbatch_dev(filters, items, planes_strides(strides, count), count, first_item, item_count, esize, chunk,
                                          d_hist.data_ptr(), d_table.data_ptr(), table_bytes, _cur_stream(d_hist)))


def planes_hist_obatch_bytes(item_count, esize):
    return lib().trc_planes_hist_obatch_bytes(item_count, esize)


def planes_hist_obatch(orders_set, items, strides, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes):
    """enqueue trc_planes_hist_obatch_dev: the histograms of orders 0 .. 3 (orders_set: bit k = order k) of every item of the range at
    its stride -- slice j (4 * esize * 256 uint64) is what planes_hist_order leaves for item first_item + j alone"""
    _chk(lib().trc_planes_hist_obatch_dev(orders_set, items, planes_strides(strides, count), count, first_item, item_count, esize, chunk,
                                          d_hist.data_ptr(), d_table.data_ptr(), table_bytes, _cur_stream(d_hist)))


def planes_advise_obatch(hist, orders_set, esize, items, count, advice=True):
    """trc_planes_advise_obatch on histograms in host memory (uint64, 4 * esize * 256 per item; needs no device)
    -> (the filter per item, the order per item, the advice per item: list of dicts, or None where advice is False)"""
    hist = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if esize in (2, 4, 8) and hist.size < count * 4 * esize * 256:
        raise TrcError("planes_advise_obatch: %d histogram words for %d items" % (hist.size, count))
    f, o = (C.c_uint8 * max(count, 1))(), (C.c_uint8 * max(count, 1))()
    adv = (PlanesOrderAdvice * max(count, 1))() if advice else None
    _chk(lib().trc_planes_advise_obatch(hist.ctypes.data, orders_set, esize, items, count, f, o, adv))
    return [int(x) for x in f[:count]], [int(x) for x in o[:count]], [_order_advice_dict(a) for a in adv[:count]] if advice else None


def planes_advise_obatch_dev(batch, esize=None, chunk=4096, orders_set=15, count=None, device="cuda", advice=True, strides=None):
    """trc_planes_advise_obatch_dev on a list of device tensors of one element size, or on a trc_planes_item array (as
    planes_advise_batch_dev), in a workspace of its own, under `strides` (see planes_strides).  Waits for the current stream.
    -> as planes_advise_obatch"""
    import torch
    if isinstance(batch, C.Array):
        items, count = batch, len(batch) if count is None else count
        dev = torch.device(device)
    else:
        tensors = list(batch)
        if not tensors or any(not t.is_cuda or not t.is_contiguous() for t in tensors):
            raise TrcError("a batch is a non-empty list of contiguous device tensors of one element size")
        items, count = planes_items([(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]), len(tensors)
        esize, dev = esize or tensors[0].element_size(), tensors[0].device
    need = lib().trc_planes_advise_obatch_work_bytes(items, count, esize, chunk)      # (0: the call names the reason itself)
    work = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    f, o = (C.c_uint8 * max(count, 1))(), (C.c_uint8 * max(count, 1))()
    adv = (PlanesOrderAdvice * max(count, 1))() if advice else None
    _chk(lib().trc_planes_advise_obatch_dev(orders_set, items, planes_strides(strides, count), count, esize, chunk, f, o, adv, work.data_ptr(), need,
                                            torch.cuda.current_stream(dev).cuda_stream))
    return [int(x) for x in f[:count]], [int(x) for x in o[:count]], [_order_advice_dict(a) for a in adv[:count]] if advice else None


def planes_hist_bbatch(filters, items, bases, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes):
    """enqueue trc_planes_hist_bbatch_dev: planes_hist_batch with item i's predicted rows counted against bases[i] (see planes_bases; an
    item without a base gets the unfiltered row alone) -- slice j is what planes_hist_base leaves for item first_item + j alone"""
    _chk(lib().trc_planes_hist_bbatch_dev(filters, items, planes_bases(bases, count), count, first_item, item_count, esize, chunk,
                                          d_hist.data_ptr(), d_table.data_ptr(), table_bytes, _cur_stream(d_hist)))


def planes_advise_batch(hist, filters, esize, items, count, advice=True, bases=False):
    """trc_planes_advise_batch on histograms in host memory (uint64, 3 * esize * 256 per item; needs no device)
    -> (the filter per item: list of ints, the advice per item: list of dicts, or None where advice is False).  bases (None, or a
    list of addresses / tensors / None per item): trc_planes_advise_bbatch, an item without a base under the unfiltered row alone"""
    hist = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if esize in (2, 4, 8) and hist.size < count * 3 * esize * 256:
        raise TrcError("planes_advise_batch: %d histogram words for %d items" % (hist.size, count))
    out = (C.c_uint8 * max(count, 1))()
    adv = (PlanesAdvice * max(count, 1))() if advice else None
    if bases is False:
        _chk(lib().trc_planes_advise_batch(hist.ctypes.data, filters, esize, items, count, out, adv))
    else:
        _chk(lib().trc_planes_advise_bbatch(hist.ctypes.data, filters, esize, items, planes_bases(bases, count), count, out, adv))
    return [int(x) for x in out[:count]], [_advice_dict(a) for a in adv[:count]] if advice else None


def planes_advise_batch_dev(batch, esize=None, chunk=4096, filters=7, count=None, device="cuda", advice=True, strides=None, bases=False):
    """trc_planes_advise_batch_dev on a list of device tensors of one element size, or on a trc_planes_item array (planes_items;
    esize is then required, count defaults to the array's length, the workspace lies on `device`), in a workspace of its own.
    Waits for the current stream.  strides (see planes_strides) given: trc_planes_advise_sbatch_dev, the choice under those strides.
    bases (None or see planes_bases) given: trc_planes_advise_bbatch_dev, the choice against those bases.  -> as planes_advise_batch"""
    import torch
    if isinstance(batch, C.Array):
        items, count = batch, len(batch) if count is None else count
        dev = torch.device(device)
    else:
        tensors = list(batch)
        if not tensors or any(not t.is_cuda or not t.is_contiguous() for t in tensors):
            raise TrcError("a batch is a non-empty list of contiguous device tensors of one element size")
        items, count = planes_items([(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]), len(tensors)
        esize, dev = esize or tensors[0].element_size(), tensors[0].device
    need = lib().trc_planes_advise_batch_work_bytes(items, count, esize, chunk)      # (0: the call names the reason itself)
    work = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    out = (C.c_uint8 * max(count, 1))()
    adv = (PlanesAdvice * max(count, 1))() if advice else None
    if bases is not False:
        _chk(lib().trc_planes_advise_bbatch_dev(filters, items, planes_bases(bases, count), count, esize, chunk, out, adv, work.data_ptr(), need,
                                                torch.cuda.current_stream(dev).cuda_stream))
    elif strides is None:
        _chk(lib().trc_planes_advise_batch_dev(filters, items, count, esize, chunk, out, adv, work.data_ptr(), need,
                                               torch.cuda.current_stream(dev).cuda_stream))
    else:
        _chk(lib().trc_planes_advise_sbatch_dev(filters, items, planes_strides(strides, count), count, esize, chunk, out, adv, work.data_ptr(), need,
                                                torch.cuda.current_stream(dev).cuda_stream))
    return [int(x) for x in out[:count]], [_advice_dict(a) for a in adv[:count]] if advice else None


def encode_aplanes_host(codec, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_aplanes_host -> (the TRCP or TRCF container the advisor chose (np.uint8), dict of the advice's fields)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(fplanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    a = PlanesAdvice()
    l = lib().trc_encode_aplanes_host(codec, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn, C.byref(a))
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy(), _advice_dict(a)


def host_decode_xplanes(comp, n):
    return _host_decode_guarded("trc_decode_xplanes_host", comp, n)


# -------------------------------------------- byte planes behind a strided filter: interleaved data (include/trc_hip.h) ---
SPLANES_MAGIC = 0x53435254                                     # "TRCS"
SPLANES_HDR = 16
STRIDE_MAX = 8


def planes_split_sfilter(filt, stride, d_in, n, esize, seg, d_planes, pitch, d_tail=None):
    """enqueue trc_planes_split_sfilter_dev: planes_split_filter with the predictor `stride` elements back (1 .. STRIDE_MAX)"""
    _chk(lib().trc_planes_split_sfilter_dev(filt, stride, d_in.data_ptr(), n, esize, seg, d_planes.data_ptr(), pitch,
                                            d_tail.data_ptr() if d_tail is not None else None, _cur_stream(d_in)))


def planes_join_sfilter(filt, stride, d_planes, pitch, d_tail, n, esize, seg, d_out):
    """enqueue trc_planes_join_sfilter_dev, the inverse of planes_split_sfilter"""
    _chk(lib().trc_planes_join_sfilter_dev(filt, stride, d_planes.data_ptr(), pitch, d_tail.data_ptr() if d_tail is not None else None, n,
                                           esize, seg, d_out.data_ptr(), _cur_stream(d_out)))


class StridedPlanesCoder(PlanesCoder):
    """PlanesCoder through the trc_*_splanes_dev calls: the same buffers and results, of the elements filtered against the element
    `stride` back (restart = chunk).  stride=1 is FilteredPlanesCoder, filter=FILTER_NONE the unfiltered coder."""
    _ENC, _DEC, _DEC_RANGE = "trc_encode_splanes_dev", "trc_decode_splanes_dev", "trc_decode_splanes_range_dev"

    def __init__(self, codec, n, esize, chunk=4096, device="cuda", cdfnum=256, prm=(5, 6), guard=0, filter=FILTER_NONE, stride=1):
        super().__init__(codec, n, esize, chunk, device, cdfnum=cdfnum, prm=prm, guard=guard)
        self.filter, self.stride = filter, stride

    def _lead(self):
        return (self.filter, self.stride)


def planes_hist_stride(filters, stride, d_in, n, esize, seg, d_hist):
    """enqueue trc_planes_hist_stride_dev: planes_hist with the rows of the zigzag-delta and xor filters counted under `stride`"""
    _chk(lib().trc_planes_hist_stride_dev(filters, stride, d_in.data_ptr(), n, esize, seg, d_hist.data_ptr(), _cur_stream(d_in)))


def splanes_bound(n, esize, chunk=0, cdfnum=0):
    return lib().trc_splanes_bound(n, esize, chunk, cdfnum)


def host_encode_splanes(codec, filt, stride, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_splanes_host -> the TRCS container (np.uint8): 16 bytes, then the TRCP container of the strided-filtered data"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(splanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    l = lib().trc_encode_splanes_host(codec, filt, stride, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def host_decode_splanes(comp, n):
    return _host_decode_guarded("trc_decode_splanes_host", comp, n)


def host_decode_splanes_range(comp, offset, length):
    return _host_decode_guarded("trc_decode_splanes_range_host", comp, length, offset)


def splanes_check(buf, outlen=None):
    """trc_splanes_check on a TRCS container in host memory (needs no device); raises TrcError with the library's reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_splanes_check(buf.ctypes.data, buf.size, (1 << 64) - 1 if outlen is None else outlen))


# ------------------------------------- byte planes behind a predictor of order 2 or 3: smooth series (include/trc_hip.h) ---
OPLANES_MAGIC = 0x4f435254                                     # "TRCO"
OPLANES_HDR = 16
ORDER_MAX = 3


def planes_split_ofilter(order, stride, d_in, n, esize, seg, d_planes, pitch, d_tail=None):
    """enqueue trc_planes_split_ofilter_dev: planes_split of the zigzagged order-th difference at `stride` (order 0 .. ORDER_MAX; 0 is
    planes_split, 1 planes_split_sfilter with FILTER_ZDELTA), restarting every seg elements"""
    _chk(lib().trc_planes_split_ofilter_dev(order, stride, d_in.data_ptr(), n, esize, seg, d_planes.data_ptr(), pitch,
                                            d_tail.data_ptr() if d_tail is not None else None, _cur_stream(d_in)))


def planes_join_ofilter(order, stride, d_planes, pitch, d_tail, n, esize, seg, d_out):
    """enqueue trc_planes_join_ofilter_dev, the inverse of planes_split_ofilter"""
    _chk(lib().trc_planes_join_ofilter_dev(order, stride, d_planes.data_ptr(), pitch, d_tail.data_ptr() if d_tail is not None else None, n,
                                           esize, seg, d_out.data_ptr(), _cur_stream(d_out)))


class OrderPlanesCoder(PlanesCoder):
    """PlanesCoder through the trc_*_oplanes_dev calls: the same buffers and results, of the zigzagged order-th difference at `stride`
    (restart = chunk).  order=1 is StridedPlanesCoder with FILTER_ZDELTA, order=0 the unfiltered coder."""
    _ENC, _DEC, _DEC_RANGE = "trc_encode_oplanes_dev", "trc_decode_oplanes_dev", "trc_decode_oplanes_range_dev"

    def __init__(self, codec, n, esize, chunk=4096, device="cuda", cdfnum=256, prm=(5, 6), guard=0, order=0, stride=1):
        super().__init__(codec, n, esize, chunk, device, cdfnum=cdfnum, prm=prm, guard=guard)
        self.order, self.stride = order, stride

    def _lead(self):
        return (self.order, self.stride)


def planes_hist_order_bytes(esize):
    return lib().trc_planes_hist_order_bytes(esize)


def planes_hist_order(orders, stride, d_in, n, esize, seg, d_hist):
    """enqueue trc_planes_hist_order_dev: the byte histograms of the planes of d_in[:n] under every order of the bit set `orders`
    (bit k = order k) at `stride`, into d_hist (4 * esize * 256 uint64 as a device tensor; zeroed by the call)"""
    _chk(lib().trc_planes_hist_order_dev(orders, stride, d_in.data_ptr(), n, esize, seg, d_hist.data_ptr(), _cur_stream(d_in)))


def _order_advice_dict(a):
    return dict(order=int(a.order), esize=int(a.esize), orders=int(a.orders), m=int(a.m),
                bits=np.array([list(r) for r in a.bits], dtype=np.float64), total_bits=np.array(list(a.total_bits), dtype=np.float64))


def planes_advise_order(hist, orders, esize, m):
    """trc_planes_advise_order on histograms in host memory (uint64 [4 * esize * 256]; needs no device) -> dict of the advice's fields"""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    if hist.size < 4 * esize * 256:                                # (a bad esize is the library's to refuse: give it something to read)
        hist = np.concatenate([hist.reshape(-1), np.zeros(4 * 8 * 256, dtype=np.uint64)])
    a = PlanesOrderAdvice()
    _chk(lib().trc_planes_advise_order(hist.ctypes.data, orders, esize, m, C.byref(a)))
    return _order_advice_dict(a)


def oplanes_bound(n, esize, chunk=0, cdfnum=0):
    return lib().trc_oplanes_bound(n, esize, chunk, cdfnum)


def host_encode_oplanes(codec, order, stride, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_oplanes_host -> the TRCO container (np.uint8): 16 bytes, then the TRCP container of the order-filtered data"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(oplanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    l = lib().trc_encode_oplanes_host(codec, order, stride, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def host_decode_oplanes(comp, n):
    return _host_decode_guarded("trc_decode_oplanes_host", comp, n)


def host_decode_oplanes_range(comp, offset, length):
    return _host_decode_guarded("trc_decode_oplanes_range_host", comp, length, offset)


def oplanes_check(buf, outlen=None):
    """trc_oplanes_check on a TRCO container in host memory (needs no device); raises TrcError with the library's reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_oplanes_check(buf.ctypes.data, buf.size, (1 << 64) - 1 if outlen is None else outlen))


def host_encode_aoplanes(codec, stride, data, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_aoplanes_host -> (the TRCP, TRCF, TRCS or TRCO container of the order the advisor chose at `stride` (np.uint8),
    dict of the advice's fields)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(oplanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    a = PlanesOrderAdvice()
    l = lib().trc_encode_aoplanes_host(codec, stride, data.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn, C.byref(a))
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy(), _order_advice_dict(a)


# ------------------------------------------------ byte planes relative to a base buffer (include/trc_hip.h) ---
BPLANES_MAGIC = 0x44435254                                     # "TRCD"
BPLANES_HDR = 32


def _ptr(t):
    return t.data_ptr() if t is not None else None


def planes_split_base(filt, d_in, d_base, n, esize, d_planes, pitch, d_tail=None):
    """enqueue trc_planes_split_base_dev: planes_split of the elements filtered against those of d_base (None with FILTER_NONE)"""
    _chk(lib().trc_planes_split_base_dev(filt, d_in.data_ptr(), _ptr(d_base), n, esize, d_planes.data_ptr(), pitch, _ptr(d_tail), _cur_stream(d_in)))


def planes_join_base(filt, d_planes, pitch, d_tail, d_base, n, esize, d_out):
    """enqueue trc_planes_join_base_dev, the inverse of planes_split_base; d_out may be d_base itself (in place)"""
    _chk(lib().trc_planes_join_base_dev(filt, d_planes.data_ptr(), pitch, _ptr(d_tail), _ptr(d_base), n, esize, d_out.data_ptr(), _cur_stream(d_out)))


class BasePlanesCoder(PlanesCoder):
    """PlanesCoder through the trc_*_bplanes_dev calls: the same buffers and results, of the elements filtered against a base that
    every call is given.  filter=FILTER_NONE is the unfiltered coder, and d_base may then be None."""

    def __init__(self, codec, n, esize, chunk=4096, device="cuda", cdfnum=256, prm=(5, 6), guard=0, filter=FILTER_NONE):
        super().__init__(codec, n, esize, chunk, device, cdfnum=cdfnum, prm=prm, guard=guard)
        self.filter = filter

    def encode(self, d_in, d_base, n=None, flags=0):
        n = self.n if n is None else n
        st = self.codec in STATIC
        _chk(lib().trc_encode_bplanes_dev(self.codec | flags, self.filter, d_in.data_ptr(), _ptr(d_base), n, self.esize, self.chunk,
                                          self.cdf.data_ptr() if st else None, self.cdfnum, self.status.data_ptr() if st else None,
                                          self.clen.data_ptr(), self.payload.data_ptr(), self.total.data_ptr(), self.tail.data_ptr(),
                                          self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode(self, d_out, d_base, n=None, flags=0):
        """d_out may be d_base itself: the delta is then applied in place"""
        n = self.n if n is None else n
        _chk(lib().trc_decode_bplanes_dev(self.codec | flags, self.filter, self.clen.data_ptr(), self.payload.data_ptr(), self.tail.data_ptr(),
                                          _ptr(d_base), n, self.esize, self.chunk, self.cdf.data_ptr() if self.codec in STATIC else None,
                                          self.cdfnum, d_out.data_ptr(), self.work.data_ptr(), self.work_bytes, self._stream()))

    def decode_range(self, d_out, d_base, first, count, n=None, flags=0):
        """elements [first * chunk, min(m, (first + count) * chunk)) to d_out[0:]; d_base is the WHOLE base"""
        n = self.n if n is None else n
        need = lib().trc_planes_range_work_bytes(self.codec, n, self.esize, self.chunk, count)
        if need > self.range_work_bytes:
            self.range_work, self.range_work_bytes = self._buf(need), need
        if self.range_work is None:
            self.range_work = self._buf(0)
        _chk(lib().trc_decode_bplanes_range_dev(self.codec | flags, self.filter, self.clen.data_ptr(), self.payload.data_ptr(), _ptr(d_base),
                                                n, self.esize, self.chunk, first, count,
                                                self.cdf.data_ptr() if self.codec in STATIC else None, self.cdfnum,
                                                d_out.data_ptr(), self.range_work.data_ptr(), self.range_work_bytes, self._stream()))


def planes_hist_base(filters, d_in, d_base, n, esize, d_hist):
    """enqueue trc_planes_hist_base_dev: planes_hist with the rows of filters 1 and 2 counted against d_base"""
    _chk(lib().trc_planes_hist_base_dev(filters, d_in.data_ptr(), _ptr(d_base), n, esize, d_hist.data_ptr(), _cur_stream(d_in)))


def base_fingerprint_enqueue(d_base, nbytes, d_fp):
    """enqueue trc_base_fingerprint_dev: the fingerprint of d_base[:nbytes] into the 8 bytes of d_fp (device tensors); does not wait"""
    _chk(lib().trc_base_fingerprint_dev(d_base.data_ptr(), nbytes, d_fp.data_ptr(), _cur_stream(d_base)))


def base_fingerprint(d_base, nbytes=None):
    """trc_base_fingerprint_dev on a uint8 device tensor -> the fingerprint (synchronises)"""
    import torch
    nbytes = d_base.numel() if nbytes is None else nbytes
    d_fp = torch.full((8,), 0xA5, dtype=torch.uint8, device=d_base.device)
    base_fingerprint_enqueue(d_base, nbytes, d_fp)
    return int(d_fp.cpu().numpy().view("<u8")[0])


def base_fingerprint_host(data):
    """trc_base_fingerprint_host (needs no device)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    return int(lib().trc_base_fingerprint_host(data.ctypes.data, data.size))


def bplanes_bound(n, esize, chunk=0, cdfnum=0):
    return lib().trc_bplanes_bound(n, esize, chunk, cdfnum)


def host_encode_bplanes(codec, filt, data, base, esize, chunk=0, cdfnum=256, prm=(5, 6)):
    """trc_encode_bplanes_host -> the TRCD container (np.uint8): 32 bytes, then the TRCP container of the data filtered against base"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    base = np.ascontiguousarray(base, dtype=np.uint8)
    if base.size < data.size - data.size % esize:
        raise ValueError("the base holds %d bytes, the elements take %d" % (base.size, data.size - data.size % esize))
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(bplanes_bound(data.size, esize, chunk, cn), 64), dtype=np.uint8)
    l = lib().trc_encode_bplanes_host(codec, filt, data.ctypes.data, base.ctypes.data, data.size, esize, chunk, out.ctypes.data, out.size, cn)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


def _host_decode_base_guarded(name, comp, base, length, offset=None):
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    base = np.ascontiguousarray(base, dtype=np.uint8)
    out = np.full(length + 64, 0xA5, dtype=np.uint8)
    f = getattr(lib(), name)
    if offset is None:
        l = f(comp.ctypes.data, comp.size, base.ctypes.data, base.size, out.ctypes.data, length)
    else:
        l = f(comp.ctypes.data, comp.size, base.ctypes.data, base.size, offset, length, out.ctypes.data)
    if l != length or not (out[length:] == 0xA5).all():
        raise TrcError(lib().trc_last_error().decode() if l != length else name + " wrote past its output")
    return out[:length].copy()


def host_decode_bplanes(comp, base, n):
    return _host_decode_base_guarded("trc_decode_bplanes_host", comp, base, n)


def host_decode_bplanes_range(comp, base, offset, length):
    return _host_decode_base_guarded("trc_decode_bplanes_range_host", comp, base, length, offset)


def bplanes_check(buf, outlen=None):
    """trc_bplanes_check on a TRCD container in host memory (needs no device); raises TrcError with the library's reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_bplanes_check(buf.ctypes.data, buf.size, (1 << 64) - 1 if outlen is None else outlen))


def encode_host_container(codec, data, chunk, cdf=None, cdfnum=256, prm=(5, 6)):
    """trc_encode_host: the TRC1 container of `data` at an explicit chunk, whatever its size"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cap = lib().trc_container_bound(data.size, chunk) + 64
    out = np.zeros(cap, dtype=np.uint8)
    st = codec in STATIC
    l = lib().trc_encode_host(codec, data.ctypes.data, data.size, chunk, out.ctypes.data, cap,
                              np.ascontiguousarray(cdf, dtype=np.uint16).ctypes.data if st else None, _cdfnum(codec, cdfnum, prm))
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy()


# ------------------------------------------------------- the TRCB container of a batch (include/trc_hip.h) ---
PLANES_BATCH_MAGIC = 0x42435254                                # "TRCB"
PLANES_BATCH_HDR = 48
ITEMS_HOST, ITEMS_DEV = 0, 1


def planes_batch_bound(codec, sizes, esize, chunk=0, cdfnum=0):
    """trc_planes_batch_bound for items of `sizes` bytes (needs no device, looks at no pointer); 0: what the calls reject"""
    return lib().trc_planes_batch_bound(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize, chunk, cdfnum)


def planes_batch_auto_chunk(codec, sizes, esize):
    return lib().trc_planes_batch_auto_chunk(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize)


def planes_batch_layout(codec, sizes, esize, chunk, cdfnum, total):
    """trc_planes_batch_layout_host -> dict(inner, off: list of esize, size)"""
    L = PlanesBatchLayout()
    tot = (C.c_uint64 * 8)(*[int(x) for x in total])
    _chk(lib().trc_planes_batch_layout_host(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize, chunk, cdfnum, tot, C.byref(L)))
    return {"inner": int(L.inner), "off": [int(x) for x in L.off[:esize]], "size": int(L.size)}


def planes_batch_check(buf, count=None):
    """trc_planes_batch_check (needs no device); raises TrcError with the reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_planes_batch_check(buf.ctypes.data, buf.size, _sz(-1).value if count is None else count))


def planes_batch_info(buf, cap=None):
    """trc_planes_batch_info -> (dict of the header's fields, n: list, filters: list) of the first min(cap, count) items"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h = PlanesBatchHdr()
    if cap is None:
        _chk(lib().trc_planes_batch_info(buf.ctypes.data, buf.size, C.byref(h), None, None, 0))
        cap = int(h.count)
    n, f = (C.c_uint64 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))()
    _chk(lib().trc_planes_batch_info(buf.ctypes.data, buf.size, C.byref(h), n, f, cap))
    got = min(cap, int(h.count))
    return {k: int(getattr(h, k)) for k, _ in PlanesBatchHdr._fields_}, [int(x) for x in n[:got]], [int(x) for x in f[:got]]


SBATCH_MAGIC = 0x54435254                                       # "TRCT"


def is_planes_sbatch(buf):
    """whether the buffer starts like a TRCT container (a TRCB container behind per-item strides)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    return buf.size >= 4 and int(buf[:4].view("<u4")[0]) == SBATCH_MAGIC


def planes_sbatch_prefix(count):
    """bytes of a TRCT container in front of its TRCB container"""
    return 16 + ((count + 15) & ~15)


def planes_sbatch_bound(codec, sizes, esize, chunk=0, cdfnum=0):
    return lib().trc_planes_sbatch_bound(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize, chunk, cdfnum)


def planes_sbatch_check(buf, count=None):
    """trc_planes_sbatch_check (needs no device); raises TrcError with the reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_planes_sbatch_check(buf.ctypes.data, buf.size, _sz(-1).value if count is None else count))


def planes_sbatch_info(buf, cap=None):
    """trc_planes_sbatch_info -> (dict of the TRCB header's fields, n: list, filters: list, strides: list) of the first min(cap, count) items"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h = PlanesBatchHdr()
    if cap is None:
        _chk(lib().trc_planes_sbatch_info(buf.ctypes.data, buf.size, C.byref(h), None, None, None, 0))
        cap = int(h.count)
    n, f, st = (C.c_uint64 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))()
    _chk(lib().trc_planes_sbatch_info(buf.ctypes.data, buf.size, C.byref(h), n, f, st, cap))
    got = min(cap, int(h.count))
    return ({k: int(getattr(h, k)) for k, _ in PlanesBatchHdr._fields_}, [int(x) for x in n[:got]], [int(x) for x in f[:got]],
            [int(x) for x in st[:got]])


OBATCH_MAGIC = 0x55435254                                       # "TRCU"


def is_planes_obatch(buf):
    """whether the buffer starts like a TRCU container (a TRCB container behind per-item strides and orders)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    return buf.size >= 4 and int(buf[:4].view("<u4")[0]) == OBATCH_MAGIC


def planes_obatch_prefix(count):
    """bytes of a TRCU container in front of its TRCB container"""
    return 16 + 2 * ((count + 15) & ~15)


def planes_obatch_bound(codec, sizes, esize, chunk=0, cdfnum=0):
    return lib().trc_planes_obatch_bound(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize, chunk, cdfnum)


def planes_obatch_check(buf, count=None):
    """trc_planes_obatch_check (needs no device); raises TrcError with the reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_planes_obatch_check(buf.ctypes.data, buf.size, _sz(-1).value if count is None else count))


def planes_obatch_info(buf, cap=None):
    """trc_planes_obatch_info -> (dict of the TRCB header's fields, n, filters, strides, orders: lists) of the first min(cap, count) items"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h = PlanesBatchHdr()
    if cap is None:
        _chk(lib().trc_planes_obatch_info(buf.ctypes.data, buf.size, C.byref(h), None, None, None, None, 0))
        cap = int(h.count)
    n, f, st, od = (C.c_uint64 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))()
    _chk(lib().trc_planes_obatch_info(buf.ctypes.data, buf.size, C.byref(h), n, f, st, od, cap))
    got = min(cap, int(h.count))
    return ({k: int(getattr(h, k)) for k, _ in PlanesBatchHdr._fields_}, [int(x) for x in n[:got]], [int(x) for x in f[:got]],
            [int(x) for x in st[:got]], [int(x) for x in od[:got]])


BBATCH_MAGIC = 0x45435254                                       # "TRCE"


def planes_bbatch_prefix(count):
    """bytes of a TRCE container in front of its TRCB container"""
    return 16 + ((8 * count + 15) & ~15)


def planes_bbatch_bound(codec, sizes, esize, chunk=0, cdfnum=0):
    return lib().trc_planes_bbatch_bound(codec, planes_items([(None, n) for n in sizes]), len(sizes), esize, chunk, cdfnum)


def planes_bbatch_check(buf, count=None):
    """trc_planes_bbatch_check (needs no device); raises TrcError with the reason"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _chk(lib().trc_planes_bbatch_check(buf.ctypes.data, buf.size, _sz(-1).value if count is None else count))


def planes_bbatch_info(buf, cap=None):
    """trc_planes_bbatch_info -> (dict of the TRCB header's fields, n: list, filters: list, base_fp: list) of the first min(cap, count) items"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h = PlanesBatchHdr()
    if cap is None:
        _chk(lib().trc_planes_bbatch_info(buf.ctypes.data, buf.size, C.byref(h), None, None, None, 0))
        cap = int(h.count)
    n, f, fp = (C.c_uint64 * max(cap, 1))(), (C.c_uint8 * max(cap, 1))(), (C.c_uint64 * max(cap, 1))()
    _chk(lib().trc_planes_bbatch_info(buf.ctypes.data, buf.size, C.byref(h), n, f, fp, cap))
    got = min(cap, int(h.count))
    return ({k: int(getattr(h, k)) for k, _ in PlanesBatchHdr._fields_}, [int(x) for x in n[:got]], [int(x) for x in f[:got]],
            [int(x) for x in fp[:got]])


def parse_planes_bbatch(buf):
    """a checked TRCE container -> parse_planes_batch of its TRCB part (offsets from the TRCB start) with prefix and base_fp: list"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h, _, _, fp = planes_bbatch_info(buf)
    prefix = planes_bbatch_prefix(h["count"])
    return dict(parse_planes_batch(buf[prefix:]), prefix=prefix, base_fp=fp)


def parse_planes_batch(buf):
    """a checked TRCB container -> dict(the header's fields, n: list, filters: list, codec, cdfnum, total: the planes' payload sizes,
    off: the sections' offsets from the TRCB start); the inner TRCP container is buf[inner:size]"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h, n, f = planes_batch_info(buf)
    inner = buf[h["inner"]:h["size"]]
    codec, esize = int(inner[4]), int(inner[6])
    cdfnum = int(inner[12:16].view("<u4")[0])
    off = [int(x) for x in inner[PLANES_HDR:PLANES_HDR + 8 * esize].view("<u8")]
    cdfb = (2 * (cdfnum + 1) + 7) & ~7 if codec in STATIC else 0
    total = [int(inner[o + cdfb + 24:o + cdfb + 32].view("<u8")[0]) for o in off]
    return dict(h, n=n, filters=f, codec=codec, cdfnum=cdfnum, total=total, off=[h["inner"] + o for o in off])


def _batch_host_items(arrays):
    """-> (trc_planes_item array, items_on, what keeps the memory alive) of numpy arrays (host) or device tensors"""
    arrays = list(arrays)
    if arrays and not isinstance(arrays[0], np.ndarray):
        keep = [t.contiguous() for t in arrays]
        return planes_items([(t.data_ptr(), t.numel() * t.element_size()) for t in keep]), ITEMS_DEV, keep
    keep = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]
    return planes_items([(a.ctypes.data, a.size) for a in keep]), ITEMS_HOST, keep


def host_encode_planes_batch(codec, arrays, esize, chunk=0, filters=None, cdfnum=256, prm=(5, 6), strides=None, orders=None):
    """trc_encode_planes_batch_host on numpy arrays (host items) or device tensors (device items): filters None, one id for all, a
    list, or "auto" (trc_encode_aplanes_batch_host) -> the TRCB container (np.uint8); with "auto": (container, the filters chosen).
    strides (see planes_strides) under which an item with a filter has a stride above 1: trc_encode_splanes_batch_host -> the TRCT
    container; other strides change nothing.  orders (see planes_orders) under which a zigzag-delta item has an order above 1:
    trc_encode_oplanes_batch_host -> the TRCU container; other orders change nothing.  orders="auto" (filters None):
    trc_encode_aoplanes_batch_host under `strides` -> (the TRCB, TRCT or TRCU container of the choice, the filters, the orders chosen)"""
    items, on, keep = _batch_host_items(arrays)
    count = len(keep)
    cn = _cdfnum(codec, cdfnum, prm)
    if isinstance(orders, str) and orders == "auto":
        if filters is not None:
            raise ValueError("orders=\"auto\" chooses the filters as well: filters must be None")
        out = np.zeros(max(lib().trc_planes_obatch_bound(codec, items, count, esize, chunk, cn), 64), dtype=np.uint8)
        cf, co = (C.c_uint8 * max(count, 1))(), (C.c_uint8 * max(count, 1))()
        l = lib().trc_encode_aoplanes_batch_host(codec, items, planes_strides(strides, count), count, esize, chunk, cn, on, out.ctypes.data, out.size, cf, co)
        if l == 0:
            raise TrcError(lib().trc_last_error().decode())
        return out[:l].copy(), [int(x) for x in cf[:count]], [int(x) for x in co[:count]]
    if orders is not None and not isinstance(filters, str):
        f, od = planes_filters(filters, count), planes_orders(orders, count)
        if f is not None and any(a == FILTER_ZDELTA and b != 1 for a, b in zip(f[:count], od[:count])):      # (a bad order: the library's to refuse)
            out = np.zeros(max(lib().trc_planes_obatch_bound(codec, items, count, esize, chunk, cn), 64), dtype=np.uint8)
            l = lib().trc_encode_oplanes_batch_host(codec, items, f, planes_strides(strides, count), od, count, esize, chunk, cn, on, out.ctypes.data, out.size)
            if l == 0:
                raise TrcError(lib().trc_last_error().decode())
            return out[:l].copy()
    if strides is not None and not isinstance(filters, str):
        f, st = planes_filters(filters, count), planes_strides(strides, count)
        if f is not None and any(a != FILTER_NONE and b != 1 for a, b in zip(f[:count], st[:count])):      # (a bad stride: the library's to refuse)
            out = np.zeros(max(lib().trc_planes_sbatch_bound(codec, items, count, esize, chunk, cn), 64), dtype=np.uint8)
            l = lib().trc_encode_splanes_batch_host(codec, items, f, st, count, esize, chunk, cn, on, out.ctypes.data, out.size)
            if l == 0:
                raise TrcError(lib().trc_last_error().decode())
            return out[:l].copy()
    out = np.zeros(max(lib().trc_planes_batch_bound(codec, items, count, esize, chunk, cn), 64), dtype=np.uint8)
    if isinstance(filters, str) and filters == "auto":
        chosen = (C.c_uint8 * max(count, 1))()
        l = lib().trc_encode_aplanes_batch_host(codec, items, count, esize, chunk, cn, on, out.ctypes.data, out.size, chosen)
    else:
        chosen = None
        l = lib().trc_encode_planes_batch_host(codec, items, planes_filters(filters, count), count, esize, chunk, cn, on, out.ctypes.data, out.size)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy() if chosen is None else (out[:l].copy(), [int(x) for x in chosen[:count]])


def _host_bases(bases, on, count):
    """-> (the host array of base addresses the host calls take, what keeps the memory alive): numpy arrays where the items are
    host arrays, device tensors where they are tensors, None for no base"""
    if bases is None:
        return None, []
    keep = [None if b is None else (np.ascontiguousarray(b).reshape(-1).view(np.uint8) if on == ITEMS_HOST else b.contiguous()) for b in bases]
    return planes_bases([None if b is None else (b.ctypes.data if on == ITEMS_HOST else b.data_ptr()) for b in keep], count), keep


def host_encode_bplanes_batch(codec, arrays, bases, esize, chunk=0, filters=None, cdfnum=256, prm=(5, 6)):
    """trc_encode_bplanes_batch_host on numpy arrays (host items and bases) or device tensors: filters one id for all, a list, or "auto"
    (trc_encode_abplanes_batch_host) -> the TRCE container (np.uint8); with "auto": (the TRCE or TRCB container, the filters chosen)"""
    items, on, keep = _batch_host_items(arrays)
    count = len(keep)
    b, keep_b = _host_bases(bases, on, count)
    cn = _cdfnum(codec, cdfnum, prm)
    out = np.zeros(max(lib().trc_planes_bbatch_bound(codec, items, count, esize, chunk, cn), 64), dtype=np.uint8)
    if isinstance(filters, str) and filters == "auto":
        chosen = (C.c_uint8 * max(count, 1))()
        l = lib().trc_encode_abplanes_batch_host(codec, items, b, count, esize, chunk, cn, on, out.ctypes.data, out.size, chosen)
    else:
        chosen = None
        l = lib().trc_encode_bplanes_batch_host(codec, items, b, planes_filters(filters, count), count, esize, chunk, cn, on, out.ctypes.data, out.size)
    if l == 0:
        raise TrcError(lib().trc_last_error().decode())
    return out[:l].copy() if chosen is None else (out[:l].copy(), [int(x) for x in chosen[:count]])


def host_decode_bplanes_batch(comp, bases, first_item=0, item_count=None, out=None):
    """trc_decode_bplanes_batch_host: items [first_item, first_item + item_count) of a TRCE (or TRCB) container against `bases` (numpy
    arrays, or device tensors with `out`; None where an item has none or outside the range) -> a list of np.uint8 arrays, or, out given
    (a list of count device tensors, None outside the range), into those -> the bytes delivered.  The bases are verified first"""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    based = comp.size >= 4 and int(comp[:4].view("<u4")[0]) == BBATCH_MAGIC
    h, n = planes_bbatch_info(comp)[:2] if based else planes_batch_info(comp)[:2]
    count = h["count"]
    item_count = count - first_item if item_count is None else item_count
    wanted = range(first_item, first_item + item_count)
    if out is None:
        res = [np.full(n[i] + 64, 0xA5, dtype=np.uint8) if i in wanted else None for i in range(count)]
        items = planes_items([(res[i].ctypes.data if i in wanted else None, n[i]) for i in range(count)])
        on = ITEMS_HOST
    else:
        items = planes_items([(out[i].data_ptr() if out[i] is not None else None, n[i]) for i in range(count)])
        on = ITEMS_DEV
    b, keep_b = _host_bases(bases, on, count)
    l = lib().trc_decode_bplanes_batch_host(comp.ctypes.data, comp.size, items, b, count, first_item, item_count, on)
    if l != sum(n[i] for i in wanted):
        raise TrcError(lib().trc_last_error().decode())
    if out is not None:
        return l
    if any((res[i][n[i]:] != 0xA5).any() for i in wanted):
        raise TrcError("trc_decode_bplanes_batch_host wrote past an item")
    return [res[i][:n[i]].copy() for i in wanted]


def host_decode_planes_batch(comp, first_item=0, item_count=None, out=None, sizes=None):
    """trc_decode_planes_batch_host (trc_decode_splanes_batch_host where comp is a TRCT container, trc_decode_oplanes_batch_host where it
    is a TRCU container): items [first_item, first_item +
    item_count) of a TRCB container -> a list of np.uint8 arrays, or,
    out given (a list of count device tensors, None outside the range), into those -> the bytes delivered.  sizes: what the call is
    told the items hold instead of the container's own table (the tests' argument errors)"""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    strided, ordered = is_planes_sbatch(comp), is_planes_obatch(comp)
    h, n = planes_obatch_info(comp)[:2] if ordered else planes_sbatch_info(comp)[:2] if strided else planes_batch_info(comp)[:2]
    count = h["count"]
    item_count = count - first_item if item_count is None else item_count
    sizes = n if sizes is None else sizes
    wanted = range(first_item, first_item + item_count)
    if out is None:
        res = [np.full(n[i] + 64, 0xA5, dtype=np.uint8) if i in wanted else None for i in range(count)]
        items = planes_items([(res[i].ctypes.data if i in wanted else None, sizes[i]) for i in range(count)])
        on = ITEMS_HOST
    else:
        items = planes_items([(out[i].data_ptr() if out[i] is not None else None, sizes[i]) for i in range(count)])
        on = ITEMS_DEV
    l = (lib().trc_decode_oplanes_batch_host if ordered else lib().trc_decode_splanes_batch_host if strided else lib().trc_decode_planes_batch_host)(comp.ctypes.data, comp.size, items, count, first_item, item_count, on)
    if l != sum(n[i] for i in wanted):
        raise TrcError(lib().trc_last_error().decode())
    if out is not None:
        return l
    if any((res[i][n[i]:] != 0xA5).any() for i in wanted):
        raise TrcError("trc_decode_planes_batch_host wrote past an item")
    return [res[i][:n[i]].copy() for i in wanted]
