"""Records what the byte-plane entry points REFUSE, and in which order they look: tests/golden/planes_refusals.json.

    python tests/golden/make_planes_refusals.py [path/to/libturborc_hip.so]

Every case is one call through ctypes that must be refused before a device is asked for: device pointers are never dereferenced in
a refused call, so they are fake, suitably aligned integers, and the file is the same on a machine with or without a GPU.  For every entry
point the cases come from one valid call and an ORDERED list of defects: one case per defect, and for every two neighbouring defects
one case with both, whose recorded text tells which check runs first (two defects of the same argument cannot be combined and are
skipped).  The file holds, per group, the entry point, the valid call's arguments, one line per single defect -- [name, the
parameters it sets and their values, the return value, the text of trc_last_error()] -- and the pairs: "a+b" sets what a and b set,
and its refusal is the named case's, or [return value, text] where it is neither's.  The parameters' kinds and names stand once
per entry point under "signatures", and an array, a buffer or a text that many cases share stands once under "values".

A recorded int call returned TRC_E_ARG, TRC_E_WORK or TRC_E_CDF; a recorded size_t call returned 0 with a text of its own that is
not the one of a missing device or a HIP error.  Anything else stops the generator: no case can pass by reaching the device.
tests/test_planes_refusals_cpu.py replays the file against the current build (run_case below is shared with it).
"""
import ctypes as C
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "planes_refusals.json")
E_ARG, E_WORK, E_CDF = -1, -3, -4
RCA, ANS4S, ANSB, RC4, RCSS, NOCODEC, TABLES_READY = 4, 1, 13, 58, 62, 42, 0x100


class Item(C.Structure):
    _fields_ = [("d_ptr", C.c_void_p), ("n", C.c_uint64)]


# ---- marshalling: a JSON value and the kind of the parameter it goes to -------------------------------------------------------------
# kinds: i int, u unsigned / uint32_t, z size_t, p pointer.  A pointer is null, a fake address (an integer) or host memory:
#   {"items": [[ptr, n], ..]}  {"u8": [..]}  {"u64": [..]}  {"ptrs": [address or null, ..]}  {"hex": ".."}  {"buf": bytes}
def _arg(kind, v, keep):
    if kind == "i":
        return C.c_int(v)
    if kind == "u":
        return C.c_uint(v)
    if kind == "z":
        return C.c_size_t(v)
    if v is None or isinstance(v, int):
        return C.c_void_p(v)
    (tag, x), = v.items()
    if tag == "items":
        a = (Item * max(len(x), 1))(*[Item(p, n) for p, n in x])
    elif tag == "u8":
        a = (C.c_uint8 * max(len(x), 1))(*x)
    elif tag == "u64":
        a = (C.c_uint64 * max(len(x), 1))(*x)
    elif tag == "ptrs":
        a = (C.c_void_p * max(len(x), 1))(*x)
    elif tag == "hex":
        a = C.create_string_buffer(bytes.fromhex(x), max(len(x) // 2, 1))
    else:
        a = C.create_string_buffer(x)
    keep.append(a)
    return C.cast(a, C.c_void_p)


SENTINEL = "planes_advise: null histogram or advice"


def run_case(lib, name, values, sigs):
    """(return value, text) of one call of entry point `name`; the text is None where the call left none of its own"""
    fn = getattr(lib, name)
    fn.restype = C.c_int if sigs[name][0] == "int" else C.c_size_t
    fn.argtypes = None
    keep = []
    args = [_arg(k, v, keep) for (_, k), v in zip(sig(sigs[name][1]), values)]
    lib.trc_last_error.restype = C.c_char_p
    lib.trc_planes_advise.restype = C.c_int
    assert lib.trc_planes_advise(None, 1, 2, 1, None) == E_ARG          # leaves SENTINEL behind: a call that says nothing shows
    rc = fn(*args)
    text = lib.trc_last_error().decode()
    return rc, (None if text == SENTINEL else text)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def sig(s):
    return [tuple(a.split(":")) for a in s.split()]


ENC_TAIL = "d_cdf:p cdfnum:u d_status:p d_clen:p d_payload:p d_total:p d_tail:p d_work:p work_bytes:z stream:p"
DEC_TAIL = "n:z esize:u chunk:u d_cdf:p cdfnum:u d_out:p d_work:p work_bytes:z stream:p"
RNG_TAIL = "n:z esize:u chunk:u first_chunk:z count:z d_cdf:p cdfnum:u d_out:p d_work:p work_bytes:z stream:p"
BENC_TAIL = "count:z esize:u chunk:u d_cdf:p cdfnum:u d_status:p d_clen:p d_payload:p d_total:p d_work:p work_bytes:z stream:p"
BDEC_TAIL = "count:z first_item:z item_count:z esize:u chunk:u d_cdf:p cdfnum:u d_work:p work_bytes:z stream:p"
SPLIT_TAIL = "count:z esize:u chunk:u d_planes:p pitch:z d_table:p table_bytes:z stream:p"
JOIN_TAIL = "count:z first_item:z item_count:z esize:u chunk:u d_table:p table_bytes:z stream:p"
PACK_TAIL = "count:z esize:u chunk:u d_cdf:p cdfnum:u d_status:p d_clen:p d_payload:p d_total:p d_out:p out_bytes:z d_size:p stream:p"
PDEC_TAIL = "count:z first_item:z item_count:z esize:u chunk:u cdfnum:u total:p d_work:p work_bytes:z stream:p"
HENC_TAIL = "n:z esize:u chunk:u out:p outcap:z cdfnum:u"
BHENC_TAIL = "count:z esize:u chunk:u cdfnum:u items_on:i out:p outcap:z"
SIGS = {
    "trc_encode_planes_dev": ("int", "codec:i d_in:p n:z esize:u chunk:u " + ENC_TAIL),
    "trc_encode_fplanes_dev": ("int", "codec:i filter:i d_in:p n:z esize:u chunk:u " + ENC_TAIL),
    "trc_encode_splanes_dev": ("int", "codec:i filter:i stride:i d_in:p n:z esize:u chunk:u " + ENC_TAIL),
    "trc_encode_bplanes_dev": ("int", "codec:i filter:i d_in:p d_base:p n:z esize:u chunk:u " + ENC_TAIL),
    "trc_decode_planes_dev": ("int", "codec:i d_clen:p d_payload:p d_tail:p " + DEC_TAIL),
    "trc_decode_fplanes_dev": ("int", "codec:i filter:i d_clen:p d_payload:p d_tail:p " + DEC_TAIL),
    "trc_decode_splanes_dev": ("int", "codec:i filter:i stride:i d_clen:p d_payload:p d_tail:p " + DEC_TAIL),
    "trc_decode_bplanes_dev": ("int", "codec:i filter:i d_clen:p d_payload:p d_tail:p d_base:p " + DEC_TAIL),
    "trc_decode_planes_range_dev": ("int", "codec:i d_clen:p d_payload:p " + RNG_TAIL),
    "trc_decode_fplanes_range_dev": ("int", "codec:i filter:i d_clen:p d_payload:p " + RNG_TAIL),
    "trc_decode_splanes_range_dev": ("int", "codec:i filter:i stride:i d_clen:p d_payload:p " + RNG_TAIL),
    "trc_decode_bplanes_range_dev": ("int", "codec:i filter:i d_clen:p d_payload:p d_base:p " + RNG_TAIL),
    "trc_planes_split_batch_dev": ("int", "items:p " + SPLIT_TAIL),
    "trc_planes_split_fbatch_dev": ("int", "items:p filters:p " + SPLIT_TAIL),
    "trc_planes_split_sbatch_dev": ("int", "items:p filters:p strides:p " + SPLIT_TAIL),
    "trc_planes_split_bbatch_dev": ("int", "items:p bases:p filters:p " + SPLIT_TAIL),
    "trc_planes_join_batch_dev": ("int", "d_planes:p pitch:z items:p " + JOIN_TAIL),
    "trc_planes_join_fbatch_dev": ("int", "d_planes:p pitch:z items:p filters:p " + JOIN_TAIL),
    "trc_planes_join_sbatch_dev": ("int", "d_planes:p pitch:z items:p filters:p strides:p " + JOIN_TAIL),
    "trc_planes_join_bbatch_dev": ("int", "d_planes:p pitch:z items:p bases:p filters:p " + JOIN_TAIL),
    "trc_encode_planes_batch_dev": ("int", "codec:i items:p " + BENC_TAIL),
    "trc_encode_fplanes_batch_dev": ("int", "codec:i items:p filters:p " + BENC_TAIL),
    "trc_encode_splanes_batch_dev": ("int", "codec:i items:p filters:p strides:p " + BENC_TAIL),
    "trc_encode_bplanes_batch_dev": ("int", "codec:i items:p bases:p filters:p " + BENC_TAIL),
    "trc_decode_planes_batch_dev": ("int", "codec:i d_clen:p d_payload:p items:p " + BDEC_TAIL),
    "trc_decode_fplanes_batch_dev": ("int", "codec:i d_clen:p d_payload:p items:p filters:p " + BDEC_TAIL),
    "trc_decode_splanes_batch_dev": ("int", "codec:i d_clen:p d_payload:p items:p filters:p strides:p " + BDEC_TAIL),
    "trc_decode_bplanes_batch_dev": ("int", "codec:i d_clen:p d_payload:p items:p bases:p filters:p " + BDEC_TAIL),
    "trc_planes_batch_pack_dev": ("int", "codec:i items:p filters:p " + PACK_TAIL),
    "trc_planes_sbatch_pack_dev": ("int", "codec:i items:p filters:p strides:p " + PACK_TAIL),
    "trc_decode_planes_batch_packed_dev": ("int", "codec:i d_cont:p cont_bytes:z items:p filters:p " + PDEC_TAIL),
    "trc_decode_splanes_batch_packed_dev": ("int", "codec:i d_cont:p cont_bytes:z items:p filters:p strides:p " + PDEC_TAIL),
    "trc_planes_batch_work_bytes": ("size", "codec:i items:p count:z esize:u chunk:u"),
    "trc_planes_batch_range_work_bytes": ("size", "codec:i items:p count:z esize:u chunk:u first_item:z item_count:z"),
    "trc_planes_bbatch_work_bytes": ("size", "codec:i items:p count:z esize:u chunk:u"),
    "trc_planes_bbatch_range_work_bytes": ("size", "codec:i items:p count:z esize:u chunk:u first_item:z item_count:z"),
    "trc_fplanes_check": ("int", "buf:p buflen:z outlen:z"),
    "trc_splanes_check": ("int", "buf:p buflen:z outlen:z"),
    "trc_bplanes_check": ("int", "buf:p buflen:z outlen:z"),
    "trc_encode_planes_host": ("size", "codec:i in:p " + HENC_TAIL),
    "trc_encode_fplanes_host": ("size", "codec:i filter:i in:p " + HENC_TAIL),
    "trc_encode_splanes_host": ("size", "codec:i filter:i stride:i in:p " + HENC_TAIL),
    "trc_encode_bplanes_host": ("size", "codec:i filter:i in:p base:p " + HENC_TAIL),
    "trc_encode_aplanes_host": ("size", "codec:i in:p " + HENC_TAIL + " advice:p"),
    "trc_decode_planes_host": ("size", "in:p inlen:z out:p outlen:z"),
    "trc_decode_fplanes_host": ("size", "in:p inlen:z out:p outlen:z"),
    "trc_decode_splanes_host": ("size", "in:p inlen:z out:p outlen:z"),
    "trc_decode_xplanes_host": ("size", "in:p inlen:z out:p outlen:z"),
    "trc_decode_bplanes_host": ("size", "in:p inlen:z base:p base_len:z out:p outlen:z"),
    "trc_decode_planes_range_host": ("size", "in:p inlen:z offset:z len:z out:p"),
    "trc_decode_fplanes_range_host": ("size", "in:p inlen:z offset:z len:z out:p"),
    "trc_decode_splanes_range_host": ("size", "in:p inlen:z offset:z len:z out:p"),
    "trc_decode_bplanes_range_host": ("size", "in:p inlen:z base:p base_len:z offset:z len:z out:p"),
    "trc_encode_planes_batch_host": ("size", "codec:i items:p filters:p " + BHENC_TAIL),
    "trc_encode_splanes_batch_host": ("size", "codec:i items:p filters:p strides:p " + BHENC_TAIL),
    "trc_encode_aplanes_batch_host": ("size", "codec:i items:p " + BHENC_TAIL + " filters_out:p"),
    "trc_decode_planes_batch_host": ("size", "in:p inlen:z items:p count:z first_item:z item_count:z items_on:i"),
    "trc_decode_splanes_batch_host": ("size", "in:p inlen:z items:p count:z first_item:z item_count:z items_on:i"),
}

SIGNATURES = {fn: [ret, s] for fn, (ret, s) in SIGS.items()}       # as the file holds them


def params(sigs, fn):
    return [n for n, _ in sig(sigs[fn][1])]


# ---- hand-built containers -----------------------------------------------------------------------------------------------------------
def trc1(byte):          # the TRC1 container of one byte, stored raw, coder RCA, chunk 256 (padded to a multiple of 8)
    return struct.pack("<IBBHIIQQ", 0x31435254, RCA, 1, 0, 256, 1, 1, 1) + struct.pack("<I", 1) + bytes([byte]) + bytes(3)


def trcp():              # the TRCP container of one 2-byte element
    body = struct.pack("<QQ", 48, 88) + trc1(0x34) + trc1(0x12)
    return struct.pack("<IBBBBIIQQ", 0x50435254, RCA, 1, 2, 0, 256, 0, 2, 32 + len(body)) + body


def prefix16(magic, filt, field, size):      # trc_fplanes_hdr / trc_splanes_hdr
    return struct.pack("<IBBHQ", magic, filt, 1, field, size)


def trcf(filt=1, zero=0, grow=0):
    return prefix16(0x46435254, filt, zero, 16 + len(trcp()) + grow) + trcp()


def trcs(filt=1, stride=2, grow=0):
    return prefix16(0x53435254, filt, stride, 16 + len(trcp()) + grow) + trcp()


def trcd(filt=1, zero=0, grow=0, base_bytes=2):
    return struct.pack("<IBBHQQQ", 0x44435254, filt, 1, zero, 32 + len(trcp()) + grow, base_bytes, 0) + trcp()


def trcb(n=2):           # the TRCB container of a batch of one item, no filter
    return struct.pack("<IBBHIIQQQQ", 0x42435254, 1, 2, 0, 256, 0, 1, 64, 64 + len(trcp()), n) + struct.pack("<Q", n) + bytes(8) + trcp()


def trct(stride=1):
    return struct.pack("<IBBHQ", 0x54435254, 1, 0, 0, 1) + bytes([stride]) + bytes(15) + trcb()


def hexbuf(b):
    return {"hex": b.hex()}


# ---- valid calls and their ordered defects -------------------------------------------------------------------------------------------
A = 0x100000            # fake device addresses, 1 MiB apart and so aligned to anything asked for
ITEMS = {"items": [[16 * A, 4096], [17 * A, 20], [18 * A, 1000]]}
BAD_PLAN = {"items": [[16 * A, 4096], [17 * A, 21], [18 * A, 1000]]}
BAD_PTR = {"items": [[16 * A, 4096], [17 * A + 8, 20], [18 * A, 1000]]}
BAD_PTR0 = {"items": [[16 * A + 8, 4096], [17 * A, 20], [18 * A, 1000]]}
NULL_PTR = {"items": [[16 * A, 4096], [None, 20], [18 * A, 1000]]}
F_SET, F_NONE, F_BAD = {"u8": [1, 0, 2]}, {"u8": [0, 0, 0]}, {"u8": [1, 0, 3]}
S_SET, S_ONE, S_BAD = {"u8": [2, 1, 3]}, {"u8": [1, 1, 1]}, {"u8": [2, 9, 3]}
BASES, BASES_NULL, BASES_OFF = {"ptrs": [20 * A, None, 21 * A]}, {"ptrs": [20 * A, None, None]}, {"ptrs": [20 * A + 8, None, 21 * A]}
FLAT = dict(codec=RCA, filter=1, stride=2, d_in=A, d_base=9 * A, n=4100, esize=4, chunk=256, d_cdf=None, cdfnum=0, d_status=None,
            d_clen=2 * A, d_payload=3 * A, d_total=4 * A, d_tail=5 * A, d_work=6 * A, work_bytes=1 << 30, stream=None, d_out=7 * A,
            first_chunk=1, count=2)
COMMON = [("tables_ready", dict(codec=RCA | TABLES_READY)), ("low4", dict(codec=RC4)), ("esize", dict(esize=3)), ("short", dict(n=2)),
          ("work_align", dict(d_work=6 * A + 16)), ("no_codec", dict(codec=NOCODEC)), ("chunk", dict(chunk=100)),
          ("many_chunks", dict(n=1 << 47)), ("chunk_max", dict(codec=ANSB, chunk=16384)), ("no_cdf", dict(codec=ANS4S)),
          ("ss_prm", dict(codec=RCSS))]
STATUS = [("no_status", dict(codec=ANS4S, d_cdf=8 * A, cdfnum=256)), None, ("status", dict(d_status=10 * A))]      # (None: no pair across -- the two cancel)
WORK = ("work_small", dict(work_bytes=4096))


def flat(kind):
    lead = {"planes": [], "fplanes": [("filter", dict(filter=3))], "splanes": [("stride", dict(stride=9)), ("filter", dict(filter=3))],
            "bplanes": [("filter", dict(filter=3)), ("base_null", dict(d_base=None)), ("base_align", dict(d_base=9 * A + 8))]}[kind]
    over = [("overlap", dict(d_base=7 * A + 16))] if kind == "bplanes" else []
    yield "trc_encode_%s_dev" % kind, FLAT, lead + COMMON + STATUS + [WORK, ("payload_align", dict(d_payload=3 * A + 1)), ("no_in", dict(d_in=None))]
    yield "trc_decode_%s_dev" % kind, FLAT, lead + COMMON + [WORK, ("out_align", dict(d_out=7 * A + 8)), ("no_tail", dict(n=4101, d_tail=None))] + over
    yield "trc_decode_%s_range_dev" % kind, FLAT, lead + COMMON + [("range", dict(first_chunk=4, count=2)), WORK, ("out_align", dict(d_out=7 * A + 8))] + over


BATCH = dict(codec=RCA, items=ITEMS, filters=F_SET, strides=S_SET, bases=BASES, count=3, first_item=1, item_count=2, esize=4, chunk=256,
             d_cdf=None, cdfnum=0, d_status=None, d_clen=2 * A, d_payload=3 * A, d_total=4 * A, d_work=6 * A, work_bytes=1 << 30, stream=None,
             d_planes=5 * A, pitch=1 << 16, d_table=8 * A, table_bytes=1 << 20, d_out=7 * A, out_bytes=1 << 30, d_size=9 * A,
             d_cont=10 * A, cont_bytes=1 << 30, total={"u64": [10, 10, 10, 10]})
PLAN = [("no_items", dict(count=0)), ("plan_esize", dict(esize=3)), ("plan_chunk", dict(chunk=100)), ("plan_item", dict(items=BAD_PLAN))]


def lead_batch(kind):
    return PLAN + {"": [], "f": [("filter", dict(filters=F_BAD))], "s": [("filter", dict(filters=F_BAD)), ("stride", dict(strides=S_BAD))],
                   "b": [("filter", dict(filters=F_BAD))]}[kind]


def batch_split_join(kind):
    base = [("base_null", dict(bases=BASES_NULL)), ("base_align", dict(bases=BASES_OFF)), ("no_bases", dict(bases=None))] if kind == "b" else []
    bufs = [("planes_align", dict(d_planes=5 * A + 64)), ("pitch", dict(pitch=1000)), ("table_align", dict(d_table=8 * A + 16)),
            ("table_small", dict(table_bytes=256))]
    yield "trc_planes_split_%sbatch_dev" % kind, BATCH, lead_batch(kind) + bufs + [("item_ptr", dict(items=BAD_PTR0))] + base
    jbufs = [("planes_align", dict(d_planes=5 * A + 32))] + bufs[1:]
    yield "trc_planes_join_%sbatch_dev" % kind, BATCH, lead_batch(kind) + [("range", dict(first_item=2, item_count=2)), ("item_ptr", dict(items=BAD_PTR))] + \
        [(l, d) for l, d in base if l != "base_align"] + jbufs
    if kind != "":      # the renaming rules: an all-NONE batch, a strided call without an effective stride
        for fn in ("trc_planes_split_%sbatch_dev", "trc_planes_join_%sbatch_dev"):
            yield fn % kind, dict(BATCH, filters=F_NONE), [("none_pitch", dict(pitch=1000)), ("none_table", dict(table_bytes=256))]
            yield fn % kind, dict(BATCH, filters=None), [("null_pitch", dict(pitch=1000)), ("null_plan", dict(count=0))]
    if kind == "s":
        for fn in ("trc_planes_split_sbatch_dev", "trc_planes_join_sbatch_dev"):
            yield fn, dict(BATCH, strides=S_ONE), [("unstrided_pitch", dict(pitch=1000)), ("unstrided_table", dict(table_bytes=256))]
    if kind == "b":     # an item without a filter needs no base; the table of a call against bases is larger
        yield "trc_planes_split_bbatch_dev", dict(BATCH, table_bytes=512), [("table_with_bases", dict())]
        yield "trc_planes_join_bbatch_dev", dict(BATCH, table_bytes=512), [("table_with_bases", dict())]


def batch_coded(kind):
    p = {"": "planes", "f": "fplanes", "s": "splanes", "b": "bplanes"}[kind]
    base = [("base_null", dict(bases=BASES_NULL)), ("no_bases", dict(bases=None))] if kind == "b" else []
    yield "trc_encode_%s_batch_dev" % p, BATCH, lead_batch(kind) + COMMON[:7] + COMMON[8:] + STATUS + [("item_ptr", dict(items=BAD_PTR))] + base + \
        [WORK, ("payload_align", dict(d_payload=3 * A + 1))]
    yield "trc_decode_%s_batch_dev" % p, BATCH, lead_batch(kind) + COMMON[:7] + COMMON[8:] + [("range", dict(first_item=2, item_count=2)), ("item_ptr", dict(items=BAD_PTR))] + \
        base + [WORK, ("payload_align", dict(d_payload=3 * A + 1))]
    if kind == "b":     # the workspace of a call against bases holds their table as well; filters == NULL is the unfiltered call
        for fn, wb in (("trc_encode_bplanes_batch_dev", "trc_planes_batch_work_bytes"), ("trc_decode_bplanes_batch_dev", "trc_planes_batch_range_work_bytes")):
            yield fn, BATCH, [("work_of_plain_call", {"work_bytes": ("work", wb)})]
            yield fn, dict(BATCH, filters=F_NONE), [("none_work_of_plain_call", {"work_bytes": ("work", wb)}), ("none_esize", dict(esize=3))]
            yield fn, dict(BATCH, filters=None), [("null_esize", dict(esize=3)), ("null_work", dict(work_bytes=4096))]


def packs():
    common = [c for c in COMMON if c[0] not in ("short", "work_align", "many_chunks")]
    bufs = [("payload_align", dict(d_payload=3 * A + 2)), ("out_align", dict(d_out=7 * A + 8)), ("out_small", dict(out_bytes=64))]
    yield "trc_planes_batch_pack_dev", BATCH, lead_batch("f") + common + STATUS + bufs
    yield "trc_planes_sbatch_pack_dev", BATCH, lead_batch("s") + [("unstrided", dict(strides=S_ONE)), ("prefix_room", dict(out_bytes=8))] + common[:3]
    pd = [("cont_align", dict(d_cont=10 * A + 4)), ("no_total", dict(total=None)), ("total", dict(total={"u64": [1 << 40, 0, 0, 0]})),
          ("cont_small", dict(cont_bytes=64))]
    dec = COMMON[5:7] + COMMON[8:] + [("range", dict(first_item=2, item_count=2)), ("item_ptr", dict(items=BAD_PTR)), WORK]
    yield "trc_decode_planes_batch_packed_dev", BATCH, lead_batch("f") + common[1:3] + pd + [COMMON[4]] + dec
    yield "trc_decode_splanes_batch_packed_dev", BATCH, lead_batch("s") + common[1:3] + pd + [COMMON[4]] + dec


def work_bytes():
    for b in ("", "b"):
        yield "trc_planes_%sbatch_work_bytes" % b, BATCH, [("size", dict()), ("one_item", dict(count=1))] + PLAN + [("item_ptr", dict(items=BAD_PTR)), ("low4", dict(codec=RC4)),
                                                                                                      ("no_codec", dict(codec=NOCODEC))]
        yield "trc_planes_%sbatch_range_work_bytes" % b, BATCH, [("size", dict()), ("one_item", dict(item_count=1))] + PLAN + \
            [("range", dict(first_item=2, item_count=2)), ("empty", dict(item_count=0)), ("item_ptr", dict(items=BAD_PTR)), ("low4", dict(codec=RC4))]


def checks():
    def buf(b, **kw):
        return dict(dict(buf=hexbuf(b), buflen=len(b)), **kw)
    for fn, mk, own in (("trc_fplanes_check", trcf, ("reserved", dict(zero=7))), ("trc_splanes_check", trcs, ("stride", dict(stride=1))),
                        ("trc_bplanes_check", trcd, ("reserved", dict(zero=7)))):
        good = mk()
        yield fn, buf(good, outlen=2), [("null", dict(buf=None)), ("short", dict(buflen=8)), ("magic", buf(b"XXXX" + good[4:])), ("version", buf(good[:5] + b"\x02" + good[6:])),
                              ("filter", buf(mk(filt=0))), ("filter3", buf(mk(filt=3))), ("filter_and_own", buf(mk(0, own[1][list(own[1])[0]]))),
                              (own[0], buf(mk(**own[1]))), (own[0] + "_and_size", buf(mk(grow=8, **own[1]))), ("size", buf(mk(grow=8))),
                              ("no_room", buf(mk(grow=-len(trcp())))), ("inner", dict(outlen=4))]
    yield "trc_splanes_check", buf(trcs(), outlen=2), [("stride9", buf(trcs(stride=9)))]
    yield "trc_bplanes_check", buf(trcd(), outlen=2), [("inner_and_base_bytes", buf(trcd(base_bytes=4), outlen=4)), ("base_bytes", buf(trcd(base_bytes=4)))]


HOST = dict(codec=RCA, filter=1, stride=2, n=4100, esize=4, chunk=256, out={"buf": 64}, outcap=1 << 20, cdfnum=0, advice=None, base={"buf": 16})
HOST["in"] = {"buf": 16}


def host_encoders():
    inner = [("no_codec", dict(codec=NOCODEC)), ("low4", dict(codec=RC4)), ("no_in", {"in": None}), ("esize", dict(esize=3)), ("short", dict(n=2)),
             ("chunk", dict(chunk=100)), ("chunk_too_large", dict(codec=ANSB, chunk=65600))]
    bad_filter = [("filter0", dict(filter=0)), ("filter3", dict(filter=3))]
    room = [("no_out", dict(out=None)), ("no_room", dict(outcap=16))]
    yield "trc_encode_planes_host", HOST, inner + [("no_out", dict(out=None))]
    yield "trc_encode_aplanes_host", HOST, inner + [("no_out", dict(out=None))]
    yield "trc_encode_fplanes_host", HOST, bad_filter + room + inner
    yield "trc_encode_splanes_host", HOST, [("stride0", dict(stride=0)), ("stride9", dict(stride=9))] + bad_filter + [("stride1", dict(stride=1))] + room + inner
    yield "trc_encode_bplanes_host", HOST, bad_filter + [("no_base", dict(base=None)), ("no_out", dict(out=None)), ("no_room", dict(outcap=32))] + inner


def host_decoders():
    def args(b, **kw):
        d = dict(inlen=len(b), out={"buf": 16}, outlen=2, offset=0, len=2, base={"buf": 16}, base_len=2)
        d["in"] = hexbuf(b)
        return dict(d, **kw)
    def cont(b):
        return {"in": hexbuf(b), "inlen": len(b)}
    p = trcp()
    for fn in ("trc_decode_planes_host", "trc_decode_xplanes_host"):
        yield fn, args(p), [("no_in", {"in": None}), ("no_out", dict(out=None)), ("short", dict(inlen=8)), ("outlen", dict(outlen=4))]
    yield "trc_decode_xplanes_host", args(trcd()), [("against_a_base", dict())]
    yield "trc_decode_xplanes_host", args(trcb()), [("another_container", dict())]
    yield "trc_decode_xplanes_host", args(trcf(0)), [("a_prefix_is_checked", dict())]
    yield "trc_decode_xplanes_host", args(trcs(1, 1)), [("a_prefix_is_checked", dict())]
    yield "trc_decode_planes_range_host", args(p), [("no_out", dict(out=None)), ("short", dict(inlen=8)), ("empty", dict(len=0)), ("past_end", dict(offset=1, len=2))]
    for name, mk in (("fplanes", trcf), ("splanes", trcs)):
        yield "trc_decode_%s_host" % name, args(mk()), [("no_out", dict(out=None)), ("prefix", cont(mk(filt=0))), ("inner", dict(outlen=4))]
        yield "trc_decode_%s_range_host" % name, args(mk()), [("no_in", {"in": None}), ("prefix", cont(mk(grow=8))), ("inner", cont(mk()[:16] + b"XXXX" + mk()[20:])),
                                                              ("past_end", dict(offset=2, len=1))]
    d = trcd()
    yield "trc_decode_bplanes_host", args(d), [("no_out", dict(out=None)), ("prefix", cont(trcd(zero=1))), ("outlen", dict(outlen=4)), ("base_bytes", cont(trcd(base_bytes=4))),
                                               ("no_base", dict(base=None)), ("base_short", dict(base_len=1))]
    yield "trc_decode_bplanes_range_host", args(d), [("no_in", {"in": None}), ("prefix", cont(trcd(filt=3))), ("no_base", dict(base=None)), ("base_short", dict(base_len=1)),
                                                     ("past_end", dict(offset=1, len=2))]


BHOST = dict(codec=RCA, items=ITEMS, filters=F_SET, strides=S_SET, count=3, esize=4, chunk=256, cdfnum=0, items_on=1, out={"buf": 64}, outcap=1 << 20, filters_out=None)


def batch_host():
    front = [("no_codec", dict(codec=NOCODEC)), ("low4", dict(codec=RC4)), ("null_items", dict(items=None)), ("items_on", dict(items_on=7))]
    back = [("cdfnum", dict(codec=ANS4S, cdfnum=0)), ("null_item", dict(items=NULL_PTR))]
    yield "trc_encode_planes_batch_host", BHOST, front + PLAN + [("filter", dict(filters=F_BAD))] + back
    yield "trc_encode_aplanes_batch_host", BHOST, front + PLAN + back
    yield "trc_encode_splanes_batch_host", BHOST, [("no_strides", dict(strides=None))] + front + PLAN + [("filter", dict(filters=F_BAD)), ("stride", dict(strides=S_BAD)),
                                                                                                       ("unstrided", dict(strides=S_ONE))] + back
    one, two = {"items": [[16 * A, 2]]}, {"items": [[16 * A, 4]]}
    for fn, b in (("trc_decode_planes_batch_host", trcb()), ("trc_decode_splanes_batch_host", trct())):
        d = dict(inlen=len(b), items=one, count=1, first_item=0, item_count=1, items_on=1)
        d["in"] = hexbuf(b)
        yield fn, d, [("no_items", dict(items=None)), ("items_on", dict(items_on=7)), ("check", dict(inlen=20)), ("count", dict(count=2)), ("item_size", dict(items=two)),
                      ("range", dict(first_item=1)), ("null_item", dict(items={"items": [[None, 2]]}))]
    yield "trc_decode_splanes_batch_host", dict(d, **{"in": hexbuf(trct(stride=2))}), [("stride_without_filter", dict())]


def groups():
    for kind in ("planes", "fplanes", "splanes", "bplanes"):
        yield from flat(kind)
    for kind in ("", "f", "s", "b"):
        yield from batch_split_join(kind)
    for kind in ("", "f", "s", "b"):
        yield from batch_coded(kind)
    for g in (packs, work_bytes, checks, host_encoders, host_decoders, batch_host):
        yield from g()


def case_groups(lib):
    """every group as dict(fn, valid = the valid call's arguments, cases = [(label, {parameter: value}), ..] for the single defects,
    pairs = [(label, label), ..] for the neighbouring ones that combine), without their results"""
    for fn, valid, defects in groups():
        names = params(SIGNATURES, fn)
        kept = [x for x in defects if x is None or all(k in names for k in x[1])]
        pairs = [(a[0], b[0]) for a, b in zip(kept, kept[1:]) if a and b and a[1] and b[1] and not set(a[1]) & set(b[1])]
        if fn.endswith("work_bytes"):
            pairs = []                              # (every answer is 0: a pair tells nothing)
        cases = []
        for label, change in [x for x in kept if x]:
            v = dict(valid, **change)
            for k, x in change.items():             # ("work", fn): the workspace the named work-bytes function states for this call
                if isinstance(x, tuple):
                    v[k] = run_case(lib, x[1], [v[n] for n in params(SIGNATURES, x[1])], SIGNATURES)[0]
            cases.append((label, {k: v[k] for k in change}))
        assert len({label for label, _ in cases}) == len(cases), "%s: a name twice in one group" % fn
        yield dict(fn=fn, valid=[valid[n] for n in names], cases=cases, pairs=pairs)


def pair_change(group, a, b):
    """what the pair of the group's cases a and b sets: both cases' parameters"""
    changes = {c[0]: c[1] for c in group["cases"]}
    return dict(changes[a], **changes[b])


def case_args(group, change, sigs, values):
    """the arguments of one case: the group's valid call with the case's parameters set; "$k" stands for values["$k"], and
    {"like": ["$k", offset, hex, ..]} for the buffer values["$k"] with those bytes at those offsets"""
    def whole(v):
        if isinstance(v, str):
            return values[v]
        if isinstance(v, dict) and "like" in v:
            b = bytearray.fromhex(values[v["like"][0]]["hex"])
            for off, h in zip(v["like"][1::2], v["like"][2::2]):
                b[off:off + len(h) // 2] = bytes.fromhex(h)
            return {"hex": b.hex()}
        return v
    names = params(sigs, group["fn"])
    return [whole(change.get(n, a)) for n, a in zip(names, group["valid"])]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "turbo-range-coder_amd", "libturborc_hip.so")
    lib = C.CDLL(path)
    lib.trc_planes_check.restype = C.c_int
    lib.trc_planes_batch_check.restype = C.c_int
    lib.trc_planes_sbatch_check.restype = C.c_int
    for mk, chk, extra in ((trcp, lib.trc_planes_check, 2), (trcf, lib.trc_fplanes_check, 2), (trcs, lib.trc_splanes_check, 2), (trcd, lib.trc_bplanes_check, 2),
                           (trcb, lib.trc_planes_batch_check, 1), (trct, lib.trc_planes_sbatch_check, 1)):
        b = mk()
        assert chk(b, C.c_size_t(len(b)), C.c_size_t(extra)) == 0, "the hand-built %s is not valid: %s" % (mk.__name__, lib.trc_last_error().decode())
    out, wrong, count = [], [], 0

    def run(g, label, change):
        fn = g["fn"]
        rc, text = run_case(lib, fn, case_args(g, change, SIGNATURES, {}), SIGNATURES)
        if fn.endswith("work_bytes"):
            ok = text is None                                   # these answer 0 or the size and say nothing
        elif SIGNATURES[fn][0] == "int":
            ok = rc in (E_ARG, E_WORK, E_CDF) and text
        else:
            ok = rc == 0 and text and "no HIP device" not in text and "hip" not in text
        if not ok:
            wrong.append("%s/%s: returned %d (%s): not a refusal before the device" % (fn, label, rc, text))
        return [rc, text]
    for g in case_groups(lib):
        done = [[label, change] + run(g, label, change) for label, change in g["cases"]]
        result = {c[0]: c[2:] for c in done}
        pairs = {}
        for a, b in g["pairs"]:                     # the label of the case whose refusal the pair's is, or [return value, text] where it is neither's
            r = run(g, a + "+" + b, pair_change(g, a, b))
            pairs[a + "+" + b] = a if r == result[a] else b if r == result[b] else r
        out.append(dict(g, cases=done, pairs=pairs))
        count += len(done) + len(pairs)
    assert not wrong, "\n".join(wrong)
    # an array or a buffer that occurs more than twice stands once, under "values", and "$k" in its places
    seen = {}
    for g in out:
        for v in g["valid"] + [x for c in g["cases"] for x in c[1].values()]:
            if isinstance(v, dict):
                seen[json.dumps(v)] = seen.get(json.dumps(v), 0) + 1
    for g in out:                                   # ... and so does a text that occurs more than twice
        for c in g["cases"]:
            if c[3]:
                seen[json.dumps(c[3])] = seen.get(json.dumps(c[3]), 0) + 1
    names = {k: "$%d" % i for i, k in enumerate(k for k, n in seen.items() if n > 2)}

    bufs = [(n, bytes.fromhex(json.loads(k)["hex"])) for k, n in names.items() if k[0] == "{" and "hex" in json.loads(k)]

    def short(v):
        if not isinstance(v, dict) or json.dumps(v) in names:
            return names.get(json.dumps(v), v) if isinstance(v, dict) else v
        if "hex" in v:                              # a buffer that differs from a shared one in a few bytes: those bytes
            b = bytes.fromhex(v["hex"])
            for n, ref in bufs:
                runs, i = [], 0
                while len(ref) == len(b) and i < len(b):
                    j = i
                    while j < len(b) and b[j] != ref[j]:
                        j += 1
                    if j > i:
                        runs += [i, b[i:j].hex()]
                    i = j + 1
                if runs and len(runs) <= 8:
                    return {"like": [n] + runs}
        return v
    with open(OUT, "w") as f:
        f.write('{"signatures": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in SIGNATURES.items()) + '},\n')
        f.write('"values": {\n' + ",\n".join("%s: %s" % (json.dumps(n), k) for k, n in names.items()) + '},\n"groups": [\n')
        f.write(",\n".join('{"fn": %s, "valid": %s, "cases": [\n%s],\n"pairs": %s}' % (
            json.dumps(g["fn"]), json.dumps([short(v) for v in g["valid"]]),
            ",\n".join(json.dumps([c[0], {k: short(v) for k, v in c[1].items()}, c[2], names.get(json.dumps(c[3]), c[3])]) for c in g["cases"]), json.dumps(g["pairs"])) for g in out) + "\n]}\n")
    print("%d cases of %d entry points -> %s" % (count, len({g["fn"] for g in out}), OUT))


if __name__ == "__main__":
    main()
