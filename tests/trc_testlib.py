"""Shared helpers for the parity tests (TEST INFRASTRUCTURE).

* deterministic synthetic inputs (own splitmix64 stream, so the GPU box regenerates the same bytes)
* ctypes bindings for the CPU oracle (oracle/libtrc_oracle.so) and, when it was built in the
  development container, the compiled reference (oracle/_ref/libtrc_ref.so)
* `ref_*` wrappers that respect the reference's calling quirks: `out` is placed at a
  HIGHER address than `in` with slack below it, and a decoder is never called on a raw stream.
* RefCalls: the same calls for a coder family's (in, n, out[, ...]) functions, which the <family>_lib modules build on
* product_lib(): the product library through trc.lib(), the one place that declares its prototypes
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "libtrc_oracle.so")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libtrc_ref.so")

# codec ids == include/trc_hip.h == oracle/trc_oracle.h
ANS4S, RCS1, RCS2, RCA, ANSA, RCB, RCAI, RCA4, RCAI4, ANSA4, RCSM, ANSO1, ANSB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
VLCU16, VLCU32, VLCV16, VLCV32, VLCVZ16, VLCVZ32 = 14, 15, 16, 17, 18, 19   # Turbo-VLC integer coders
VLAU16, VLAUZ16, VLAV16, VLAVZ16, VLAV32, VLAVZ32 = 20, 21, 22, 23, 24, 25   # ... over the CDF rANS
RCV8, RCVI8 = 26, 27                                                          # "vnibble" coders (rccdfenc8 / rccdfienc8, ids 48/49)
CODEC_NAMES = {ANS4S: "anscdf4s", RCS1: "rccdfs", RCS2: "rccdfs2", RCA: "rccdf", ANSA: "anscdf", RCB: "rcs", RCAI: "rccdfi",
               RCA4: "rccdf4", RCAI4: "rccdf4i", ANSA4: "anscdf4", RCSM: "rccdfsm", ANSO1: "anscdf1", ANSB: "ansb",
               VLCU16: "rccdfu16", VLCU32: "rccdfu32", VLCV16: "rccdfv16", VLCV32: "rccdfv32", VLCVZ16: "rccdfvz16", VLCVZ32: "rccdfvz32",
               VLAU16: "anscdfu16", VLAUZ16: "anscdfuz16", VLAV16: "anscdfv16", VLAVZ16: "anscdfvz16", VLAV32: "anscdfv32", VLAVZ32: "anscdfvz32",
               RCV8: "rccdf8", RCVI8: "rccdfi8"}
VLA_CODECS = (VLAU16, VLAUZ16, VLAV16, VLAVZ16, VLAV32, VLAVZ32)
VLC_CODECS = (VLCU16, VLCU32, VLCV16, VLCV32, VLCVZ16, VLCVZ32) + VLA_CODECS
VLC_ELEM = {VLCU16: 2, VLCU32: 4, VLCV16: 2, VLCV32: 4, VLCVZ16: 2, VLCVZ32: 4,
            VLAU16: 2, VLAUZ16: 2, VLAV16: 2, VLAVZ16: 2, VLAV32: 4, VLAVZ32: 4}   # element bytes
NIBBLE_CODECS = (RCA4, RCAI4, ANSA4)          # `turborc -n` coders: input values 0..15
# adaptive coders: (oracle encoder, oracle decoder, reference encoder, reference decoder); ANS ones take a variant suffix
_ADAPTIVE = {RCA: ("rccdfenc", "rccdfdec"), ANSA: ("anscdfenc", "anscdfdec"), RCB: ("rcsenc", "rcsdec"),
             RCAI: ("rccdfienc", "rccdfidec"), RCA4: ("rccdf4enc", "rccdf4dec"), RCAI4: ("rccdf4ienc", "rccdf4idec"),
             ANSA4: ("anscdf4enc", "anscdf4dec"), ANSO1: ("anscdf1enc", "anscdf1dec"), ANSB: ("ansbc", "ansbd"),
             VLCU16: ("rccdfuenc16", "rccdfudec16"), VLCU32: ("rccdfuenc32", "rccdfudec32"),
             VLCV16: ("rccdfvenc16", "rccdfvdec16"), VLCV32: ("rccdfvenc32", "rccdfvdec32"),
             VLCVZ16: ("rccdfvzenc16", "rccdfvzdec16"), VLCVZ32: ("rccdfvzenc32", "rccdfvzdec32"),
             VLAU16: ("anscdfuenc16", "anscdfudec16"), VLAUZ16: ("anscdfuzenc16", "anscdfuzdec16"),
             VLAV16: ("anscdfvenc16", "anscdfvdec16"), VLAVZ16: ("anscdfvzenc16", "anscdfvzdec16"),
             VLAV32: ("anscdfvenc32", "anscdfvdec32"), VLAVZ32: ("anscdfvzenc32", "anscdfvzdec32"),
             RCV8: ("rccdfenc8", "rccdfdec8"), RCVI8: ("rccdfienc8", "rccdfidec8")}
STATIC_CODECS = (ANS4S, RCS1, RCS2, RCSM)

_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)


# ------------------------------------------------------------------------------- inputs ---------
def splitmix64(n, seed):
    """n 64-bit words of the splitmix64 stream started at `seed` (vectorised)."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform_bytes(n, seed=1):
    w = splitmix64((n + 7) // 8, seed)
    return w.view(np.uint8)[:n].copy()


def table_bytes(n, weights, seed=1):
    """i.i.d. bytes drawn from `weights` (len <= 256) by inverse-CDF on the splitmix64 stream."""
    w = np.asarray(weights, dtype=np.float64)
    cum = np.cumsum(w / w.sum())
    cum[-1] = 1.0
    u = (splitmix64(n, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    return np.searchsorted(cum, u, side="right").astype(np.uint8)


def splitmix64_range(start, count, seed):
    """words start .. start+count-1 (0-based) of the same stream: any slice of a big input can be regenerated alone"""
    with np.errstate(over="ignore"):
        z = (np.arange(start + 1, start + count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _cum(weights):
    w = np.asarray(weights, dtype=np.float64)
    cum = np.cumsum(w / w.sum())
    cum[-1] = 1.0
    return cum


def table_bytes_range(start, count, weights, seed=1):
    """bytes start .. start+count-1 of table_bytes(n, weights, seed), for any n >= start+count"""
    u = (splitmix64_range(start, count, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    return np.searchsorted(_cum(weights), u, side="right").astype(np.uint8)


def table_bytes_device(torch, dev, n, weights, seed=1, out=None, slab=1 << 26):
    """table_bytes generated ON THE DEVICE (1 GB per GPU never crosses PCIe): the same splitmix64
    stream in wrapping int64 arithmetic, the same double-precision inverse-CDF lookup -> byte-identical to the numpy
    generator (tests compare slices).  Returns a uint8 tensor of n (+ pad if `out` is given) bytes."""
    def s64(x):                                                 # unsigned 64-bit constant as the signed value torch takes
        return x - (1 << 64) if x >= (1 << 63) else x
    cum = torch.from_numpy(_cum(weights)).to(dev)
    res = out if out is not None else torch.empty(n, dtype=torch.uint8, device=dev)
    G, M1, M2 = s64(0x9E3779B97F4A7C15), s64(0xBF58476D1CE4E5B9), s64(0x94D049BB133111EB)
    for o in range(0, n, slab):
        c = min(slab, n - o)
        z = torch.arange(o + 1, o + c + 1, dtype=torch.int64, device=dev) * G + s64(seed & ((1 << 64) - 1))
        z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * M1            # logical shifts: mask off the sign extension
        z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * M2
        z = z ^ ((z >> 31) & ((1 << 33) - 1))
        u = ((z >> 11) & ((1 << 53) - 1)).to(torch.float64) * (1.0 / (1 << 53))
        res[o:o + c] = torch.searchsorted(cum, u, right=True).to(torch.uint8)
    return res


def zipf_weights(alpha=1.1, nsym=256):
    return 1.0 / np.arange(1, nsym + 1) ** alpha


def mix_bytes(n, seed=13):
    """heterogeneous workload ("mix100m"): stretches of 1..64 KiB, each one of text / uniform (incompressible) / runs /
    constant, so that chunks of one wave differ in compressibility (lane imbalance) and raw chunks sit among coded
    ones.  Deterministic."""
    out = np.empty(n, dtype=np.uint8)
    text, uni, runs = text_bytes(n, seed), uniform_bytes(n, seed + 1), runs_bytes(n, seed + 2)
    ctl = splitmix64(n // 1024 + 8, seed + 3)
    pos = i = 0
    while pos < n:
        ln = min(n - pos, (int(ctl[i] >> np.uint64(8)) % 64 + 1) * 1024)
        kind = int(ctl[i] & np.uint64(7))
        src = text if kind < 3 else uni if kind < 5 else runs if kind < 7 else None
        out[pos:pos + ln] = src[pos:pos + ln] if src is not None else int(ctl[i] >> np.uint64(40)) & 255
        pos += ln; i += 1
    return out


def zipf_bytes(n, alpha=1.1, nsym=256, seed=1):
    return table_bytes(n, 1.0 / np.arange(1, nsym + 1) ** alpha, seed)


def text_bytes(n, seed=7):
    """'enwik8 stand-in' (SURVEY 8d cfg 2): i.i.d. bytes, English-like order-0 table, ~5.1 bit/B."""
    return table_bytes(n, text_weights(), seed)


def text_weights():
    w = np.full(256, 2e-5)
    common = b" etaoinshrdlcumwfgypbvkjxqz"
    freq = [17.0, 9.6, 7.0, 6.2, 5.9, 5.5, 5.3, 5.0, 4.5, 4.4, 3.3, 3.1, 2.4, 2.2, 2.1, 1.9, 1.8, 1.6, 1.5, 1.3,
            1.2, 0.8, 0.6, 0.15, 0.13, 0.1, 0.07]
    for ch, f in zip(common, freq):
        w[ch] = f
    for ch in range(ord("A"), ord("Z") + 1):
        w[ch] = 0.18
    for ch in b"0123456789":
        w[ch] = 0.45
    for ch, f in zip(b"[]|=<>/&;:.,'\"\n-()", [1.2, 1.2, 0.7, 0.6, 0.9, 0.9, 0.6, 0.5, 0.5, 0.4, 0.9, 1.0, 0.5, 0.5, 1.3, 0.4, 0.2, 0.2]):
        w[ch] = f
    return w


def runs_bytes(n, seed=3, mean_run=6.0, alpha=1.2):
    """'enwik8bwt stand-in' (SURVEY 8d cfg 3): geometric runs over a Zipf alphabet."""
    nr = int(n / mean_run * 1.3) + 16
    sym = zipf_bytes(nr, alpha, 256, seed)
    u = (splitmix64(nr, seed + 99) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    rl = (np.floor(np.log1p(-u) / np.log1p(-1.0 / mean_run)) + 1).astype(np.int64)
    out = np.repeat(sym, rl)
    while out.size < n:
        out = np.concatenate([out, out])
    return out[:n].copy()


def drift_bytes(n, seed=3, mean_seg=768.0, kmax=8, decay=0.6, alpha=1.3):
    """'enwik8bwt stand-in' with statistics that DRIFT (round 4; SURVEY 8d cfg 3 asks for ~25 % adaptive ratio,
    README.md:88,92: 24.81 % / 24.85 %): piecewise stationary like a BWT output -- segments of geometric length (mean
    `mean_seg`), in each of them 2..kmax symbols drawn from a Zipf(alpha) alphabet with geometrically decaying
    probabilities (the first one dominates, runs come by themselves).  Whole-buffer reference ratios at 10 MB:
    rccdfenc 26.7 %, rcsenc 25.6 %, static anscdf4senc 60.0 % -- an order-0 ADAPTIVE model gains a factor two over
    a static one here (on `runs_bytes`, whose symbols are stationary, it gains nothing: 59.7 % vs 66 %)."""
    nseg = int(n / mean_seg * 1.25) + 16
    u = (splitmix64(nseg, seed + 101) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    sl = (np.floor(np.log1p(-u) / np.log1p(-1.0 / mean_seg)) + 1).astype(np.int64)
    while sl.sum() < n:
        sl = np.concatenate([sl, sl])
    cs = np.cumsum(sl)
    nseg = int(np.searchsorted(cs, n) + 1)
    sl = sl[:nseg]; cs = cs[:nseg]
    k = (splitmix64(nseg, seed + 102) % np.uint64(kmax - 1)).astype(np.int64) + 2                  # symbols in use: 2..kmax
    syms = np.stack([table_bytes(nseg, zipf_weights(alpha, 256), seed + 110 + j) for j in range(kmax)], axis=1)
    # (round 5: the bytes themselves in blocks -- every byte depends on its own index and its segment only, and 1 GB of the
    # whole-array form needs ~50 GB of temporaries; the output is the same)
    out = np.empty(n, dtype=np.uint8)
    BLK = 32 * 1000 * 1000
    for lo in range(0, n, BLK):
        cnt = min(BLK, n - lo)
        seg = np.searchsorted(cs, np.arange(lo, lo + cnt, dtype=np.int64), side="right")
        v = (splitmix64_range(lo, cnt, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
        # rank j with probability (1 - decay) * decay^j, the tail mass on the segment's last symbol
        j = np.minimum(np.floor(np.log(np.maximum(1.0 - v, 1e-300)) / np.log(decay)).astype(np.int64), k[seg] - 1)
        out[lo:lo + cnt] = syms[seg, j]
    return out


def nibble_bytes(n, seed=5, kind="geo"):
    """`turborc -n` style input: values 0..15.  geo: skewed (geometric); runs: run-heavy; uniform: incompressible-ish."""
    u = (splitmix64(n, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    if kind == "uniform":
        return (u * 16).astype(np.uint8)
    v = np.minimum(np.floor(np.log1p(-u) / np.log(0.62)), 15).astype(np.uint8)
    if kind == "runs":
        rl = (splitmix64(n, seed + 7) % np.uint64(9)).astype(np.int64) + 1
        v = np.repeat(v[:n // 4 + 4], rl[:n // 4 + 4])
        while v.size < n:
            v = np.concatenate([v, v])
    return v[:n].copy()


def small_bytes(n, seed=15, kind="geo"):
    """bytes that are mostly small values -- what the vnibble coders (`turborc -e48/-e49`) are for.
    geo: geometric from 0; mid: geometric from 13 (the two-symbol range)"""
    u = (splitmix64(n, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    if kind == "mid":
        return (13 + np.minimum(np.floor(np.log1p(-u) / np.log(0.9)), 200)).astype(np.uint8)
    return np.minimum(np.floor(np.log1p(-u) / np.log(0.85)), 255).astype(np.uint8)


def int_bytes(n, es, kind="walk", seed=9):
    """16/32-bit integer series as bytes (n a multiple of es) for the Turbo-VLC coders.
    small: mostly tiny values; walk: slow random walk around mid-range (what the zigzag-delta coders are for);
    mixed: tiny values with rare large ones; wide: uniform over the whole range (incompressible)."""
    ne = n // es
    u = splitmix64(ne, seed)
    f = (u >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    top = 1 << (8 * es)
    if kind == "small":
        v = np.minimum(np.floor(np.log1p(-f) / np.log(0.8)), 60000).astype(np.uint64)
    elif kind == "walk":
        v = (np.cumsum((u % np.uint64(61)).astype(np.int64) - 30) + (top >> 2)).astype(np.uint64)
    elif kind == "mixed":
        big = (splitmix64(ne, seed + 1) % np.uint64(top >> 1))
        v = np.where(f < 0.9, u % np.uint64(20), big).astype(np.uint64)
    else:
        v = u % np.uint64(top)
    return (v % np.uint64(top)).astype(np.uint16 if es == 2 else np.uint32).view(np.uint8).copy()


def fnv1a64(b):
    """FNV-1a-64 of a bytes-like (for large-case fixtures)."""
    h = 0xCBF29CE484222325
    for x in bytes(b):
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------------------- oracle ---------
def build_oracle():
    if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(os.path.join(ORACLE_DIR, "trc_oracle.c")):
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "libtrc_oracle.so"])
    return ORACLE_SO


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(build_oracle())
        sz = C.c_size_t
        lib.orc_cdfini.restype = C.c_int
        lib.orc_cdfini.argtypes = [_u8p, sz, _u16p, C.c_uint]
        for name in ("orc_rccdfsenc", "orc_rccdfsdec", "orc_rccdfs2enc", "orc_rccdfs2dec", "orc_rccdfsmenc", "orc_rccdfsmdec"):
            f = getattr(lib, name); f.restype = sz; f.argtypes = [_u8p, sz, _u8p, _u16p, C.c_uint]
        lib.orc_anscdf4senc.restype = sz; lib.orc_anscdf4senc.argtypes = [_u8p, sz, _u8p, _u16p]
        lib.orc_anscdf4sdec.restype = sz; lib.orc_anscdf4sdec.argtypes = [_u8p, sz, _u8p, _u16p, C.c_uint]
        for pair in _ADAPTIVE.values():
            for name in pair:
                f = getattr(lib, "orc_" + name); f.restype = sz; f.argtypes = [_u8p, sz, _u8p]
        lib.orc_chunked_enc.restype = sz
        lib.orc_chunked_enc.argtypes = [C.c_int, _u8p, sz, sz, _u16p, C.c_uint, _u8p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        lib.orc_chunked_dec.restype = sz
        lib.orc_chunked_dec.argtypes = [C.c_int, _u8p, C.POINTER(C.c_uint32), sz, sz, _u16p, C.c_uint, _u8p]
        _oracle = lib
    return _oracle


def _p8(a):
    return a.ctypes.data_as(_u8p)


def _p16(a):
    return a.ctypes.data_as(_u16p)


def orc_cdfini(data, cdfnum=None):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if cdfnum is None:
        cdfnum = int(data.max()) + 1
    cdf = np.zeros(257, dtype=np.uint16)
    r = oracle().orc_cdfini(_p8(data), data.size, _p16(cdf), cdfnum)
    return r, cdf, cdfnum


def orc_enc(codec, data, cdf=None, cdfnum=256):
    """Whole-buffer oracle encode -> bytes (np.uint8 array of the returned length)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    out = np.zeros(n + 64, dtype=np.uint8)
    o = oracle()
    if codec == ANS4S:
        l = o.orc_anscdf4senc(_p8(data), n, _p8(out), _p16(cdf))
    elif codec == RCS1:
        l = o.orc_rccdfsenc(_p8(data), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCS2:
        l = o.orc_rccdfs2enc(_p8(data), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCSM:
        l = o.orc_rccdfsmenc(_p8(data), n, _p8(out), _p16(cdf), cdfnum)
    elif codec in _ADAPTIVE:
        l = getattr(o, "orc_" + _ADAPTIVE[codec][0])(_p8(data), n, _p8(out))
    else:
        raise ValueError(codec)
    return out[:l].copy()


def orc_dec(codec, comp, n, cdf=None, cdfnum=256):
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    if comp.size == n:
        return comp.copy()                      # stored raw (CCPY rule, turborc.c:434)
    src = np.zeros(comp.size + 64, dtype=np.uint8)
    src[:comp.size] = comp
    out = np.zeros(n + 8, dtype=np.uint8)
    o = oracle()
    if codec == ANS4S:
        o.orc_anscdf4sdec(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCS1:
        o.orc_rccdfsdec(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCS2:
        o.orc_rccdfs2dec(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCSM:
        o.orc_rccdfsmdec(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec in _ADAPTIVE:
        getattr(o, "orc_" + _ADAPTIVE[codec][1])(_p8(src), n, _p8(out))
    else:
        raise ValueError(codec)
    return out[:n].copy()


def orc_chunked_enc(codec, data, chunk, cdf=None, cdfnum=256):
    """-> (payload bytes, clen[nchunks] u32, poff[nchunks+1] u64): chunk c's payload = coder(chunk c)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    nch = (n + chunk - 1) // chunk
    payload = np.zeros(n + 64, dtype=np.uint8)
    clen = np.zeros(max(nch, 1), dtype=np.uint32)
    poff = np.zeros(nch + 1, dtype=np.uint64)
    cdfp = _p16(cdf) if cdf is not None else None
    tot = oracle().orc_chunked_enc(codec, _p8(data), n, chunk, cdfp, cdfnum, _p8(payload),
                                   clen.ctypes.data_as(C.POINTER(C.c_uint32)), poff.ctypes.data_as(C.POINTER(C.c_uint64)))
    return payload[:tot].copy(), clen[:nch].copy(), poff


def orc_chunked_enc_mt(codec, data, chunk, cdf=None, cdfnum=256, threads=None):
    """orc_chunked_enc over the host's cores: the chunk range is cut into one run per thread (ctypes releases the GIL),
    results concatenated -> (payload, clen).  For the BASELINE-size total-parity tests."""
    import concurrent.futures as cf
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    nch = (n + chunk - 1) // chunk
    threads = threads or min(64, os.cpu_count() or 1)
    per = max(1, (nch + threads - 1) // threads) * chunk
    parts = [data[o:o + per] for o in range(0, n, per)]
    with cf.ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(lambda x: orc_chunked_enc(codec, x, chunk, cdf, cdfnum)[:2], parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


# the exact (workload, coder, chunk) configurations bench.py reports on (BASELINE.json configs 2-4); the expected
# payload hashes are committed in tests/golden/bench_configs.json, generated THROUGH THE REFERENCE (oracle/_ref)
BENCH_CONFIGS = [
    dict(name="anscdf4s-text100m-512", codec=ANS4S, kind="text", seed=7, n=100 * 1000 * 1000, chunk=512),      # the headline
    dict(name="rccdfs2-text100m-896", codec=RCS2, kind="text", seed=7, n=100 * 1000 * 1000, chunk=896),        # `-e45` literal
    dict(name="rccdf-bwt100m-512", codec=RCA, kind="bwt", seed=3, n=100 * 1000 * 1000, chunk=512),             # config 3, `-e46`
    dict(name="anscdf-bwt100m-512", codec=ANSA, kind="bwt", seed=3, n=100 * 1000 * 1000, chunk=512),           # config 3, `-e56`
    dict(name="rcs-text100m-512", codec=RCB, kind="text", seed=7, n=100 * 1000 * 1000, chunk=512),             # config 4, `-e1`
    dict(name="anscdf4s-text100m-4096", codec=ANS4S, kind="text", seed=7, n=100 * 1000 * 1000, chunk=4096),    # the chunk size of the large-input regime
    # the chunks bench.py runs these coders at since round 3 (one residency round of their waves at 100 MB)
    dict(name="rccdfs2-text100m-1024", codec=RCS2, kind="text", seed=7, n=100 * 1000 * 1000, chunk=1024),
    dict(name="rccdf-bwt100m-1536", codec=RCA, kind="bwt", seed=3, n=100 * 1000 * 1000, chunk=1536),
    dict(name="anscdf-bwt100m-1536", codec=ANSA, kind="bwt", seed=3, n=100 * 1000 * 1000, chunk=1536),
    dict(name="rcs-text100m-1536", codec=RCB, kind="text", seed=7, n=100 * 1000 * 1000, chunk=1536),
    # round 4: config 3 on data whose statistics DRIFT (drift_bytes: piecewise stationary, whole-buffer rccdfenc ~27 %) -- what
    # bench.py runs the adaptive coders on since then; the `bwt` entries above (stationary runs) stay as parity cases
    dict(name="rccdf-drift100m-1536", codec=RCA, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=1536),
    dict(name="anscdf-drift100m-1536", codec=ANSA, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=1536),
    dict(name="rccdf-drift100m-4096", codec=RCA, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=4096),
    dict(name="anscdf-drift100m-4096", codec=ANSA, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=4096),
    # round 5: 1 GB inputs (`bench.py --codec X --size 1000000000`), where trc_round_chunk now lets the chunk grow to one residency
    # round (~15 KiB): only the size ONE whole-buffer call of the reference returns is recorded (chunk None: no per-chunk hashes)
    dict(name="rccdf-drift1g-whole", codec=RCA, kind="drift", seed=3, n=1000 * 1000 * 1000, chunk=None),
    dict(name="anscdf-drift1g-whole", codec=ANSA, kind="drift", seed=3, n=1000 * 1000 * 1000, chunk=None),
    dict(name="rcs-text1g-whole", codec=RCB, kind="text", seed=7, n=1000 * 1000 * 1000, chunk=None),
    # the coders `bench.py --codec X` reports on without a committed hash so far, at the chunk trc_round_chunk gives them
    dict(name="rccdfi-drift100m-1536", codec=RCAI, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=1536),
    dict(name="anscdf1-drift100m-4096", codec=ANSO1, kind="drift", seed=3, n=100 * 1000 * 1000, chunk=4096),
    dict(name="ansb-text100m-1536", codec=ANSB, kind="text", seed=7, n=100 * 1000 * 1000, chunk=1536),
    dict(name="rccdfs-text100m-512", codec=RCS1, kind="text", seed=7, n=100 * 1000 * 1000, chunk=512),
    dict(name="rccdfsm-text100m-512", codec=RCSM, kind="text", seed=7, n=100 * 1000 * 1000, chunk=512),
]


def bench_input(kind, n, seed):
    return runs_bytes(n, seed) if kind == "bwt" else drift_bytes(n, seed) if kind == "drift" else text_bytes(n, seed)


def orc_chunked_dec(codec, payload, clen, n, chunk, cdf=None, cdfnum=256):
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    clen = np.ascontiguousarray(clen, dtype=np.uint32)
    out = np.zeros(n + 8, dtype=np.uint8)
    cdfp = _p16(cdf) if cdf is not None else None
    src = np.zeros(payload.size + 64, dtype=np.uint8); src[:payload.size] = payload
    oracle().orc_chunked_dec(codec, _p8(src), clen.ctypes.data_as(C.POINTER(C.c_uint32)), n, chunk, cdfp, cdfnum, _p8(out))
    return out[:n].copy()


# ------------------------------------------------------------------------------- reference ------
_ref = None


def have_ref():
    return os.path.exists(REF_SO)


def ref():
    global _ref
    if _ref is None:
        lib = C.CDLL(REF_SO)
        sz = C.c_size_t
        lib.cdfini.restype = C.c_int; lib.cdfini.argtypes = [_u8p, sz, _u16p, C.c_uint]
        for name in ("rccdfsenc", "rccdfsbdec", "rccdfsldec", "rccdfsvbdec", "rccdfsvldec", "rccdfs2enc", "rccdfsb2dec",
                     "rccdfsmenc", "rccdfsmbdec", "rccdfsmldec"):
            f = getattr(lib, name); f.restype = sz; f.argtypes = [_u8p, sz, _u8p, _u16p, C.c_uint]
        for name in ("anscdf4senc", "anscdf4sencs", "anscdf4sencx"):
            f = getattr(lib, name); f.restype = sz; f.argtypes = [_u8p, sz, _u8p, _u16p]
        names = [n for pair in _ADAPTIVE.values() for n in pair]
        names += [n + v for n in ("anscdfenc", "anscdfdec", "anscdf4enc", "anscdf4dec", "anscdf1enc", "anscdf1dec") for v in ("s", "x")]
        names += [n + v for c in VLA_CODECS for n in _ADAPTIVE[c] for v in ("s", "x")]
        for name in names:
            f = getattr(lib, name); f.restype = sz; f.argtypes = [_u8p, sz, _u8p]
        _ref = lib
    return _ref


def _arena(n):
    """One allocation with `in` low and `out` high and 2n+64 bytes of slack between
    them (anscdf4senc writes downward from out+n and may under-run `out` on expanding data)."""
    gap = 2 * n + 64
    buf = np.zeros(n + gap + n + n // 2 + 1024, dtype=np.uint8)
    return buf, 0, n + gap


class RefCalls:
    """The reference calls of one coder family: ref_fn maps a codec to its (encoder, decoder) names in the shared object `so`,
    every one a (u8 *in, size_t n, u8 *out) function followed by arguments of the types in `extra`; the calls take those
    arguments' values behind their own.  The shared object is opened at the first call.
    guard: the encoder's arena is filled with 0xA5, and that many bytes in front of `out` and behind what the encoder returns
    must still hold it (0: the arena stays zero, nothing is asserted).
    chunk_hook(codec, piece, *extra) -> the payload of one chunk, where chunked_enc is not to call enc on every piece."""

    def __init__(self, ref_fn, so, extra=(), guard=0, chunk_hook=None):
        self.ref_fn, self.so, self.extra, self.guard, self.chunk_hook = ref_fn, so, list(extra), guard, chunk_hook
        self._lib = None

    def have(self):
        return os.path.exists(self.so)

    def _fn(self, name):
        if self._lib is None:
            lib = C.CDLL(self.so)
            for pair in self.ref_fn.values():
                for f in (getattr(lib, n) for n in pair):
                    f.restype = C.c_size_t
                    f.argtypes = [_u8p, C.c_size_t, _u8p] + self.extra
            self._lib = lib
        return getattr(self._lib, name)

    def enc(self, codec, data, *extra):
        """one call of the reference encoder on `data`, `in` below `out` in one arena (_arena)"""
        name = self.ref_fn[codec][0]
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = data.size
        buf, io, oo = _arena(n)
        if self.guard:
            buf[:] = 0xA5
        buf[io:io + n] = data
        base = buf.ctypes.data
        l = self._fn(name)(C.cast(base + io, _u8p), n, C.cast(base + oo, _u8p), *extra)
        if self.guard:
            assert (buf[oo - self.guard:oo] == 0xA5).all() and (buf[oo + l:oo + l + self.guard] == 0xA5).all(), (name, n)
        return buf[oo:oo + l].copy()

    def chunked_enc(self, codec, data, chunk, *extra):
        """-> (clen u32 array, payload u8 array): the reference called once per chunk"""
        one = self.chunk_hook or self.enc
        outs = [one(codec, data[i:i + chunk], *extra) for i in range(0, data.size, chunk)]
        clen = np.array([o.size for o in outs], dtype=np.uint32)
        payload = np.concatenate(outs) if outs else np.zeros(0, np.uint8)
        return clen, payload

    def dec(self, codec, comp, n, *extra):
        """the reference decoder on one coded chunk; a raw one (comp.size == n) is the output itself"""
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        if comp.size == n:
            return comp.copy()
        src = np.zeros(comp.size + 1024, dtype=np.uint8); src[:comp.size] = comp
        out = np.zeros(n + 64, dtype=np.uint8)
        self._fn(self.ref_fn[codec][1])(_p8(src), n, _p8(out), *extra)
        return out[:n].copy()


def product_lib():
    """trc.lib(), the product library with every prototype the tests call declared; built first where it is missing"""
    import trc
    if not os.path.exists(trc.LIB):
        import __graft_entry__ as g
        g.build()
    return trc.lib()


def ref_enc(codec, data, cdf=None, cdfnum=256, variant=""):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    buf, io, oo = _arena(n)
    buf[io:io + n] = data
    base = buf.ctypes.data
    pin = C.cast(base + io, _u8p); pout = C.cast(base + oo, _u8p)
    r = ref()
    if codec == ANS4S:
        l = getattr(r, "anscdf4senc" + variant)(pin, n, pout, _p16(cdf))
    elif codec == RCS1:
        l = r.rccdfsenc(pin, n, pout, _p16(cdf), cdfnum)
    elif codec == RCS2:
        l = r.rccdfs2enc(pin, n, pout, _p16(cdf), cdfnum)
    elif codec == RCSM:
        l = r.rccdfsmenc(pin, n, pout, _p16(cdf), cdfnum)
    elif codec in _ADAPTIVE:
        l = getattr(r, _ADAPTIVE[codec][0] + (variant if codec in (ANSA, ANSA4, ANSO1) + VLA_CODECS else ""))(pin, n, pout)
    else:
        raise ValueError(codec)
    return buf[oo:oo + l].copy()


def ref_dec(codec, comp, n, cdf=None, cdfnum=256, variant="", search="b"):
    """Reference decode; ANS4S has no byte-alphabet reference decoder -> None."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    if comp.size == n:
        return comp.copy()
    if codec == ANS4S:
        return None
    src = np.zeros(comp.size + 1024, dtype=np.uint8); src[:comp.size] = comp
    out = np.zeros(n + 64, dtype=np.uint8)
    r = ref()
    if codec == RCS1:
        getattr(r, "rccdfs%sdec" % search)(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCS2:
        r.rccdfsb2dec(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec == RCSM:
        getattr(r, "rccdfsm%sdec" % search)(_p8(src), n, _p8(out), _p16(cdf), cdfnum)
    elif codec in _ADAPTIVE:
        getattr(r, _ADAPTIVE[codec][1] + (variant if codec in (ANSA, ANSA4, ANSO1) + VLA_CODECS else ""))(_p8(src), n, _p8(out))
    return out[:n].copy()


def ref_cdfini(data, cdfnum=None):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if cdfnum is None:
        cdfnum = int(data.max()) + 1
    cdf = np.zeros(257, dtype=np.uint16)
    r = ref().cdfini(_p8(data), data.size, _p16(cdf), cdfnum)
    return r, cdf, cdfnum
