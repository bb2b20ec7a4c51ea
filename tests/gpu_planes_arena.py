"""The byte-plane calls of include/trc_hip.h in the audited arena of tests/gpu_arena.py: every buffer at its stated size and its
stated alignment and no better, a base and a batch item with NO slack (poison follows their last byte), planes at the smallest
pitch, workspaces, tables, histograms and containers of exactly the bytes their size functions name, everything poisoned (seeded
random bytes or 0xFF) before the inputs go in.  After every library call the whole allocation is audited against its image.
Expected values never come from the device: the numpy models (planes_lib, fplanes_lib, splanes_lib, oplanes_lib, bplanes_lib,
planes_batch_lib.virtual, advise_lib), per plane the oracle (trc_testlib.orc_cdfini / orc_chunked_enc: plane k's result is
trc_encode_dev on plane k), for containers the layout functions.  Stray READS leave no trace: a read past a no-slack buffer shows
only where it changes a result, which is why every run_* returns its outputs for gpu_arena.same_outputs under the two poisons.

A plain helper module (not collected).  Nothing here needs a device at import: tests/test_arena_cpu.py uses the layouts and the
inputs of section B."""
import ctypes as C

import numpy as np

import advise_lib as AL
import bplanes_lib as BPL
import fplanes_lib as FL
import gpu_arena as GA
import oplanes_lib as OL
import planes_batch_lib as BL
import planes_lib as PL
import planes_matrix_lib as PM
import splanes_lib as SL
import trc
import trc_testlib as T
from planes_batch_lib import up256

PAD = GA.PAD
SEG = 256                                                      # the restart length of the flat filtered kernels ...
SEG_PARTIAL = 576                                              # ... and one whose spans end in a partial tile of the scanning join
ESIZES = PL.ESIZES
CDF_STRIDE = trc.PLANES_CDF_STRIDE
# (kind, filter, stride); ("ofilter", order, stride): the predictor of that order, which has no filter argument
FLAT_FAMILIES = ([("plain", 0, 0)] + [("filter", f, 0) for f in FL.FILTERS] + [("sfilter", f, s) for f in FL.FILTERS for s in (1, 3, 8)]
                 + [("base", f, 0) for f in FL.FILTERS] + [("ofilter", k, s) for k, s in ((2, 1), (3, 3), (2, 6), (3, 8))])
SEG_KINDS = ("filter", "sfilter", "ofilter")                   # the kinds whose calls take a restart length


def flat_shapes(esize):
    """(m, t): one element; less than a vector with a full tail; one vector (all three: fewer elements than ORDER * S, where an order
    split reaches up to three vectors back); a partial vector behind 256 of them; more than one workgroup with a partial vector and
    a full tail"""
    return [(1, 0), (7, esize - 1), (8, 0), (8 * 256 + 9, 1), (2049 * 8 + 5, esize - 1)]


def fam_name(fam):
    kind, f, s = fam
    if kind == "ofilter":
        return "ofilter-o%d-s%d" % (f, s)
    return kind + ("-" + FL.FILTER_NAMES[f] if f else "") + ("-s%d" % s if s else "")


def forward(fam, d, base, esize, seg):
    """what the family's split sees in front of the planes: the model"""
    kind, f, s = fam
    if kind == "plain":
        return np.ascontiguousarray(d, dtype=np.uint8)
    if kind == "filter":
        return FL.forward(d, esize, f, seg)
    if kind == "sfilter":
        return SL.forward(d, esize, f, seg, s)
    if kind == "ofilter":
        return OL.forward(d, esize, f, seg, s)
    return BPL.forward(d, base, esize, f)


def inverse(fam, y, base, esize, seg):
    kind, f, s = fam
    if kind == "plain":
        return np.ascontiguousarray(y, dtype=np.uint8)
    if kind == "filter":
        return FL.inverse(y, esize, f, seg)
    if kind == "sfilter":
        return SL.inverse(y, esize, f, seg, s)
    if kind == "ofilter":
        return OL.inverse(y, esize, f, seg, s)
    return BPL.inverse(y, base, esize, f)


def flat_input(fam, esize, m, t):
    """-> (data of m elements and t tail bytes, base of m elements or None)"""
    kind, f, s = fam
    seed = 1000 * esize + m
    if kind == "base":
        return BPL.gen_pair(BPL.KINDS[(m + esize) % 4], esize, m, t, seed)
    if kind == "ofilter":
        return OL.gen(OL.KINDS[(m + esize) % 4], esize, m, t, seed, s), None
    if s > 1:
        return SL.gen("interleaved", esize, m, t, seed, s), None
    return FL.gen(FL.KINDS[(m + esize) % 4], esize, m, t, seed), None


def arena(torch, specs, poison, seed, alias=None, device="cuda:0"):
    return GA.Arena(torch, GA.Layout(specs, alias), device, poison, seed)


def ok(rc, tag):
    assert rc == 0, "%s returned %d: %s" % (tag, rc, trc.lib().trc_last_error().decode())


# ------------------------------------------------------------------------------------------------- A. the flat kernels ---
def flat_specs(fam, esize, m, t):
    n = m * esize + t
    specs = [("in", n), ("planes", esize * up256(m)), ("tail", 8), ("out", n)]
    if fam[0] == "base":
        specs += [("base", m * esize), ("io.base", n)]         # io.base: the base a join decodes onto, n bytes: the tail lands behind it
    return specs, ({"io.out": "io.base"} if fam[0] == "base" else None)


def split_flat(fam, A, n, esize, pitch, seg=SEG):
    L, (kind, f, s) = trc.lib(), fam
    i, p, tl = A.ptr("in"), A.ptr("planes"), A.ptr("tail")
    if kind == "plain":
        return L.trc_planes_split_dev(i, n, esize, p, pitch, tl, None)
    if kind == "filter":
        return L.trc_planes_split_filter_dev(f, i, n, esize, seg, p, pitch, tl, None)
    if kind == "sfilter":
        return L.trc_planes_split_sfilter_dev(f, s, i, n, esize, seg, p, pitch, tl, None)
    if kind == "ofilter":
        return L.trc_planes_split_ofilter_dev(f, s, i, n, esize, seg, p, pitch, tl, None)
    return L.trc_planes_split_base_dev(f, i, A.ptr("base"), n, esize, p, pitch, tl, None)


def join_flat(fam, A, n, esize, pitch, out="out", base="base", seg=SEG):
    L, (kind, f, s) = trc.lib(), fam
    p, tl, o = A.ptr("planes"), A.ptr("tail"), A.ptr(out)
    if kind == "plain":
        return L.trc_planes_join_dev(p, pitch, tl, n, esize, o, None)
    if kind == "filter":
        return L.trc_planes_join_filter_dev(f, p, pitch, tl, n, esize, seg, o, None)
    if kind == "sfilter":
        return L.trc_planes_join_sfilter_dev(f, s, p, pitch, tl, n, esize, seg, o, None)
    if kind == "ofilter":
        return L.trc_planes_join_ofilter_dev(f, s, p, pitch, tl, n, esize, seg, o, None)
    return L.trc_planes_join_base_dev(f, p, pitch, tl, A.ptr(base), n, esize, o, None)


def plane_writes(name, esize, pitch, m):
    return [(name, k * pitch, k * pitch + m) for k in range(esize)]


def run_flat(torch, fam, esize, m, t, poison, seed, drop=None, seg=SEG):
    """split at the smallest pitch, join into a separate output and (base) onto the base itself.  Audited: the split writes [0, m)
    of each plane and [0, t) of the tail, the join [0, n) of its output; the pitch gaps and every slack are hard.  drop: the name
    of one permitted write range left out (the audit's own test); seg: the restart length of the kinds that have one -> what the
    calls returned"""
    d, base = flat_input(fam, esize, m, t)
    n, pitch = d.size, up256(m)
    tag = "%s esize %d (m %d, t %d), seg %d, poison %s" % (fam_name(fam), esize, m, t, seg, poison)
    specs, alias = flat_specs(fam, esize, m, t)
    A = arena(torch, specs, poison, seed, alias)
    A.put("in", d)
    if base is not None:
        A.put("base", base)
        A.put("io.base", base)
    y = forward(fam, d, base, esize, seg)
    planes, tail = PL.split(y, esize)
    writes = plane_writes("planes", esize, pitch, m) + [("tail", 0, t)]
    if drop == "tail":
        writes = writes[:-1]
    ok(A.call(lambda: split_flat(fam, A, n, esize, pitch, seg), tag + ": split", writes), tag + ": split")
    got_planes = A.get("planes", esize * pitch).reshape(esize, pitch)[:, :m]
    got_tail = A.get("tail", t)
    assert np.array_equal(got_planes, planes), "%s: split: %s" % (tag, PM.first_difference("planes", got_planes, planes))
    assert np.array_equal(got_tail, tail), tag + ": split: the tail bytes"
    got = dict(planes=got_planes, tail=got_tail, out=[])
    ok(A.call(lambda: join_flat(fam, A, n, esize, pitch, seg=seg), tag + ": join", [("out", 0, n)]), tag + ": join")
    got["out"].append(A.get("out", n))
    if base is not None:                                       # in place: d_out is the address the base is read from
        assert A.ptr("io.out") == A.ptr("io.base")
        ok(A.call(lambda: join_flat(fam, A, n, esize, pitch, "io.out", "io.base"), tag + ": join in place", [("io.out", 0, n)]), tag + ": join in place")
        got["out"].append(A.get("io.out", n))
    for o in got["out"]:
        assert np.array_equal(o, d), "%s: join(split(x)) != x: %s" % (tag, PM.first_difference("bytes", o, d))
    return got


def hist_model(fam, d, base, esize, seg, filters=7):
    """uint64 [3, esize, 256]: row f under the family's filter f"""
    d = np.ascontiguousarray(d, dtype=np.uint8)
    d = d[:d.size // esize * esize]
    h = np.zeros((3, esize, 256), dtype=np.uint64)
    for f in range(3):
        if filters >> f & 1:
            y = d if f == 0 else forward((fam[0], f, fam[2]), d, base, esize, seg)
            for k, p in enumerate(PL.split(y, esize)[0]):
                h[f, k] = np.bincount(p, minlength=256)
    return h


def run_hist(torch, fam, esize, m, t, poison, seed, drop=None):
    """trc_planes_hist_dev (filter), trc_planes_hist_stride_dev (sfilter) or trc_planes_hist_base_dev (base), all three filters,
    into exactly trc_planes_hist_bytes(esize) poisoned bytes"""
    kind, _, s = fam
    d, base = flat_input(fam, esize, m, t)
    n, hb = d.size, trc.planes_hist_bytes(esize)
    assert hb == 3 * esize * 256 * 8
    tag = "hist %s esize %d (m %d, t %d), poison %s" % (fam_name(fam), esize, m, t, poison)
    A = arena(torch, [("in", n), ("hist", hb)] + ([("base", m * esize)] if kind == "base" else []), poison, seed)
    A.put("in", d)
    L = trc.lib()
    if kind == "base":
        A.put("base", base)
        fn = lambda: L.trc_planes_hist_base_dev(7, A.ptr("in"), A.ptr("base"), n, esize, A.ptr("hist"), None)       # noqa: E731
    elif kind == "sfilter":
        fn = lambda: L.trc_planes_hist_stride_dev(7, s, A.ptr("in"), n, esize, SEG, A.ptr("hist"), None)           # noqa: E731
    else:
        fn = lambda: L.trc_planes_hist_dev(7, A.ptr("in"), n, esize, SEG, A.ptr("hist"), None)                    # noqa: E731
    ok(A.call(fn, tag, [] if drop == "hist" else [("hist", 0, hb)]), tag)
    h = A.get("hist", hb).view("<u8").reshape(3, esize, 256).copy()
    exp = hist_model(fam, d, base, esize, SEG)
    assert np.array_equal(h, exp), "%s: %s" % (tag, PM.first_difference("counters", h, exp))
    return dict(hist=h)


def hist_order_specs(esize, m, t):
    return [("in", m * esize + t), ("hist", 4 * esize * 256 * 8)]


def run_hist_order(torch, orders, stride, esize, m, t, poison, seed, drop=None, seg=SEG):
    """trc_planes_hist_order_dev under the order set `orders` into exactly trc_planes_hist_order_bytes(esize) poisoned bytes: the
    header has the call zero all of them first, so the whole buffer is its write range and the rows of an order that was not
    requested are zero, not poison"""
    d, _ = flat_input(("ofilter", 2, stride), esize, m, t)
    n, hb = d.size, trc.planes_hist_order_bytes(esize)
    specs = hist_order_specs(esize, m, t)
    assert hb == specs[1][1]
    tag = "hist orders %d stride %d esize %d (m %d, t %d), seg %d, poison %s" % (orders, stride, esize, m, t, seg, poison)
    A = arena(torch, specs, poison, seed)
    A.put("in", d)
    fn = lambda: trc.lib().trc_planes_hist_order_dev(orders, stride, A.ptr("in"), n, esize, seg, A.ptr("hist"), None)      # noqa: E731
    ok(A.call(fn, tag, [] if drop == "hist" else [("hist", 0, hb)]), tag)
    h = A.get("hist", hb).view("<u8").reshape(4, esize, 256).copy()
    exp = OL.hist4(d, esize, seg, stride, orders).reshape(4, esize, 256)
    assert not exp[[k for k in range(4) if not orders >> k & 1]].any()
    assert np.array_equal(h, exp), "%s: %s" % (tag, PM.first_difference("counters", h, exp))
    return dict(hist=h)


FP_SIZES = (0, 1, 15, 16, 17, 4099)


def run_fingerprint(torch, nbytes, poison, seed):
    """trc_base_fingerprint_dev over a base of nbytes with no slack: the poison directly behind it must not reach the value"""
    d = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    tag = "fingerprint of %d bytes, poison %s" % (nbytes, poison)
    A = arena(torch, [("base", nbytes), ("fp", 8)], poison, seed)
    A.put("base", d)
    ok(A.call(lambda: trc.lib().trc_base_fingerprint_dev(A.ptr("base"), nbytes, A.ptr("fp"), None), tag, [("fp", 0, 8)]), tag)
    fp = int(A.get("fp", 8).view("<u8")[0])
    assert fp == BPL.fingerprint(d), "%s: %#x, the model has %#x" % (tag, fp, BPL.fingerprint(d))
    return dict(fp=np.array([fp], dtype=np.uint64))


# --------------------------------------------------------------------------------------------- B. the coded flat calls ---
CODED_SHAPES = ((66, 37), (3, 3))                              # (chunks per plane, elements of the last one); t = esize - 1, then 0
CODED_FAMILIES = ("planes", "fplanes", "splanes", "bplanes", "oplanes")
CODED_ORDERS = ((2, 3), (3, 8))                                # (order, stride) of the oplanes cases
PLAIN_CODERS = (trc.ANS4S, trc.RCS1, trc.RCA, trc.RCB, trc.ANSO1)
FILTERED_CODERS = (trc.ANS4S, trc.RCA)
PLANE_SEED = {}                                                # (codec, esize, shape, plane) -> seed, where 10 * plane misses the mix


def coded_cases():
    """(family, codec, esize, shape) and, for oplanes, (order, stride) behind them: esize 4 for every coder, 2 and 8 for ans4s"""
    out = []
    for fam in CODED_FAMILIES:
        for codec in (PLAIN_CODERS if fam == "planes" else FILTERED_CODERS):
            for esize in ((2, 4, 8) if codec == trc.ANS4S else (4,)):
                for shape in CODED_SHAPES:
                    out += [(fam, codec, esize, shape, pred) for pred in CODED_ORDERS] if fam == "oplanes" else [(fam, codec, esize, shape)]
    return out


def case_id(c):
    return "%s-%s-e%d-%dx%d" % (c[0], trc.CODEC_NAMES[c[1]], c[2], c[3][0], c[3][1]) + ("-o%d-s%d" % c[4] if len(c) > 4 else "")


_coded = {}


class Coded:
    """one input of one coded call: plane k is planes_matrix_lib.mixed_input of the coder with seed 10 k, the call's input the
    join of the planes with its t tail bytes behind the family's inverse filter; .exp[k] = what the oracle gives for plane k.
    pred: (order, stride) of an oplanes case; .stride is the family's stride, .order the predictor's order where it has one"""

    def __init__(self, fam, codec, esize, shape, pred=None):
        assert (pred is not None) == (fam == "oplanes")
        self.fam, self.codec, self.esize, self.shape = fam, codec, esize, shape
        self.order, self.stride = pred if pred else (None, 3 if fam == "splanes" else 0)
        self.name = trc.CODEC_NAMES[codec]
        nch, last = shape
        self.chunk = chunk = PM.chunk_of(codec)
        self.planes = np.stack([PM.mixed_input(codec, nch, last, PLANE_SEED.get((codec, esize, shape, k), 10 * k), chunk)[2] for k in range(esize)])
        self.m, self.nc = self.planes.shape[1], nch
        assert self.m == (nch - 1) * chunk + last
        self.t = esize - 1 if nch > 3 else 0
        rng = np.random.default_rng(esize + nch)
        self.tail = rng.integers(0, 256, self.t, dtype=np.uint8)
        self.filtered = PL.join(self.planes, self.tail)
        self.n = self.filtered.size
        self.filt = FL.ZDELTA if codec == trc.ANS4S else FL.XOR
        self.base = FL.gen("random", esize, self.m, 0, 3 + esize) if fam == "bplanes" else None
        self.model = {"planes": ("plain", 0, 0), "fplanes": ("filter", self.filt, 0), "splanes": ("sfilter", self.filt, self.stride),
                      "bplanes": ("base", self.filt, 0), "oplanes": ("ofilter", self.order, self.stride)}[fam]
        self.d = inverse(self.model, self.filtered, self.base, esize, chunk)
        assert np.array_equal(forward(self.model, self.d, self.base, esize, chunk), self.filtered)
        self.static = codec in trc.STATIC
        self.cdfnum = trc._cdfnum(codec, 256, (5, 6))
        self.pitch = up256(self.m + PAD)
        self.range = (63, 2) if nch >= 65 else (0, 1)
        first, count = self.range
        self.range_elems = (first * chunk, min(self.m, (first + count) * chunk))
        self.range_bytes = (self.range_elems[1] - self.range_elems[0]) * esize
        self.tag = "%s %s esize %d (%d, %d) chunk %d" % (fam_name(self.model) if pred else fam, self.name, esize, nch, last, chunk)
        self._exp = None

    @property
    def exp(self):
        """per plane: dict(clen, payload, cdf (or None))"""
        if self._exp is None:
            self._exp = oracle_planes(self.codec, self.planes, self.chunk)
        return self._exp

    def mix(self):
        """per plane (raw, coded) chunks of the oracle's directory"""
        lens = np.minimum(self.chunk, self.m - np.arange(0, self.m, self.chunk))
        return [(int((e["clen"] == lens).sum()), int((e["clen"] < lens).sum())) for e in self.exp]

    def work_bytes(self):
        L = trc.lib()
        return (L.trc_planes_work_bytes(self.codec, self.n, self.esize, self.chunk),
                L.trc_planes_range_work_bytes(self.codec, self.n, self.esize, self.chunk, self.range[1]))

    def specs(self):
        wb, rwb = self.work_bytes()
        assert wb and rwb and self.pitch == trc.planes_pitch(self.n, self.esize), self.tag
        e = self.esize
        s = [("in", self.n), ("work", wb), ("clen", 4 * e * self.nc), ("payload", e * self.pitch), ("total", 8 * e), ("tail", 8),
             ("cdf", 2 * e * CDF_STRIDE), ("status", 4 * e), ("out", self.n), ("range_out", self.range_bytes), ("range_work", rwb), ("b.work", wb)]
        if self.fam == "bplanes":
            s += [("base", self.m * e), ("io.base", self.n)]
        return s, ({"io.out": "io.base"} if self.fam == "bplanes" else None)


def coded(fam, codec, esize, shape, pred=None):
    key = (fam, codec, esize, shape, pred)
    if key not in _coded:
        _coded[key] = Coded(*key)
    return _coded[key]


def _lead(c):
    return {"planes": (), "fplanes": (c.filt,), "splanes": (c.filt, c.stride), "bplanes": (c.filt,), "oplanes": (c.order, c.stride)}[c.fam]


def _fn(c, what):
    return getattr(trc.lib(), {"planes": "trc_%s_planes%s_dev", "fplanes": "trc_%s_fplanes%s_dev", "splanes": "trc_%s_splanes%s_dev",
                               "bplanes": "trc_%s_bplanes%s_dev", "oplanes": "trc_%s_oplanes%s_dev"}[c.fam] % what)


def encode_coded(c, A, work_bytes):
    cdf, status = (A.ptr("cdf"), A.ptr("status")) if c.static else (None, None)
    src = (A.ptr("in"), A.ptr("base")) if c.fam == "bplanes" else (A.ptr("in"),)
    return _fn(c, ("encode", ""))(c.codec, *_lead(c), *src, c.n, c.esize, c.chunk, cdf, c.cdfnum, status, A.ptr("clen"), A.ptr("payload"),
                                  A.ptr("total"), A.ptr("tail"), A.ptr("work"), work_bytes, None)


def decode_coded(c, A, out, work, work_bytes, base="base"):
    b = (A.ptr(base),) if c.fam == "bplanes" else ()
    return _fn(c, ("decode", ""))(c.codec, *_lead(c), A.ptr("clen"), A.ptr("payload"), A.ptr("tail"), *b, c.n, c.esize, c.chunk,
                                  A.ptr("cdf") if c.static else None, c.cdfnum, out, A.ptr(work), work_bytes, None)


def decode_range_coded(c, A, out, work_bytes, base="base"):
    b = (A.ptr(base),) if c.fam == "bplanes" else ()
    return _fn(c, ("decode", "_range"))(c.codec, *_lead(c), A.ptr("clen"), A.ptr("payload"), *b, c.n, c.esize, c.chunk, c.range[0], c.range[1],
                                        A.ptr("cdf") if c.static else None, c.cdfnum, out, A.ptr("range_work"), work_bytes, None)


def oracle_planes(codec, planes, chunk):
    """per plane what trc_encode_dev gives for it, by the oracle: dict(clen, payload, cdf = (status, CDF) or None)"""
    out = []
    for p in planes:
        cdf = T.orc_cdfini(p, 256)[:2] if codec in trc.STATIC else None
        payload, clen, _ = T.orc_chunked_enc(codec, p, chunk, cdf[1] if cdf else None, 256)
        out.append(dict(clen=clen, payload=payload, cdf=cdf))
    return out


def encode_rules(A, e, nc, pitch, x, static, drop=None, payload="payload"):
    """(writes, soft) of a coded planes encode into the buffers clen, `payload`, total, work, cdf, status: plane k writes its
    directory, [0, total_k) of its payload slice, its total, 257 entries of its CDF slot and its status; writable slack (recorded,
    else open as far as PLANES_ALLOW says): the slack of clen, total, work, status and the payload buffer, [total_k + 64, pitch)
    of every payload slice, the 7 spare entries of every CDF slot.  [total_k, total_k + 64) is hard"""
    totals = [int(x[k]["payload"].size) for k in range(e)]
    writes = [("clen", 0, 4 * e * nc), ("total", 0, 8 * e), ("work", 0, A.layout["work"].size)]
    writes += [(payload, k * pitch, k * pitch + totals[k]) for k in range(e) if not (drop == "payload" and k == e - 1)]
    soft = [GA.slack(A, "clen"), GA.slack(A, "total"), GA.slack(A, "work"), GA.slack(A, payload)]
    soft += [(payload, k * pitch + totals[k] + 64, (k + 1) * pitch, k * pitch + totals[k]) for k in range(e) if totals[k] + 64 < pitch]
    if static:
        writes += [("status", 0, 4 * e)] + [("cdf", 2 * CDF_STRIDE * k, 2 * CDF_STRIDE * k + 514) for k in range(e)]
        soft += [GA.slack(A, "status"), GA.slack(A, "cdf")]
        soft += [("cdf", 2 * CDF_STRIDE * k + 514, 2 * CDF_STRIDE * (k + 1), 2 * CDF_STRIDE * k + 514) for k in range(e)]
    return writes, soft


def check_encoded(A, tag, e, nc, pitch, m, x, static, payload="payload"):
    """directory, payload, total, CDF and status of every plane against the oracle's -> what the call returned"""
    if A.buf.is_cuda:
        A.torch.cuda.synchronize()
    clen = A.get("clen", 4 * e * nc).view("<u4").reshape(e, nc).copy()
    total = A.get("total", 8 * e).view("<u8").astype(np.int64)
    pl = A.get(payload, e * pitch).reshape(e, pitch)
    for k in range(e):
        want = int(x[k]["payload"].size)
        msg = PM.first_difference("directory", clen[k], x[k]["clen"]) or \
            PM.first_difference("payload", pl[k, :min(max(int(total[k]), 0), pitch)], x[k]["payload"], clen=x[k]["clen"])
        assert not msg and total[k] == want, "%s, plane %d: %s (total %d, the oracle has %d)" % (tag, k, msg, total[k], want)
    got = dict(clen=clen, total=total, payload=np.concatenate([pl[k, :int(total[k])] for k in range(e)]), out=[])
    if static:
        got["cdf"] = A.get("cdf", 2 * e * CDF_STRIDE).view("<u2").reshape(e, CDF_STRIDE)[:, :257].copy()
        got["status"] = A.get("status", 4 * e).view("<i4").copy()
        for k in range(e):
            assert got["status"][k] == x[k]["cdf"][0] == m and np.array_equal(got["cdf"][k], x[k]["cdf"][1]), "%s: CDF / status of plane %d" % (tag, k)
    return got


def run_coded(torch, c, poison, seed, drop=None):
    """encode, decode, a chunk range in its own exact-size workspace and output, a decode in a second workspace that holds poison
    and has never encoded, (bplanes) the whole and the range decoded onto the base; then one byte short of either workspace"""
    e, m, n, nc, pitch, x = c.esize, c.m, c.n, c.nc, c.pitch, c.exp
    specs, alias = c.specs()
    A = arena(torch, specs, poison, seed, alias)
    L = A.layout
    A.put("in", c.d)
    if c.base is not None:
        A.put("base", c.base)
        A.put("io.base", c.base)
    key = c.fam + ":" + c.name
    kw = dict(coder=key, allow=GA.PLANES_ALLOW)
    tag = "%s, poison %s" % (c.tag, poison)
    wb, rwb = L["work"].size, L["range_work"].size
    writes, soft = encode_rules(A, e, nc, pitch, x, c.static, drop)
    A.snapshot()
    ok(encode_coded(c, A, wb), tag + ": encode")
    got = check_encoded(A, tag + ": encode", e, nc, pitch, m, x, c.static)
    got["tail"] = A.get("tail", c.t)
    assert np.array_equal(got["tail"], c.tail), tag + ": encode: the tail bytes"
    A.audit(tag + ": encode", writes + [("tail", 0, c.t)], soft, **kw)

    def decoded(what, fn, buf, lo, nbytes, want, work, wsize):
        if buf == "io.out":
            A.put("io.base", c.base)
        else:
            A.poison(buf)
        ok(A.call(fn, "%s: %s" % (tag, what), [(buf, lo, lo + nbytes), (work, 0, wsize)], [GA.slack(A, work)], **kw), "%s: %s" % (tag, what))
        out = A.get(buf, lo + nbytes)[lo:]
        msg = PM.first_difference("decoded bytes", out, want, chunk=c.chunk * e)
        assert not msg, "%s: %s: %s" % (tag, what, msg)
        got["out"].append(out)

    first = c.range[0] * c.chunk * e
    want_range = c.d[first:first + c.range_bytes]
    decoded("decode", lambda: decode_coded(c, A, A.ptr("out"), "work", wb), "out", 0, n, c.d, "work", wb)
    decoded("decode_range (%d, %d)" % c.range, lambda: decode_range_coded(c, A, A.ptr("range_out"), rwb), "range_out", 0, c.range_bytes,
            want_range, "range_work", rwb)
    decoded("decode in a decode-only workspace", lambda: decode_coded(c, A, A.ptr("out"), "b.work", wb), "out", 0, n, c.d, "b.work", wb)
    if c.fam == "bplanes":
        decoded("decode in place", lambda: decode_coded(c, A, A.ptr("io.out"), "work", wb, "io.base"), "io.out", 0, n, c.d, "work", wb)
        decoded("decode_range (%d, %d) in place" % c.range, lambda: decode_range_coded(c, A, A.ptr("io.out") + first, rwb, "io.base"), "io.out",
                first, c.range_bytes, want_range, "range_work", rwb)
    A.snapshot()                                               # one byte short: TRC_E_WORK, the whole allocation unchanged
    assert encode_coded(c, A, wb - 1) == GA.TRC_E_WORK, tag + ": encode, one byte short of the workspace"
    assert decode_coded(c, A, A.ptr("out"), "work", wb - 1) == GA.TRC_E_WORK, tag + ": decode, one byte short of the workspace"
    assert decode_range_coded(c, A, A.ptr("range_out"), rwb - 1) == GA.TRC_E_WORK, tag + ": decode_range, one byte short of the range workspace"
    A.audit(tag + ": calls refused with TRC_E_WORK")
    return got


# ------------------------------------------------------------------------------------------------------ C. the batches ---
BATCH_SIZES = [1, 256, 7, 513, 64, 1, 257, 2049, 255, 256, 9, 300]      # m[i], in elements: one-element items, items of exactly one chunk
BATCH_CHUNK = 256
BATCH_FAMILIES = ("batch", "fbatch", "sbatch", "bbatch")
BATCH_CODERS = (trc.ANS4S, trc.RCA)


def ranges(count):
    return [(0, 1), (3, 1), (count - 1, 1), (2, 5), (0, count)]


class Batch:
    """twelve items, each a buffer of its own with no slack, per-item filters / strides / bases by family; .virtual = the model's
    virtual buffer V([G(0) .. G(count - 1)])"""

    def __init__(self, fam, esize, coded_for=None):
        self.fam, self.esize, self.chunk = fam, esize, BATCH_CHUNK
        self.count = count = len(BATCH_SIZES)
        self.sizes = [m * esize for m in BATCH_SIZES]
        if coded_for is None:
            self.datas = [SL.gen("interleaved", esize, m, 0, 40 + i + esize, 1 + i % 8) if fam == "sbatch" else
                          FL.gen(FL.KINDS[i % 4], esize, m, 0, 70 + i + esize) for i, m in enumerate(BATCH_SIZES)]
        else:                                                  # weights with uniform spans, so that raw and coded chunks mix
            self.datas = [PL.mixed_weights(m, esize, self.chunk, 0, seed=11 + i) for i, m in enumerate(BATCH_SIZES)]
        self.filters = None if fam == "batch" else [(i + 1) % 3 for i in range(count)]
        self.strides = [1 + (5 * i) % 8 for i in range(count)] if fam == "sbatch" else None
        self.bases = [FL.gen("random", esize, m, 0, 90 + i) for i, m in enumerate(BATCH_SIZES)] if fam == "bbatch" else None
        self.plan, self.first = BL.plan(self.sizes, esize, self.chunk)
        self.M, self.NC = self.plan["m_total"], self.plan["chunks"]
        g = []
        for i, d in enumerate(self.datas):
            f = 0 if self.filters is None else self.filters[i]
            if f == 0:
                g.append(d)
            elif fam == "bbatch":
                g.append(BPL.forward(d, self.bases[i], esize, f))
            else:
                g.append(SL.forward(d, esize, f, self.chunk, 1 if self.strides is None else self.strides[i]))
        self.virtual = BL.virtual(g, esize, self.chunk)
        assert self.virtual.size == self.plan["n_virtual"]
        self.table_fn = trc.lib().trc_planes_bbatch_table_bytes if fam == "bbatch" else trc.lib().trc_planes_batch_table_bytes

    def item_specs(self, prefix="i"):
        return [("%s%d.item" % (prefix, i), n) for i, n in enumerate(self.sizes)]

    def base_specs(self):
        return [("b%d.base" % i, n) for i, n in enumerate(self.sizes)] if self.bases is not None else []

    def items(self, A, prefix="i", only=None):
        return trc.planes_items([(A.ptr("%s%d.item" % (prefix, i)) if only is None or i in only else None, n) for i, n in enumerate(self.sizes)])

    def base_ptrs(self, A, only=None, onto=None):
        """the bases' addresses; onto = (item index, buffer): that item's base is that buffer (in place)"""
        if self.bases is None:
            return None
        p = [A.ptr("b%d.base" % i) if only is None or i in only else None for i in range(self.count)]
        if onto is not None:
            p[onto[0]] = A.ptr(onto[1])
        return (C.c_void_p * self.count)(*p)

    def fam_args(self, A, only=None, onto=None):
        """what the family's calls take behind `items`"""
        fl = trc.planes_filters(self.filters, self.count)
        if self.fam == "batch":
            return ()
        if self.fam == "fbatch":
            return (fl,)
        if self.fam == "sbatch":
            return (fl, trc.planes_strides(self.strides, self.count))
        return (self.base_ptrs(A, only, onto), fl)

    def put(self, A):
        for i, d in enumerate(self.datas):
            A.put("i%d.item" % i, d)
        for i, b in enumerate(self.bases or []):
            A.put("b%d.base" % i, b)


def _bfn(fam, what):
    """the family's C entry point: what = "planes_split_%s_dev", "encode_%s_dev" ..."""
    names = {"batch": ("batch", "planes_batch"), "fbatch": ("fbatch", "fplanes_batch"), "sbatch": ("sbatch", "splanes_batch"),
             "bbatch": ("bbatch", "bplanes_batch")}[fam]
    return getattr(trc.lib(), "trc_" + (what % names[0] if what.startswith("planes_") else what % names[1]))


def run_batch_kernels(torch, fam, esize, poison, seed, drop=None):
    """the batched split into planes at the smallest pitch with a table of exactly its bytes; the whole join; the join of every
    range of ranges(count) from a 64-byte placed copy of the range's planes with NULL pointers outside the range"""
    b = Batch(fam, esize)
    count, chunk, M, first = b.count, b.chunk, b.M, b.first
    pitch = up256(M)
    tb = b.table_fn(count, b.NC)
    rng_specs = []
    for j, (fi, ic) in enumerate(ranges(count)):
        elems = min(M, first[fi + ic] * chunk) - first[fi] * chunk
        rng_specs += [("r%d.jplanes" % j, esize * up256(elems)), ("r%d.table" % j, b.table_fn(ic, first[fi + ic] - first[fi]))]
    specs = b.item_specs() + b.base_specs() + [("planes", esize * pitch), ("table", tb)] + b.item_specs("o") + rng_specs
    A = arena(torch, specs, poison, seed)
    b.put(A)
    tag = "%s esize %d, poison %s" % (fam, esize, poison)
    planes = PL.split(b.virtual, esize)[0]
    writes = plane_writes("planes", esize, pitch, M) + [("table", 0, tb)]
    ok(A.call(lambda: _bfn(fam, "planes_split_%s_dev")(b.items(A), *b.fam_args(A), count, esize, chunk, A.ptr("planes"), pitch, A.ptr("table"), tb, None),
              tag + ": split", writes[:-1] if drop == "table" else writes), tag + ": split")
    got_planes = A.get("planes", esize * pitch).reshape(esize, pitch)[:, :M].copy()
    assert np.array_equal(got_planes, planes), "%s: split: %s" % (tag, PM.first_difference("planes of the virtual buffer", got_planes, planes))
    got = dict(planes=got_planes, out=[])

    def joined(what, d_planes, jpitch, fi, ic, table, tbytes):
        only = range(fi, fi + ic)
        for i in range(count):
            A.poison("o%d.item" % i)
        w = [("o%d.item" % i, 0, b.sizes[i]) for i in only] + [(table, 0, tbytes)]
        ok(A.call(lambda: _bfn(fam, "planes_join_%s_dev")(d_planes, jpitch, b.items(A, "o", only), *b.fam_args(A, only), count, fi, ic, esize, chunk,
                                                          A.ptr(table), tbytes, None), "%s: %s" % (tag, what), w), "%s: %s" % (tag, what))
        for i in only:
            o = A.get("o%d.item" % i, b.sizes[i])
            assert np.array_equal(o, b.datas[i]), "%s: %s: item %d: %s" % (tag, what, i, PM.first_difference("bytes", o, b.datas[i]))
            got["out"].append(o)

    joined("join of all items", A.ptr("planes"), pitch, 0, count, "table", tb)
    for j, (fi, ic) in enumerate(ranges(count)):
        e0 = first[fi] * chunk
        elems = min(M, first[fi + ic] * chunk) - e0
        jp = up256(elems)
        img = np.zeros((esize, jp), dtype=np.uint8)
        img[:, :elems] = planes[:, e0:e0 + elems]
        img[:, elems:] = A.get("r%d.jplanes" % j, esize * jp).reshape(esize, jp)[:, elems:]      # the pitch gap keeps its poison
        A.put("r%d.jplanes" % j, img)
        joined("join of items (%d, %d) from planes at 64 (mod 128)" % (fi, ic), A.ptr("r%d.jplanes" % j), jp, fi, ic, "r%d.table" % j,
               A.layout["r%d.table" % j].size)
    return got


def _range_work_fn(fam):
    return trc.lib().trc_planes_bbatch_range_work_bytes if fam == "bbatch" else trc.lib().trc_planes_batch_range_work_bytes


def _coded_batch(fam, codec, payload="payload"):
    """-> (the batch of esize 4, the oracle's planes of its virtual buffer, the specs of its coded buffers, cdfnum, encode workspace bytes)"""
    b = Batch(fam, 4, coded_for=codec)
    e, L = b.esize, trc.lib()
    x = oracle_planes(codec, PL.split(b.virtual, e)[0], b.chunk)
    null = trc.planes_items([(16, n) for n in b.sizes])      # the size functions refuse a NULL or misaligned pointer and read none
    wb = (L.trc_planes_bbatch_work_bytes if fam == "bbatch" else L.trc_planes_batch_work_bytes)(codec, null, b.count, e, b.chunk)
    pitch = up256(b.M + PAD)
    assert wb and pitch == b.plan["pitch"]
    specs = b.item_specs() + b.base_specs() + [("work", wb), ("clen", 4 * e * b.NC), (payload, e * pitch), ("total", 8 * e),
                                               ("cdf", 2 * e * CDF_STRIDE), ("status", 4 * e)] + b.item_specs("o")
    return b, x, specs, trc._cdfnum(codec, 256, (5, 6)), wb


def _encode_batch(A, b, codec, cdfnum, wb, tag, kw, x, payload="payload"):
    e, static = b.esize, codec in trc.STATIC
    pitch = b.plan["pitch"]
    writes, soft = encode_rules(A, e, b.NC, pitch, x, static, payload=payload)
    A.snapshot()
    ok(_bfn(b.fam, "encode_%s_dev")(codec, b.items(A), *b.fam_args(A), b.count, e, b.chunk, A.ptr("cdf") if static else None, cdfnum,
                                    A.ptr("status") if static else None, A.ptr("clen"), A.ptr(payload), A.ptr("total"), A.ptr("work"), wb, None),
       tag + ": encode")
    got = check_encoded(A, tag + ": encode", e, b.NC, pitch, b.M, x, static, payload)
    A.audit(tag + ": encode", writes, soft, **kw)
    return got


def run_batch_coded(torch, fam, codec, poison, seed):
    """the coded batch: encode in a workspace of exactly its bytes, then every item range of ranges(count) decoded in a workspace
    of exactly trc_planes_(b)batch_range_work_bytes with NULL pointers outside it; bbatch: item 3 alone decoded onto its own base"""
    b, x, specs, cdfnum, wb = _coded_batch(fam, codec)
    e, count, static = b.esize, b.count, codec in trc.STATIC
    null = trc.planes_items([(16, n) for n in b.sizes])      # the size functions refuse a NULL or misaligned pointer and read none
    rwb = [_range_work_fn(fam)(codec, null, count, e, b.chunk, fi, ic) for fi, ic in ranges(count)]
    assert all(rwb)
    A = arena(torch, specs + [("r%d.range_work" % j, w) for j, w in enumerate(rwb)], poison, seed)
    b.put(A)
    name = trc.CODEC_NAMES[codec]
    kw = dict(coder=fam + ":" + name, allow=GA.PLANES_ALLOW)
    tag = "%s %s esize %d, poison %s" % (fam, name, e, poison)
    got = _encode_batch(A, b, codec, cdfnum, wb, tag, kw, x)

    def decode(what, fi, ic, work, onto=None):
        only = range(fi, fi + ic)
        for i in range(count):
            A.poison("o%d.item" % i)
        items = b.items(A, "o", only)
        dst = {i: "o%d.item" % i for i in only}
        if onto is not None:                                   # in place: the item's pointer is its base's
            A.put("b%d.base" % onto, b.bases[onto])
            items[onto].d_ptr = A.ptr("b%d.base" % onto)
            dst[onto] = "b%d.base" % onto
        wsize = A.layout[work].size
        w = [(dst[i], 0, b.sizes[i]) for i in only] + [(work, 0, wsize)]
        ok(A.call(lambda: _bfn(fam, "decode_%s_dev")(codec, A.ptr("clen"), A.ptr("payload"), items, *b.fam_args(A, only), count, fi, ic, e, b.chunk,
                                                     A.ptr("cdf") if static else None, cdfnum, A.ptr(work), wsize, None),
                  "%s: %s" % (tag, what), w, [GA.slack(A, work)], **kw), "%s: %s" % (tag, what))
        for i in only:
            o = A.get(dst[i], b.sizes[i])
            assert np.array_equal(o, b.datas[i]), "%s: %s: item %d: %s" % (tag, what, i, PM.first_difference("bytes", o, b.datas[i], chunk=b.chunk * e))
            got["out"].append(o)
        if onto is not None:
            A.put("b%d.base" % onto, b.bases[onto])

    for j, (fi, ic) in enumerate(ranges(count)):
        decode("decode of items (%d, %d)" % (fi, ic), fi, ic, "r%d.range_work" % j)
    if fam == "bbatch":
        assert b.filters[3] != 0 and ranges(count)[1] == (3, 1)
        decode("decode of item 3 onto its own base", 3, 1, "r1.range_work", onto=3)
    return got


def run_batch_container(torch, fam, codec, poison, seed):
    """fbatch: trc_planes_batch_pack_dev (the TRCB container); sbatch: trc_planes_sbatch_pack_dev (TRCT).  The coded batch (its
    payload 4-byte placed, as the pack call asks) is packed into exactly the bound's bytes at 16 (the header's rule for the pack's
    d_out), checked against the layout functions and the oracle's sections, copied to a container buffer at 8 (mod 16) of exactly
    the bound's bytes, and every item range is decoded from there in an exact-size workspace.  (For the TRCT container the header
    asks for 16 bytes at d_cont; the call checks 8, its prefix is a multiple of 16, and the kernels read the TRCB part at 8 (mod 16)
    exactly as they do for a TRCB container: the case runs at 8 (mod 16) too.)"""
    assert fam in ("fbatch", "sbatch")
    b, x, specs, cdfnum, wb = _coded_batch(fam, codec, "payload4")
    e, count, static, L = b.esize, b.count, codec in trc.STATIC, trc.lib()
    null = trc.planes_items([(16, n) for n in b.sizes])      # the size functions refuse a NULL or misaligned pointer and read none
    bound = (L.trc_planes_sbatch_bound if fam == "sbatch" else L.trc_planes_batch_bound)(codec, null, count, e, b.chunk, cdfnum)
    rwb = [L.trc_planes_batch_range_work_bytes(codec, null, count, e, b.chunk, fi, ic) for fi, ic in ranges(count)]
    assert bound and all(rwb)
    A = arena(torch, specs + [("packed.out", bound), ("size", 8), ("cont", bound)] + [("r%d.range_work" % j, w) for j, w in enumerate(rwb)], poison, seed)
    b.put(A)
    name = trc.CODEC_NAMES[codec]
    kw = dict(coder=fam + ":" + name, allow=GA.PLANES_ALLOW)
    tag = "%s %s container, poison %s" % (fam, name, poison)
    got = _encode_batch(A, b, codec, cdfnum, wb, tag, kw, x, "payload4")
    totals = [int(p["payload"].size) for p in x]
    lay = trc.planes_batch_layout(codec, b.sizes, e, b.chunk, cdfnum, totals)
    import planes_container_lib as CL
    assert (lay["inner"], lay["off"], lay["size"]) == CL.layout(b.sizes, e, b.chunk, codec, cdfnum, totals), tag + ": trc_planes_batch_layout_host"
    prefix = trc.planes_sbatch_prefix(count) if fam == "sbatch" else 0
    size = prefix + lay["size"]
    assert size <= bound - PAD
    fam_args = b.fam_args(A)
    pack = L.trc_planes_sbatch_pack_dev if fam == "sbatch" else L.trc_planes_batch_pack_dev
    ok(A.call(lambda: pack(codec, b.items(A), *fam_args, count, e, b.chunk, A.ptr("cdf") if static else None, cdfnum, A.ptr("status") if static else None,
                           A.ptr("clen"), A.ptr("payload4"), A.ptr("total"), A.ptr("packed.out"), bound, A.ptr("size"), None),
              tag + ": pack", [("packed.out", 0, size), ("size", 0, 8)]), tag + ": pack")
    assert int(A.get("size", 8).view("<u8")[0]) == size, tag + ": *d_size is %d, the layout gives %d" % (int(A.get("size", 8).view("<u8")[0]), size)
    cont = A.get("packed.out", size)
    if fam == "sbatch":
        trc.planes_sbatch_check(cont, count)
        stored = [s if f else 1 for s, f in zip(b.strides, b.filters)]          # "the stored stride of an item without a filter is 1"
        assert trc.planes_sbatch_info(cont)[3] == stored, tag + ": the strides of the TRCT prefix"
    body = cont[prefix:]
    trc.planes_batch_check(body, count)
    front = CL.front(b.sizes, b.filters, e, b.chunk, lay["size"])
    assert np.array_equal(body[:lay["inner"]], front), tag + ": header, n[] or filters: " + PM.first_difference("front", body[:lay["inner"]], front)
    assert np.array_equal(body[lay["inner"] + 32:lay["inner"] + 32 + 8 * e].view("<u8"), np.array(lay["off"]) - lay["inner"]), tag + ": the section offsets"
    cdfb = CL.up8(2 * (cdfnum + 1)) if static else 0
    ends = lay["off"][1:] + [lay["size"]]
    for k in range(e):
        o = lay["off"][k]
        if static:
            want = np.zeros(cdfb, dtype=np.uint8)
            want[:514] = x[k]["cdf"][1].astype("<u2").view(np.uint8)
            assert np.array_equal(body[o:o + cdfb], want), tag + ": the CDF of section %d" % k
        o += cdfb
        assert int(body[o + 24:o + 32].view("<u8")[0]) == totals[k], tag + ": the payload size in the header of section %d" % k
        o += 32
        assert np.array_equal(body[o:o + 4 * b.NC].view("<u4"), x[k]["clen"]), tag + ": the directory of section %d" % k
        o += 4 * b.NC
        assert np.array_equal(body[o:o + totals[k]], x[k]["payload"]), tag + ": the payload of section %d" % k
        assert not body[o + totals[k]:ends[k]].any() and ends[k] - o - totals[k] < 8, tag + ": the zero bytes behind section %d" % k
    got["container"] = cont
    A.put("cont", cont)                                        # at 8 (mod 16); TRC_PAD readable bytes behind `size`: poison
    assert A.ptr("cont") % 16 == 8
    tot = (C.c_uint64 * 8)(*totals)
    unpack = L.trc_decode_splanes_batch_packed_dev if fam == "sbatch" else L.trc_decode_planes_batch_packed_dev
    for j, (fi, ic) in enumerate(ranges(count)):
        only = range(fi, fi + ic)
        for i in range(count):
            A.poison("o%d.item" % i)
        work, what = "r%d.range_work" % j, "%s: packed decode of items (%d, %d)" % (tag, fi, ic)
        w = [("o%d.item" % i, 0, b.sizes[i]) for i in only] + [(work, 0, rwb[j])]
        ok(A.call(lambda: unpack(codec, A.ptr("cont"), bound, b.items(A, "o", only), *fam_args, count, fi, ic, e, b.chunk, cdfnum, tot,
                                 A.ptr(work), rwb[j], None), what, w, [GA.slack(A, work)], **kw), what)
        for i in only:
            o = A.get("o%d.item" % i, b.sizes[i])
            assert np.array_equal(o, b.datas[i]), "%s: item %d: %s" % (what, i, PM.first_difference("bytes", o, b.datas[i], chunk=b.chunk * e))
            got["out"].append(o)
    return got


def run_batch_hist(torch, fam, esize, poison, seed):
    """trc_planes_hist_batch_dev (batch) / trc_planes_hist_sbatch_dev (sbatch), all three filters, for every range of
    ranges(count): histograms and table of exactly their bytes, NULL pointers outside the range"""
    b = Batch(fam, esize)
    count, L = b.count, trc.lib()
    specs = b.item_specs()
    for j, (fi, ic) in enumerate(ranges(count)):
        specs += [("r%d.hist" % j, L.trc_planes_hist_batch_bytes(ic, esize)), ("r%d.table" % j, L.trc_planes_batch_table_bytes(ic, b.first[fi + ic] - b.first[fi]))]
    A = arena(torch, specs, poison, seed)
    b.put(A)
    got = dict(out=[])
    strides = trc.planes_strides(b.strides, count)
    for j, (fi, ic) in enumerate(ranges(count)):
        tag = "hist %s esize %d items (%d, %d), poison %s" % (fam, esize, fi, ic, poison)
        hb, tb = A.layout["r%d.hist" % j].size, A.layout["r%d.table" % j].size
        assert hb == ic * 3 * esize * 256 * 8 and tb
        items = b.items(A, only=range(fi, fi + ic))
        s = (strides,) if fam == "sbatch" else ()
        fn = L.trc_planes_hist_sbatch_dev if fam == "sbatch" else L.trc_planes_hist_batch_dev
        ok(A.call(lambda: fn(7, items, *s, count, fi, ic, esize, b.chunk, A.ptr("r%d.hist" % j), A.ptr("r%d.table" % j), tb, None), tag,
                  [("r%d.hist" % j, 0, hb), ("r%d.table" % j, 0, tb)]), tag)
        h = A.get("r%d.hist" % j, hb).view("<u8").reshape(ic, 3, esize, 256).copy()
        for i in range(fi, fi + ic):
            exp = hist_model(("sfilter", 0, b.strides[i] if fam == "sbatch" else 1), b.datas[i], None, esize, b.chunk)
            assert np.array_equal(h[i - fi], exp), "%s: item %d: %s" % (tag, i, PM.first_difference("counters", h[i - fi], exp))
        got["out"].append(h)
    return got


def run_batch_advise(torch, esize, poison, seed):
    """trc_planes_advise_batch_dev in a workspace of exactly trc_planes_advise_batch_work_bytes: the choice per item is
    advise_lib's on the model's histograms"""
    b = Batch("batch", esize)
    count, L = b.count, trc.lib()
    null = trc.planes_items([(16, n) for n in b.sizes])      # the size functions refuse a NULL or misaligned pointer and read none
    wb = L.trc_planes_advise_batch_work_bytes(null, count, esize, b.chunk)
    assert wb
    A = arena(torch, b.item_specs() + [("work", wb)], poison, seed)
    b.put(A)
    tag = "advise_batch_dev esize %d, poison %s" % (esize, poison)
    out = (C.c_uint8 * count)()
    ok(A.call(lambda: L.trc_planes_advise_batch_dev(7, b.items(A), count, esize, b.chunk, out, None, A.ptr("work"), wb, None), tag,
              [("work", 0, wb)]), tag)
    want = [AL.advise(AL.hist(d, esize, b.chunk, 7), 7, esize, d.size // esize)[0] for d in b.datas]
    assert [int(v) for v in out] == want, "%s: choices %r, the model has %r" % (tag, [int(v) for v in out], want)
    return dict(filters=np.array([int(v) for v in out]))
