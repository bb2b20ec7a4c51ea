"""Every buffer of a device-layer call out of ONE audited allocation, at the documented minimum geometry of include/trc_hip.h: the
stated size plus TRC_PAD bytes of slack and nothing more, at the documented alignment and no better, a guard zone between any two
buffers and a margin of a megabyte on both sides, everything poisoned (seeded random bytes or 0xFF, never zeros) before the inputs
go into their stated extents.  After every library call the whole allocation is compared, on the device, with the image saved
before the call: whatever changed outside what that call may write is a failed assertion that names the buffer, or the zone
between two buffers, and the first and last offending offset.  Stray READS leave no trace and stay unobserved.

A plain helper module (not collected): Layout (arithmetic only, no device), Arena (the allocation and the audit; CPU tensors work
as well, for tests/test_arena_cpu.py), ArenaCoder (a trc.DeviceCoder on arena views), the case lists of the 60 coders of the codec table and run_case,
the sequence tests/test_gpu_arena.py runs per case and poison.

The slack of an output is "readable/writable" in the header.  What the kernels do to the slack of d_work, d_clen, d_total, d_status
and to d_payload[total + 64, n + TRC_PAD) was recorded once over all cases (TRC_ARENA_RECORD=<file> makes the audit record instead
of judge; profiles/arena/arena_notes.md holds the result): ALLOW lists every such write, everything else is a hard rule.  No coder
wrote any of it, so ALLOW is empty and every rule is hard.

The byte-plane calls use the same Layout and Arena from tests/gpu_planes_arena.py: further buffer kinds with their own alignment,
a slack per kind (none behind a base or a batch item), an alias for the two names of an in-place decode, and PLANES_ALLOW."""
import hashlib
import os

import numpy as np

import bytesweep_lib as B
import planes_matrix_lib as PM
import sweep_lib as S
import trc
import trc_testlib as T

PAD = trc.PAD
MARGIN = 1 << 20                                               # in front of the first and behind the last buffer
ZONE = 4096                                                    # between any two buffers (plus what the next alignment takes)
BASE_ALIGN = 512                                               # layout offsets count from an address that is a multiple of this
# the alignment trc_encode_dev / trc_decode_dev check (include/trc_hip.h); EXACT: placed at an odd multiple of it
ALIGN = {"in": 16, "out": 16, "work": 256, "total": 8, "clen": 4, "payload": 2, "cdf": 256, "status": 256}
EXACT = ("in", "out", "work", "total", "clen", "payload")      # the header states nothing for d_cdf and d_status: they stay 256-aligned
KIND = {"range_out": "out", "range_work": "work", "cdfini_work": "work"}
# the byte-plane calls (tests/gpu_planes_arena.py): a base and a batch item are read in their stated bytes only, so they get NO slack
# and end where the poison of the guard zone begins; planes and tables are 256-byte aligned, the planes a batched join reads 64;
# payload4: d_payload of the pack / packed-decode calls (4); histograms, fingerprint, container and its size 8; the 8-byte tail
# buffer has no stated alignment and lies at an odd address
ALIGN.update({"base": 16, "item": 16, "planes": 256, "table": 256, "jplanes": 64, "payload4": 4, "hist": 8, "fp": 8, "cont": 8,
              "size": 8, "tail": 1})
EXACT += ("base", "item", "planes", "table", "jplanes", "payload4", "hist", "fp", "cont", "size")
ODD = ("tail",)
SLACK = {"base": 0, "item": 0}                                 # bytes of slack behind the stated size; every other kind: TRC_PAD
POISONS = ("random", "ff")
TRC_E_WORK = -3
AVAILABLE_SHAPES = ((129, 100), (66, 37), (63, None))          # (nchunks, tail); None: a full last chunk -- less than one wave
WAVE_CASES = (("edges", 129), ("alt", 63), ("alt", 65))        # of the sweep / bytesweep fixtures, at chunk 256
MIX_MIN = 30                                                   # raw and coded chunks each, at (129, 100), for every coder that stores raw

# (coder name, buffer kind) -> the furthest byte a call writes behind the stated size (d_payload on the encode side: behind
# `total`), as recorded on the MI355X over all cases and both poisons; a pair that is not listed must not be written at all
ALLOW = {}
# the same for the byte-plane calls (tests/gpu_planes_arena.py), keyed ("<call family>:<coder>", buffer kind), as recorded over
# tests/test_gpu_planes_arena.py (profiles/arena/planes_arena_notes.md): nothing was written there either
PLANES_ALLOW = {}

RECORDING = bool(os.environ.get("TRC_ARENA_RECORD"))
RECORD = {}                                                    # filled in recording mode: (coder, kind) -> furthest offset


def kind_of(name):
    k = name.split(".")[-1]
    return KIND.get(k, k)


class Buf:
    def __init__(self, name, size, start):
        self.name, self.size, self.start = name, size, start
        self.kind = kind_of(name)
        self.slack = SLACK.get(self.kind, PAD)                 # exactly TRC_PAD; none behind a base or a batch item
        self.end = start + size + self.slack


class Layout:
    """where the buffers of `specs` = [(name, stated size), ...] lie, as offsets from an address that is a multiple of BASE_ALIGN.
    alias = {second name: buffer}: two names for one extent (an in-place decode: `out` is `base`); the second name has no region"""

    def __init__(self, specs, alias=None):
        self.bufs, self.by_name = [], {}
        pos = MARGIN
        for name, size in specs:
            a = ALIGN[kind_of(name)]
            pos += ZONE
            if kind_of(name) in ODD:
                start = pos | 1
            elif kind_of(name) in EXACT:                       # the next address = a (mod 2 a): aligned to a, and to nothing more
                start = pos + (a - pos) % (2 * a)
            else:
                start = pos + (-pos) % a
            b = Buf(name, size, start)
            assert name not in self.by_name
            self.bufs.append(b)
            self.by_name[name] = b
            pos = b.end
        for second, name in (alias or {}).items():
            assert second not in self.by_name
            self.by_name[second] = self.by_name[name]
        self.size = pos + MARGIN
        self.regions = []                                      # (lo, hi, text of the place, offset the reported number counts from)
        prev = None
        for b in self.bufs:
            if prev is None:
                self.regions.append((0, b.start, "the front margin (ends %%d bytes before %s)" % b.name, None))
            else:
                self.regions.append((prev.end, b.start, "the guard zone between %s and %s, byte %%d of it" % (prev.name, b.name), prev.end))
            self.regions.append((b.start, b.start + b.size, "%s, byte %%d of its stated %d" % (b.name, b.size), b.start))
            if b.slack:
                self.regions.append((b.start + b.size, b.end, "the slack of %s, stated size + %%d" % b.name, b.start + b.size))
            prev = b
        self.regions.append((prev.end, self.size, "the rear margin, byte %%d behind the slack of %s" % prev.name, prev.end))
        self.starts = np.array([r[0] for r in self.regions], dtype=np.int64)

    def __getitem__(self, name):
        return self.by_name[name]

    def place(self, off):
        """the name of arena offset `off`"""
        lo, hi, text, origin = self.regions[int(np.searchsorted(self.starts, off, side="right")) - 1]
        return text % (hi - off if origin is None else off - origin)


class Arena:
    """the allocation: .buf is the layout's extent (a uint8 tensor on `device`), .image what it held at the last snapshot()"""

    def __init__(self, torch, layout, device, poison, seed, record=None):
        assert poison in POISONS
        self.torch, self.layout, self.poison_kind = torch, layout, poison
        self.record = RECORD if record is None and RECORDING else None if record is False else record   # False: judge, whatever the mode
        whole = torch.empty(layout.size + BASE_ALIGN, dtype=torch.uint8, device=device)
        shift = (-whole.data_ptr()) % BASE_ALIGN
        self.buf = whole[shift:shift + layout.size]
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self._fill(self.buf)
        self.image = None

    def _fill(self, t):
        if self.poison_kind == "ff":
            t.fill_(0xFF)
        else:
            t.random_(0, 256, generator=self.gen)

    def view(self, name, dtype=None):
        """the buffer with its slack"""
        b = self.layout[name]
        t = self.buf[b.start:b.end]
        return t if dtype is None else t.view(dtype)

    def ptr(self, name):
        return self.buf.data_ptr() + self.layout[name].start

    def put(self, name, a):
        """bytes into the front of a buffer's stated extent"""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        b = self.layout[name]
        assert a.size <= b.size, name
        self.buf[b.start:b.start + a.size] = self.torch.from_numpy(a).to(self.buf.device)

    def get(self, name, nbytes):
        b = self.layout[name]
        return self.buf[b.start:b.start + nbytes].cpu().numpy()

    def poison(self, name):
        """fresh poison over a buffer's stated extent: an output about to be written again"""
        b = self.layout[name]
        self._fill(self.buf[b.start:b.start + b.size])

    def snapshot(self):
        if self.image is None:
            self.image = self.buf.clone()
        else:
            self.image.copy_(self.buf)

    def audit(self, tag, writes=(), soft=(), coder=None, allow=None):
        """everything outside `writes` = [(buffer, lo, hi), ...] equals the image.  soft = [(buffer, lo, hi, origin), ...]: writable
        slack -- recorded as furthest offset - origin in recording mode, else open up to origin + allow[(coder, kind)] only"""
        t = self.torch
        if self.buf.is_cuda:
            t.cuda.synchronize()
        diff = self.buf != self.image
        for name, lo, hi in writes:
            s = self.layout[name].start
            if self.record is not None and name.endswith("work") and hi - lo >= 8192:   # how close to its end the workspace is written
                nz = diff[s + hi - 8192:s + hi].nonzero()
                gap = 8191 - int(nz.max()) if nz.numel() else 8192
                key = (coder, name.split(".")[-1] + " unwritten bytes at the end (8192: at least)")
                self.record[key] = min(self.record.get(key, 8192), gap)
            diff[s + lo:s + hi] = False
        allow = ALLOW if allow is None else allow
        for name, lo, hi, origin in soft:
            s = self.layout[name].start
            key = (coder, name.split(".")[-1])
            if self.record is not None:
                nz = diff[s + lo:s + hi].nonzero()
                if nz.numel():
                    self.record[key] = max(self.record.get(key, -1), lo + int(nz.max()) - origin)
                diff[s + lo:s + hi] = False
            elif key in allow:
                diff[s + lo:s + min(hi, origin + allow[key] + 1)] = False
        if diff.any().item():
            raise AssertionError("%s: %s" % (tag, self.describe(diff)))

    def describe(self, diff):
        """the places of the changed bytes: per region the first and the last"""
        idx = diff.nonzero().reshape(-1)
        starts = self.torch.from_numpy(self.layout.starts).to(idx.device)
        reg = self.torch.bucketize(idx, starts, right=True) - 1
        out = []
        regs = self.torch.unique_consecutive(reg).cpu().tolist()
        for r in regs[:6]:
            sel = idx[reg == r]
            first, last = int(sel[0]), int(sel[-1])
            out.append("%d byte(s) changed in %s%s" % (sel.numel(), self.layout.place(first),
                                                       "" if last == first else " .. " + self.layout.place(last)))
        if len(regs) > 6:
            out.append("and %d more places" % (len(regs) - 6))
        return "; ".join(out)

    def call(self, fn, tag, writes=(), soft=(), coder=None, allow=None):
        self.snapshot()
        rc = fn()
        self.audit(tag, writes, soft, coder, allow)
        return rc


# ------------------------------------------------------------------------------------------------------------------ cases ---
class Case:
    """one input of one coder: shape now, bytes and expectation on demand"""

    def __init__(self, codec, n, chunk, tag, ent=None, shape=None):
        self.codec, self.n, self.chunk, self.tag, self.ent, self.shape = codec, n, chunk, tag, ent, shape
        self.name = trc.CODEC_NAMES[codec]
        self.nchunks = trc.nchunks(n, chunk)
        self.static = codec in trc.STATIC
        self.prm = B.prm_of(ent) if ent is not None else None
        self.range = (63, 2) if self.nchunks >= 65 else (0, self.nchunks)
        first, count = self.range
        self.range_bytes = min(n, (first + count) * chunk) - first * chunk
        self._data = None

    def cdfnum(self):
        return trc._cdfnum(self.codec, 256, self.prm or (5, 6))

    def specs(self, rx=True, short=None):
        """(name, stated size) of every buffer of the case; short = {name: bytes}: that buffer DECLARED so much shorter than it
        is and than the library is told (the audit's own test)"""
        lib = trc.lib()
        wb = lib.trc_work_bytes(self.codec, self.n, self.chunk)
        rwb = lib.trc_range_work_bytes(self.codec, self.n, self.chunk, self.range[1])
        assert wb and rwb, self.tag
        s = [("in", self.n), ("a.work", wb), ("a.clen", 4 * self.nchunks), ("a.payload", self.n), ("a.total", 8),
             ("out", self.n), ("range_out", self.range_bytes), ("a.range_work", rwb), ("a.cdf", 2 * (256 + 1)), ("a.status", 4)]
        if self.static:
            s.append(("a.cdfini_work", lib.trc_work_bytes(0, 0, 0)))
        if rx:
            s.append(("b.work", wb))
        return [(name, size - (short or {}).get(name, 0)) for name, size in s]

    def data(self):
        """-> dict: d the input, want what a decoder returns, and either (clen, payload) of the oracle (the coders of
        trc.AVAILABLE; static ones with cdf = (status, cdf)) or the fixture entry's hashes"""
        if self._data is None:
            if self.ent is None:
                n, chunk, d = PM.mixed_input(self.codec, *self.shape)
                assert (n, chunk) == (self.n, self.chunk)
                cdf = T.orc_cdfini(d, 256)[:2] if self.static else None
                payload, clen, _ = T.orc_chunked_enc(self.codec, d, chunk, cdf[1] if cdf else None, 256)
                self._data = dict(d=d, want=d, clen=clen, payload=payload, cdf=cdf)
            else:
                lib_ = S if self.codec in S.FAMILY else B
                d = lib_.build_input(self.codec, self.ent)
                assert d.size == self.n and hashlib.sha256(d.tobytes()).hexdigest() == self.ent["in_sha256"], "the input does not regenerate"
                want = d if self.codec in S.FAMILY else B.expected_of(self.codec, d, self.ent)
                self._data = dict(d=d, want=want, cdf=None)
        return self._data

    def check_encoded(self, clen, payload, total, tag):
        """directory, payload and total against the expectation"""
        x = self.data()
        if self.ent is None:
            msg = PM.first_difference("directory", clen, x["clen"]) or PM.first_difference("payload", payload, x["payload"], clen=x["clen"])
            assert not msg and total == x["payload"].size, "%s: %s (total %d, the oracle has %d)" % (tag, msg, total, x["payload"].size)
        else:
            e = self.ent
            ok = (clen.size == e["nchunks"] and total == payload.size == e["payload_bytes"]
                  and _sha(clen.astype("<u4")) == e["clen_sha256"] and _sha(payload) == e["payload_sha256"])
            assert ok, "%s: lengths / payload differ from the reference (%d bytes, fixture %d)" % (tag, total, e["payload_bytes"])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_gold = {}


def _wave_entries(codec):
    lib_ = S if codec in S.FAMILY else B
    if lib_ not in _gold:
        _gold[lib_] = lib_.load()["codecs"]
    out = []
    for pattern, nch in WAVE_CASES:
        (e,) = [e for e in _gold[lib_][lib_.NAMES[codec]] if e["fam"] == "wave" and not e.get("again")
                and (e["pattern"], e["nchunks"], e["chunk"]) == (pattern, nch, 256)]
        out.append(e)
    return out


def cases_of(codec):
    """the three cases of a coder"""
    name = trc.CODEC_NAMES[codec]
    if codec in trc.AVAILABLE:
        chunk = PM.chunk_of(codec)
        out = []
        for nch, tail in AVAILABLE_SHAPES:
            tail = chunk if tail is None else tail
            out.append(Case(codec, (nch - 1) * chunk + tail, chunk, "%s (%d, %d) chunk %d" % (name, nch, tail, chunk), shape=(nch, tail)))
        return out
    assert codec in S.FAMILY or codec in B.CODECS, codec
    return [Case(codec, e["n"], e["chunk"], "%s wave %s/%d n=%d" % (name, e["pattern"], e["nchunks"], e["n"]), ent=e)
            for e in _wave_entries(codec)]


def mix_of(case):
    """(raw, coded) chunks of the oracle's directory"""
    clen = case.data()["clen"].astype(np.int64)
    lens = S.chunk_lens(case.n, case.chunk)
    return int((clen == lens).sum()), int((clen < lens).sum())


# ------------------------------------------------------------------------------------------------------------- the coder ---
class ArenaCoder(trc.DeviceCoder):
    """a DeviceCoder whose buffers are views of an Arena: work, clen, payload, total, cdf, status and the range workspace of the
    buffers `prefix`.*; rx_of: a decode-only coder with a workspace of its own that shares everything else with that coder"""

    def __init__(self, arena, prefix, case, rx_of=None):
        torch = arena.torch
        self.torch, self.arena, self.prefix = torch, arena, prefix
        self.codec, self.n, self.chunk, self.nch = case.codec, case.n, case.chunk, case.nchunks
        self.dev = arena.buf.device
        self.work_bytes = trc.lib().trc_work_bytes(case.codec, case.n, case.chunk)
        self.work = arena.view(prefix + ".work")
        own = prefix if rx_of is None else rx_of.prefix
        self.clen = arena.view(own + ".clen", torch.int32)
        self.payload = arena.view(own + ".payload")
        self.total = arena.view(own + ".total", torch.int64)
        self.cdf = arena.view(own + ".cdf", torch.int16)
        self.status = arena.view(own + ".status", torch.int32)
        self.cdfini_work = arena.view(own + ".cdfini_work") if case.static else None
        self.cdfnum = rx_of.cdfnum if rx_of is not None else 0
        self.tables_ready = 0
        self.range_tables = 0
        if rx_of is None:
            self.range_work = arena.view(prefix + ".range_work")
            self.range_work_bytes = trc.lib().trc_range_work_bytes(case.codec, case.n, case.chunk, case.range[1])
        else:
            self.range_work, self.range_work_bytes = None, 0

    def cdfini(self, d_in, n, cdfnum, tables=True):
        """trc_cdfini_dev in its own 4096-byte workspace; tables=False leaves trc_tables_dev to the caller (_tables)"""
        trc._chk(trc.lib().trc_cdfini_dev(d_in.data_ptr(), n, self.cdf.data_ptr(), cdfnum, self.status.data_ptr(),
                                          self.cdfini_work.data_ptr(), self._stream()))
        self.cdfnum = cdfnum
        if tables:
            self._tables()


def slack(arena, name):
    """the soft rule of a buffer's whole slack"""
    b = arena.layout[name]
    return (name, b.size, b.size + b.slack, b.size)


def run_case(torch, case, poison, seed, short=None, allow=None, record=None, device="cuda:0"):
    """the sequence of one case under one poison, an audit after every library call -> what the calls returned (directory,
    payload, total, CDF, every decoded output), for the comparison between the two poisons"""
    x = case.data()
    n, chunk, nch, name = case.n, case.chunk, case.nchunks, case.name
    L = Layout(case.specs(short=short))
    A = Arena(torch, L, device, poison, seed, record)
    A.put("in", x["d"])
    d_in = A.view("in")
    dc = ArenaCoder(A, "a", case)
    kw = dict(coder=name, allow=allow)
    tag = "%s, poison %s" % (case.tag, poison)
    prm = {} if case.prm is None else {"prm": case.prm}
    wa, wb_ = L["a.work"].size, L["b.work"].size
    got = {}
    if case.static:                                            # 1. cdfini, then the tables
        A.call(lambda: dc.cdfini(d_in, n, 256, tables=False), tag + ": trc_cdfini_dev",
               [("a.cdf", 0, 2 * 257), ("a.status", 0, 4), ("a.cdfini_work", 0, 4096)],
               [slack(A, "a.status"), slack(A, "a.cdfini_work")], **kw)
        status, cdf = x["cdf"]
        got["status"], got["cdf"] = int(dc.status[0].item()), A.get("a.cdf", 2 * 257).view(np.uint16).copy()
        assert got["status"] == status == n and np.array_equal(got["cdf"], cdf), tag + ": status / CDF of trc_cdfini_dev differ from orc_cdfini"
        A.call(dc._tables, tag + ": trc_tables_dev", [("a.work", 0, wa)], [slack(A, "a.work")], **kw)
    A.snapshot()                                               # 2. encode
    dc.encode(d_in, n, **prm)
    clen, payload = dc.result(n)
    total = int(dc.total[0].item())
    case.check_encoded(clen, payload, total, tag + ": trc_encode_dev")
    A.audit(tag + ": trc_encode_dev", [("a.clen", 0, 4 * nch), ("a.payload", 0, total), ("a.total", 0, 8), ("a.work", 0, wa)],
            [slack(A, "a.clen"), slack(A, "a.total"), slack(A, "a.work"), ("a.payload", total + 64, n + PAD, total)], **kw)
    got.update(clen=clen, payload=payload, total=total, out=[])

    def decoded(what, fn, buf, nbytes, want, writes, soft):
        A.poison(buf)
        A.call(fn, "%s: %s" % (tag, what), [(buf, 0, nbytes)] + writes, soft, **kw)
        out = A.get(buf, nbytes)
        msg = PM.first_difference("decoded bytes", out, want, chunk=chunk)
        assert not msg, "%s: %s: %s" % (tag, what, msg)
        got["out"].append(out)

    out = A.view("out")
    a_work = ([("a.work", 0, wa)], [slack(A, "a.work")])
    decoded("trc_decode_dev", lambda: dc.decode(out, n, **prm), "out", n, x["want"], *a_work)          # 3. decode, twice
    decoded("trc_decode_dev with TRC_DIR_READY", lambda: dc.decode(out, n, dir_ready=True, **prm), "out", n, x["want"], *a_work)
    first, count = case.range                                  # 4. a range, in its own exact-size workspace and output
    rw = L["a.range_work"].size
    decoded("trc_decode_range_dev (%d, %d)" % case.range, lambda: dc.decode_range(A.view("range_out"), first, count, n, **prm),
            "range_out", case.range_bytes, x["want"][first * chunk:first * chunk + case.range_bytes],
            [("a.range_work", 0, rw)], [slack(A, "a.range_work")])
    assert dc.range_work.data_ptr() == A.ptr("a.range_work"), tag + ": the range workspace left the arena"
    rx = ArenaCoder(A, "b", case, rx_of=dc)                    # 5. a workspace that holds poison and has never encoded
    b_work = ([("b.work", 0, wb_)], [slack(A, "b.work")])
    if case.static:
        A.call(rx._tables, tag + ": trc_tables_dev of the decode-only workspace", *b_work, **kw)
    decoded("trc_decode_dev in a decode-only workspace", lambda: rx.decode(out, n, **prm), "out", n, x["want"], *b_work)
    return got


def same_outputs(a, b, tag):
    """what run_case returned under the two poisons is the same: the slack is only read"""
    for k in a:
        xs, ys = (a[k], b[k]) if k == "out" else ([a[k]], [b[k]])
        assert len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys)), "%s: %s differs between the two poisons" % (tag, k)


def refusal_arena(torch, case, device="cuda:0"):
    """the case's buffers without a second workspace, poisoned with 0xFF, the image taken"""
    A = Arena(torch, Layout(case.specs(rx=False)), device, "ff", 0)
    A.snapshot()
    return A
