"""tests/gpu_arena.py without a GPU: the layout arithmetic for every buffer of every case of every coder, the audit on CPU tensors
(one changed byte in each kind of zone is found and named; what a call may write passes; the allow-list opens writable slack up to
its recorded offset and no further), and the raw / coded mix of the oracle's directories for the cases of trc.AVAILABLE."""
import numpy as np
import pytest

import gpu_arena as GA
import planes_matrix_lib as PM
import trc

torch = pytest.importorskip("torch")
by_name = pytest.mark.parametrize("codec", PM.ASSIGNED, ids=lambda c: trc.CODEC_NAMES[c])


def test_every_coder_has_its_cases():
    assert len(PM.ASSIGNED) == 60
    assert sorted(PM.ASSIGNED) == sorted(set(trc.AVAILABLE) | set(GA.S.CODECS) | set(GA.B.CODECS))
    assert len(trc.AVAILABLE) == 27 and len(GA.S.CODECS) == 26 and len(GA.B.CODECS) == 7


@by_name
def test_layout(codec):
    lib = trc.lib()
    cases = GA.cases_of(codec)
    assert [c.nchunks for c in cases] == ([129, 66, 63] if codec in trc.AVAILABLE else [129, 63, 65])
    for case in cases:
        for kw in (dict(), dict(rx=False)):
            specs = case.specs(**kw)
            L = GA.Layout(specs)
            stated = dict(specs)
            assert stated["in"] == stated["out"] == stated["a.payload"] == case.n and stated["a.clen"] == 4 * case.nchunks
            assert stated["a.total"] == 8 and stated["a.status"] == 4 and stated["a.cdf"] == 514
            assert stated["a.work"] == lib.trc_work_bytes(codec, case.n, case.chunk) == stated.get("b.work", stated["a.work"])
            assert stated["a.range_work"] == lib.trc_range_work_bytes(codec, case.n, case.chunk, case.range[1])
            assert stated["range_out"] == case.range_bytes == (case.n - 63 * case.chunk if case.nchunks == 65 else
                                                                 2 * case.chunk if case.nchunks > 65 else case.n)
            assert ("a.cdfini_work" in stated) == (codec in trc.STATIC) and stated.get("a.cdfini_work", 4096) == 4096
            assert [b.name for b in L.bufs] == [s[0] for s in specs]
            assert L.bufs[0].start >= GA.MARGIN + GA.ZONE and L.size - L.bufs[-1].end == GA.MARGIN
            prev_end = None
            for b in L.bufs:
                a = GA.ALIGN[b.kind]
                assert b.size == stated[b.name] and b.end - b.start - b.size == trc.PAD == 256, b.name
                if b.kind in GA.EXACT:
                    assert b.start % (2 * a) == a, "%s: aligned to %d and to nothing more" % (b.name, a)
                else:
                    assert b.kind in ("cdf", "status") and b.start % 256 == 0, b.name
                if prev_end is not None:                       # disjoint, a whole guard zone apart, and no further than the alignment asks
                    assert GA.ZONE <= b.start - prev_end < GA.ZONE + 2 * a, b.name
                prev_end = b.end
            kinds = {b.name: (b.kind, GA.ALIGN[b.kind]) for b in L.bufs}
            assert kinds["in"] == ("in", 16) and kinds["out"] == kinds["range_out"] == ("out", 16) and kinds["a.total"] == ("total", 8)
            assert kinds["a.work"] == kinds["a.range_work"] == ("work", 256) and kinds["a.clen"] == ("clen", 4)
            assert kinds["a.payload"] == ("payload", 2)
            # every byte of the allocation has exactly one name
            assert L.regions[0][0] == 0 and L.regions[-1][1] == L.size
            assert all(r[1] == s[0] and r[0] < r[1] for r, s in zip(L.regions, L.regions[1:]))


def test_arena_views_keep_the_alignment():
    case = GA.cases_of(trc.ANS4S)[1]
    A = GA.Arena(torch, GA.Layout(case.specs()), "cpu", "ff", 0)
    assert A.buf.data_ptr() % GA.BASE_ALIGN == 0 and A.buf.numel() == A.layout.size
    dc = GA.ArenaCoder(A, "a", case)
    rx = GA.ArenaCoder(A, "b", case, rx_of=dc)
    assert dc.work.data_ptr() % 512 == 256 and rx.work.data_ptr() % 512 == 256 and dc.range_work.data_ptr() % 512 == 256
    assert dc.work.data_ptr() != rx.work.data_ptr() and dc.work_bytes == A.layout["a.work"].size
    assert dc.clen.data_ptr() % 8 == 4 and dc.payload.data_ptr() % 4 == 2 and dc.total.data_ptr() % 16 == 8
    assert A.view("in").data_ptr() % 32 == 16 and A.view("out").data_ptr() % 32 == 16 and A.view("range_out").data_ptr() % 32 == 16
    assert dc.cdf.data_ptr() % 256 == 0 and dc.status.data_ptr() % 256 == 0 and dc.cdfini_work.data_ptr() % 512 == 256
    assert rx.clen.data_ptr() == dc.clen.data_ptr() and rx.payload.data_ptr() == dc.payload.data_ptr() and rx.cdf.data_ptr() == dc.cdf.data_ptr()
    assert dc.clen.numel() == case.nchunks + 64 and dc.total.numel() == 33 and dc.payload.numel() == case.n + 256


@pytest.mark.parametrize("poison", GA.POISONS)
def test_poison_and_inputs(poison):
    case = GA.cases_of(trc.RCB)[2]
    L = GA.Layout(case.specs())
    A = GA.Arena(torch, L, "cpu", poison, 3)
    d = case.data()["d"]
    A.put("in", d)
    img = A.buf.numpy()
    b = L["in"]
    assert np.array_equal(img[b.start:b.start + case.n], d)
    rest = np.concatenate([img[:b.start], img[b.start + b.size:]])
    if poison == "ff":
        assert (rest == 0xFF).all()
    else:                                                      # seeded, every byte value, zeros no more often than any other
        assert np.array_equal(A.buf.numpy(), _again(L, d, 3)) and len(np.unique(rest)) == 256
        assert (rest == 0).mean() < 1 / 200


def _again(L, d, seed):
    A = GA.Arena(torch, L, "cpu", "random", seed)
    A.put("in", d)
    return A.buf.numpy()


def test_audit_names_a_changed_byte_in_every_kind_of_zone():
    case = GA.cases_of(trc.RCB)[2]
    L = GA.Layout(case.specs())
    A = GA.Arena(torch, L, "cpu", "random", 11, record=False)
    A.snapshot()
    A.audit("untouched", allow={})
    i, w, o, last = L["in"], L["a.work"], L["out"], L.bufs[-1]
    places = [(0, "the front margin (ends %d bytes before in)" % i.start),
              (i.start - 1, "the front margin (ends 1 bytes before in)"),
              (i.start + 5, "in, byte 5 of its stated %d" % case.n),
              (i.start + i.size, "the slack of in, stated size + 0"),
              (i.end - 1, "the slack of in, stated size + 255"),
              (i.end, "the guard zone between in and a.work, byte 0 of it"),
              (w.start - 1, "the guard zone between in and a.work, byte %d of it" % (w.start - i.end - 1)),
              (w.start + w.size + 3, "the slack of a.work, stated size + 3"),
              (o.start + o.size, "the slack of out, stated size + 0"),
              (last.end, "the rear margin, byte 0 behind the slack of b.work"),
              (L.size - 1, "the rear margin, byte %d behind the slack of b.work" % (GA.MARGIN - 1))]
    for off, text in places:
        A.buf[off] ^= 0x80
        with pytest.raises(AssertionError) as e:
            A.audit("tag", allow={})
        assert str(e.value) == "tag: 1 byte(s) changed in " + text, off
        A.buf[off] ^= 0x80
        A.audit("restored", allow={})
    A.buf[i.start + 5] ^= 1                                     # two places, first and last of each
    A.buf[w.start + w.size + 3] ^= 1
    A.buf[w.start + w.size + 9] ^= 1
    with pytest.raises(AssertionError) as e:
        A.audit("tag", allow={})
    assert str(e.value) == ("tag: 1 byte(s) changed in in, byte 5 of its stated %d; 2 byte(s) changed in the slack of a.work, "
                            "stated size + 3 .. the slack of a.work, stated size + 9" % case.n)


def test_audit_rules():
    """what a call may write passes and nothing next to it; writable slack is open up to the allow-list's offset only; recording
    mode records the furthest offset and judges nothing there, but still judges everything else"""
    case = GA.cases_of(trc.RCB)[2]
    L = GA.Layout(case.specs())
    A = GA.Arena(torch, L, "cpu", "ff", 0, record=False)
    w, p = L["a.work"], L["a.payload"]
    total = 1000
    writes = [("a.work", 0, w.size), ("a.payload", 0, total)]
    soft = [GA.slack(A, "a.work"), ("a.payload", total + 64, case.n + GA.PAD, total)]
    A.snapshot()
    A.buf[w.start:w.start + w.size] = 1
    A.buf[p.start:p.start + total] = 2
    A.audit("allowed", writes, soft, "rcs", {})
    for off, text in ((p.start + total, "a.payload, byte 1000 of its stated"), (p.start + total + 63, "a.payload, byte 1063 of its stated"),
                      (p.start + total + 64, "a.payload, byte 1064"), (p.start + p.size + 255, "the slack of a.payload, stated size + 255"),
                      (p.end, "the guard zone between a.payload and a.total"), (w.start + w.size, "the slack of a.work, stated size + 0")):
        A.buf[off] = 3
        with pytest.raises(AssertionError, match=text.replace("+", r"\+")):
            A.audit("tag", writes, soft, "rcs", {})
        A.buf[off] = 0xFF
    A.buf[w.start + w.size + 15] = 3                            # the allow-list: open up to its offset, for its coder, and no further
    A.buf[p.start + total + 64] = 3
    allow = {("rcs", "work"): 15, ("rcs", "payload"): 64}
    A.audit("listed", writes, soft, "rcs", allow)
    with pytest.raises(AssertionError, match="slack of a.work"):
        A.audit("another coder", writes, soft, "rccdf", allow)
    with pytest.raises(AssertionError, match=r"slack of a.work, stated size \+ 15"):
        A.audit("one less", writes, soft, "rcs", {("rcs", "work"): 14, ("rcs", "payload"): 64})
    with pytest.raises(AssertionError, match="a.payload, byte 1064"):
        A.audit("one less", writes, soft, "rcs", {("rcs", "work"): 15, ("rcs", "payload"): 63})
    rec = {}
    A.record = rec
    A.audit("recording", writes, soft, "rcs", {})
    assert rec[("rcs", "work")] == 15 and rec[("rcs", "payload")] == 64
    A.buf[w.start - 1] = 3
    with pytest.raises(AssertionError, match="guard zone between in and a.work"):
        A.audit("recording still judges the hard rules", writes, soft, "rcs", {})


def test_allow_list_stays_inside_the_slack():
    names = set(trc.CODEC_NAMES.values())
    for (coder, kind), far in GA.ALLOW.items():
        assert coder in names and kind in ("work", "range_work", "cdfini_work", "clen", "total", "status", "payload"), (coder, kind)
        assert 0 <= far < trc.PAD, (coder, kind, far)


@pytest.mark.parametrize("codec", trc.AVAILABLE, ids=lambda c: trc.CODEC_NAMES[c])
def test_raw_and_coded_mix(codec):
    """the mix test_gpu_arena.py asserts holds for the oracle alone: at (129, 100) at least 30 raw and 30 coded chunks, except for
    the three nibble coders, which never store a chunk raw; every case has a ragged or full last chunk as its shape says"""
    cases = GA.cases_of(codec)
    raw, coded = GA.mix_of(cases[0])
    if codec in trc.NIBBLE_CODECS:
        assert (raw, coded) == (0, 129)
    else:
        assert raw >= GA.MIX_MIN and coded >= GA.MIX_MIN and raw + coded == 129, (raw, coded)
    assert [c.n % c.chunk for c in cases] == [100, 37, 0]
    x = cases[1].data()
    assert x["clen"].size == 66 and int(x["clen"].sum()) == x["payload"].size


# ---- the byte-plane calls in the arena (tests/gpu_planes_arena.py) -----------------------------------------------------------
import gpu_planes_arena as P  # noqa: E402

RESIDUE = {"in": (32, 16), "out": (32, 16), "base": (32, 16), "item": (32, 16), "planes": (512, 256), "work": (512, 256), "table": (512, 256),
           "jplanes": (128, 64), "payload": (4, 2), "payload4": (8, 4), "clen": (8, 4), "total": (16, 8), "hist": (16, 8), "fp": (16, 8),
           "cont": (16, 8), "size": (16, 8), "tail": (2, 1), "cdf": (256, 0), "status": (256, 0)}       # kind -> start = r (mod q)
EVERY_KIND = [("in", 1001), ("i0.item", 2), ("i1.item", 512), ("b0.base", 0), ("b1.base", 33), ("planes", 4 * 256), ("work", 4096),
              ("table", 256), ("r0.jplanes", 4 * 256), ("payload", 77), ("c.payload4", 78), ("clen", 12), ("total", 32), ("hist", 3 * 2 * 256 * 8),
              ("fp", 8), ("cont", 1000), ("size", 8), ("tail", 8), ("cdf", 2 * 4 * 264), ("status", 16), ("out", 1001), ("range_out", 24),
              ("range_work", 8192)]


def planes_layouts():
    """(specs, alias) of one layout with every kind and of the layouts of sections A, B and C"""
    yield EVERY_KIND, {"io.out": "b1.base"}
    for fam in P.FLAT_FAMILIES:
        for esize in P.ESIZES:
            for m, t in P.flat_shapes(esize):
                yield P.flat_specs(fam, esize, m, t)
    for case in P.coded_cases():
        yield P.coded(*case).specs()
    for esize in P.ESIZES:
        yield P.hist_order_specs(esize, *P.flat_shapes(esize)[-1]), None
    b = P.Batch("bbatch", 8)
    yield b.item_specs() + b.base_specs() + [("planes", 8 * P.up256(b.M)), ("table", 256)] + b.item_specs("o") + [("r0.jplanes", 8 * 256)], None


def test_planes_layouts():
    """every kind lands at its residue and nowhere better; a base and an item end at start + size, every other buffer TRC_PAD
    later; an alias is a second name of the same buffer and adds no region; no two regions overlap, every byte has one name"""
    count = 0
    for specs, alias in planes_layouts():
        L = GA.Layout(specs, alias)
        count += 1
        assert [b.name for b in L.bufs] == [s[0] for s in specs]
        prev_end = GA.MARGIN
        for b, (name, size) in zip(L.bufs, specs):
            q, r = RESIDUE[b.kind]
            assert b.start % q == r, "%s (%s) at %d: not %d (mod %d)" % (name, b.kind, b.start, r, q)
            assert b.size == size and b.end == b.start + size + (0 if b.kind in ("base", "item") else trc.PAD), name
            assert GA.ZONE <= b.start - prev_end < GA.ZONE + q + (256 if b.kind in ("cdf", "status") else 0), name
            prev_end = b.end
        assert L.size - prev_end == GA.MARGIN
        for second, name in (alias or {}).items():
            assert L[second] is L[name] and second not in [b.name for b in L.bufs] and all(second not in r[2] for r in L.regions)
        assert L.regions[0][0] == 0 and L.regions[-1][1] == L.size
        assert all(r[1] == s[0] and r[0] <= r[1] for r, s in zip(L.regions, L.regions[1:]))
        assert all(r[0] < r[1] or "stated 0" in r[2] for r in L.regions), "an empty region that is not a buffer of 0 bytes"
    assert count > 200
    A = GA.Arena(torch, GA.Layout(EVERY_KIND, {"io.out": "b1.base"}), "cpu", "ff", 0)
    assert A.ptr("tail") % 2 == 1 and A.ptr("cont") % 16 == 8 and A.ptr("r0.jplanes") % 128 == 64 and A.ptr("c.payload4") % 8 == 4
    assert A.ptr("io.out") == A.ptr("b1.base") and A.ptr("b1.base") % 32 == 16 and A.view("b1.base").numel() == 33 and A.view("i0.item").numel() == 2


def test_planes_audit_names_the_byte_behind_an_item_a_pitch_gap_and_the_tail_buffer():
    """what the byte-plane audits rest on, on CPU tensors: with a split's writes permitted ([0, m) of each plane, [0, t) of the
    tail), one changed byte directly behind an item or a base, in a pitch gap and in bytes 1 .. 7 of the tail buffer is named"""
    esize, m, t, pitch = 4, 300, 1, 512
    specs = [("i0.item", 64), ("b0.base", 48), ("planes", esize * pitch), ("tail", 8), ("out", m * esize + t)]
    L = GA.Layout(specs)
    A = GA.Arena(torch, L, "cpu", "random", 2, record=False)
    writes = P.plane_writes("planes", esize, pitch, m) + [("tail", 0, t)]
    A.snapshot()
    for k in range(esize):
        A.buf[L["planes"].start + k * pitch:L["planes"].start + k * pitch + m] ^= 0x11
    A.buf[L["tail"].start] ^= 0x11
    A.audit("a split's own writes", writes, allow={})
    it, ba, pl, tl = L["i0.item"], L["b0.base"], L["planes"], L["tail"]
    assert it.end == it.start + 64 and ba.end == ba.start + 48
    places = [(it.start + 64, "the guard zone between i0.item and b0.base, byte 0 of it"),
              (ba.start + 48, "the guard zone between b0.base and planes, byte 0 of it"),
              (pl.start + m, "planes, byte 300 of its stated 2048"), (pl.start + pitch - 1, "planes, byte 511 of its stated 2048"),
              (pl.start + 3 * pitch + m, "planes, byte %d of its stated 2048" % (3 * pitch + m)),
              (pl.start + esize * pitch, "the slack of planes, stated size + 0")]
    places += [(tl.start + i, "tail, byte %d of its stated 8" % i) for i in range(1, 8)]
    for off, text in places:
        A.buf[off] ^= 0x80
        with pytest.raises(AssertionError) as e:
            A.audit("tag", writes, allow={})
        assert str(e.value) == "tag: 1 byte(s) changed in " + text, off
        A.buf[off] ^= 0x80
    A.audit("restored", writes, allow={})


@pytest.mark.parametrize("case", P.coded_cases(), ids=P.case_id)
def test_coded_planes_inputs_mix_raw_and_coded_chunks(case):
    """for every input of the coded flat calls the oracle alone gives at least one raw and one coded chunk in every plane; the
    call's input is the family's inverse filter of the joined planes"""
    c = P.coded(*case)
    assert c.planes.shape == (c.esize, c.m) and c.n == c.m * c.esize + c.t and c.nc == trc.nchunks(c.m, c.chunk)
    assert (c.nc, c.m % c.chunk, c.t, c.range) in ((66, 37, c.esize - 1, (63, 2)), (3, 3, 0, (0, 1)))
    for k, (raw, coded) in enumerate(c.mix()):
        assert raw >= 1 and coded >= 1 and raw + coded == c.nc, "%s: plane %d has %d raw and %d coded chunks" % (c.tag, k, raw, coded)
    assert np.array_equal(P.PL.split(P.forward(c.model, c.d, c.base, c.esize, c.chunk), c.esize)[0], c.planes)


def test_the_order_family_is_in_every_section_of_the_planes_arena():
    """the flat order calls at the four (order, stride) points, among them the rotating even stride 6; the coded order calls at two,
    for every coder and width the other filtered families have; what each case hands to its C entry point"""
    assert [f[1:] for f in P.FLAT_FAMILIES if f[0] == "ofilter"] == [(2, 1), (3, 3), (2, 6), (3, 8)]
    assert [P.fam_name(f) for f in P.FLAT_FAMILIES if f[0] == "ofilter"][2:] == ["ofilter-o2-s6", "ofilter-o3-s8"]
    cases = [c for c in P.coded_cases() if c[0] == "oplanes"]
    assert len(cases) == 2 * len([c for c in P.coded_cases() if c[0] == "splanes"])
    assert {c[4] for c in cases} == {(2, 3), (3, 8)} and len(set(map(P.case_id, P.coded_cases()))) == len(P.coded_cases())
    for case in cases:
        c = P.coded(*case)
        assert c.model == ("ofilter",) + case[4] and P._lead(c) == case[4] and P._fn(c, ("decode", "_range")) is not None
        assert P.coded(*case) is c
    s = P.coded("splanes", trc.RCA, 4, (3, 3))
    assert (s.order, s.stride, P._lead(s)) == (None, 3, (s.filt, 3))
    assert dict(P.hist_order_specs(4, 9, 3)) == {"in": 39, "hist": trc.lib().trc_planes_hist_order_bytes(4)}


def test_planes_allow_list_stays_inside_the_slack():
    names = set(trc.CODEC_NAMES.values())
    fams = set(P.CODED_FAMILIES) | set(P.BATCH_FAMILIES)
    for (key, kind), far in GA.PLANES_ALLOW.items():
        fam, coder = key.split(":")
        assert fam in fams and coder in names and kind in ("work", "range_work", "clen", "total", "status", "payload", "payload4", "cdf"), (key, kind)
        assert 0 <= far < trc.PAD, (key, kind, far)
