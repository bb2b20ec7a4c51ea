"""What the byte-plane GPU tests share (test_gpu_planes / fplanes / splanes, their _batch files, test_gpu_abatch, test_gpu_advise,
test_gpu_planes_container, test_gpu_planes_matrix, test_gpu_oplanes, test_gpu_planes_restart): the guarded buffers, the packed batch, and the device-check layer of the flat
kernels, the batched kernels, the coded calls and the histograms.  Every function takes the family as data (filt / stride, filters /
strides: None selects the call without them, so each family keeps running its own C entry point), takes its input bytes and the numpy
model's expectation from the caller, and does the device calls and every comparison.  This module is not a test file, so pytest does
not rewrite its asserts: each one carries a message that names the case."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import planes_batch_lib as BL
import planes_lib as PL
import trc
from planes_batch_lib import GUARD, up256  # noqa: F401 (up256: for the test files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRCFILE = os.path.join(ROOT, "harness", "trcfile")
PRM = (4, 7)
CHUNK = 256
E_ARG, E_WORK = -1, -3


# ---- buffers -------------------------------------------------------------------------------------------------------------
class Guarded:
    """a device buffer of nbytes (from `data`, else `fill` throughout) with GUARD bytes of 0xA5 behind it and `front` bytes of 0xA5
    in front (GUARD: a guard on both sides); .t is the buffer itself, .whole the allocation, .img what was uploaded"""

    def __init__(self, torch, nbytes, data=None, fill=0xA5, front=GUARD):
        a = np.full(front + nbytes + GUARD, 0xA5, dtype=np.uint8)
        a[front:front + nbytes] = fill if data is None else data
        self.nbytes, self.front, self.img = nbytes, front, a
        self.whole = torch.from_numpy(a).to("cuda:0")
        self.t = self.whole[front:]
        assert self.t.data_ptr() % 256 == 0, "a fresh device buffer of %d bytes is not 256-byte aligned" % nbytes

    def get(self):
        """-> (the nbytes, True where the guards are intact)"""
        a = self.whole.cpu().numpy()
        f = self.front
        return a[f:f + self.nbytes], bool((a[:f] == 0xA5).all() and (a[f + self.nbytes:] == 0xA5).all())


def guarded(torch, nbytes, data=None, fill=0xA5):
    """the one-sided form: a device tensor of nbytes (from `data`, else `fill` throughout) followed by the guard"""
    return Guarded(torch, nbytes, data, fill, front=0).t


def padded(torch, d):
    """the input on the device with TRC_PAD zero bytes and the guard behind it"""
    return guarded(torch, d.size + trc.PAD, np.concatenate([d, np.zeros(trc.PAD, np.uint8)]))


def first_diff(got, exp):
    return int(np.flatnonzero(got != exp)[0]) if got.shape == exp.shape else -1


class Packed:
    """the items of a batch in one device allocation (BL.offsets / BL.image), or -- data = False -- their places filled with 0xA5"""

    def __init__(self, torch, datas, seed=0, data=True):
        self.torch, self.datas, self.seed = torch, datas, seed
        self.sizes = [d.size for d in datas]
        self.offs, self.total = BL.offsets(self.sizes, seed)
        self.img = BL.image(datas if data else [None] * len(datas), self.offs, self.total)
        self.buf = torch.from_numpy(self.img).to("cuda:0")
        assert self.buf.data_ptr() % 16 == 0, "the packed batch is not 16-byte aligned"

    def views(self, only=None):
        return BL.views(self.buf, self.offs, self.sizes, only)

    def items(self, only=None):
        return trc.planes_items([(v.data_ptr() if v is not None else None, n) for v, n in zip(self.views(only), self.sizes)])

    def expect(self, only=None):
        """the allocation with the items of `only` (default: all) in place and 0xA5 everywhere else"""
        return BL.image([d if only is None or i in only else None for i, d in enumerate(self.datas)], self.offs, self.total)

    def blank(self):
        """the same layout with every item's place filled with 0xA5: where a join or a decode writes"""
        return Packed(self.torch, self.datas, seed=self.seed, data=False)

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.img)


def ranges(count):
    return [(0, 1), (3, 1), (count - 1, 1), (2, 5), (0, count)]


def item_ranges(count, more):
    """every single item, the ranges of `more`, all items"""
    return [(i, 1) for i in range(count)] + list(more) + [(0, count)]


def pad_mask(sizes, esize, chunk, M):
    """True at the elements of V that are pad"""
    _, first = BL.plan(sizes, esize, chunk)
    mask = np.zeros(M, dtype=bool)
    for i, n in enumerate(sizes[:-1]):
        mask[first[i] * chunk + n // esize:first[i + 1] * chunk] = True
    return mask


# ---- the flat kernels ------------------------------------------------------------------------------------------------------
def flat_calls(filt=None, stride=None, seg=None, order=None):
    """-> (split, join) with the family's leading and restart arguments bound: trc.planes_split / join (filt None),
    planes_split_filter / join_filter (stride None), planes_split_sfilter / join_sfilter, planes_split_ofilter / join_ofilter
    (order given, no filt)"""
    if order is not None:
        lead, split, join = (order, stride), trc.planes_split_ofilter, trc.planes_join_ofilter
    elif filt is None:
        return trc.planes_split, trc.planes_join
    else:
        lead = (filt,) if stride is None else (filt, stride)
        split = trc.planes_split_filter if stride is None else trc.planes_split_sfilter
        join = trc.planes_join_filter if stride is None else trc.planes_join_sfilter
    return (lambda d_in, n, esize, d_planes, pitch, d_tail: split(*lead, d_in, n, esize, seg, d_planes, pitch, d_tail),
            lambda d_planes, pitch, d_tail, n, esize, d_out: join(*lead, d_planes, pitch, d_tail, n, esize, seg, d_out))


def split_join_flat(torch, d, esize, m, t, planes, tail, tag, filt=None, stride=None, seg=None, order=None):
    """split d (m elements of esize bytes and t tail bytes) at the smallest pitch the call takes, join the planes again; planes /
    tail: what the model expects.  Compared: the planes with the pitch gaps behind them, the tail, the guards on both sides of all
    four buffers, join(split(x)) == x, the unchanged input"""
    n = d.size
    assert n == m * esize + t, tag + ": %d bytes are not %d elements and %d tail bytes" % (n, m, t)
    pitch = up256(m)
    d_in, d_planes, d_tail, d_out = Guarded(torch, n, d), Guarded(torch, esize * pitch), Guarded(torch, 8), Guarded(torch, n)
    split, join = flat_calls(filt, stride, seg, order)
    split(d_in.t, n, esize, d_planes.t, pitch, d_tail.t if t else None)
    join(d_planes.t, pitch, d_tail.t if t else None, n, esize, d_out.t)
    torch.cuda.synchronize()
    exp = np.full(esize * pitch, 0xA5, dtype=np.uint8)          # (the pitch gap behind m stays as it was)
    for k in range(esize):
        exp[k * pitch:k * pitch + m] = planes[k]
    got, intact = d_planes.get()
    assert np.array_equal(got, exp), tag + ": planes or the gaps behind them (first difference at %d)" % first_diff(got, exp)
    assert intact, tag + ": split wrote outside its planes"
    exp_tail = np.full(8, 0xA5, dtype=np.uint8)
    exp_tail[:t] = tail
    got, intact = d_tail.get()
    assert np.array_equal(got, exp_tail) and intact, tag + ": tail or the bytes around it"
    got, intact = d_out.get()
    assert np.array_equal(got, d), tag + ": join(split(x)) != x (first difference at byte %d)" % first_diff(got, d)
    assert intact, tag + ": join wrote outside its output"
    got, intact = d_in.get()
    assert np.array_equal(got, d) and intact, tag + ": the input changed"


# ---- the batched kernels ---------------------------------------------------------------------------------------------------
def batch_calls(filters=None, strides=None):
    """-> (split, join, the family's arguments between `items` and `count`): the plain, fbatch or sbatch pair"""
    if filters is None and strides is None:
        return trc.planes_split_batch, trc.planes_join_batch, ()
    if strides is None:
        return trc.planes_split_fbatch, trc.planes_join_fbatch, (filters,)
    return trc.planes_split_sbatch, trc.planes_join_sbatch, (filters, strides)


def _of(x, i):
    return 0 if x is None else x if isinstance(x, int) else x[i]


def split_join_batch(torch, datas, esize, chunk, virtual, tag, filters=None, strides=None, partial=True):
    """the items packed with the chunk as seed, split at the smallest pitch the call takes and joined again; virtual: the model's
    (filtered) virtual buffer.  Compared: the plan; the planes with their zero pad and the guard behind them; the untouched input
    and table guard; the whole join from the zero-pad planes and from the same planes with every pad byte 0xFF (what the join
    restores must not depend on the pad), with the item named where it differs; the untouched planes after the joins; and --
    partial -- the join of every range of ranges(count) with NULL pointers outside it"""
    split, join, fam = batch_calls(filters, strides)
    count = len(datas)
    src = Packed(torch, datas, seed=chunk)
    pl, first = BL.plan(src.sizes, esize, chunk)
    got, got_first = trc.planes_batch_plan(src.items(), count, esize, chunk)
    assert got == pl and got_first == first, tag + ": trc_planes_batch_plan gives %r, %r" % (got, got_first)
    M = pl["m_total"]
    pitch = up256(M)                                            # the smallest pitch the call takes
    assert virtual.size == pl["n_virtual"], tag + ": the model's virtual buffer has %d bytes, the plan %d" % (virtual.size, pl["n_virtual"])
    planes, _ = PL.split(virtual, esize)
    tb = trc.lib().trc_planes_batch_table_bytes(count, pl["chunks"])
    d_planes, d_table = guarded(torch, esize * pitch), guarded(torch, tb)
    split(src.items(), *fam, count, esize, chunk, d_planes, pitch, d_table, tb)
    torch.cuda.synchronize()
    exp = np.full(esize * pitch + GUARD, 0xA5, dtype=np.uint8)
    for k in range(esize):
        exp[k * pitch:k * pitch + M] = planes[k]
    got = d_planes.cpu().numpy()
    assert np.array_equal(got, exp), tag + ": planes, their pad zeros or the bytes behind them (first difference at %d)" % first_diff(got, exp)
    assert src.unchanged(), tag + ": split changed its input"
    assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), tag + ": split wrote behind its table"
    loud = exp.copy()
    mask = pad_mask(src.sizes, esize, chunk, M)
    assert int(mask.sum()) == pl["pad_elems"] > 0, tag + ": %d pad elements in the mask, %d in the plan" % (int(mask.sum()), pl["pad_elems"])
    for k in range(esize):
        loud[k * pitch:k * pitch + M][mask] = 0xFF
    d_loud = torch.from_numpy(loud).to("cuda:0")
    # join, whole: every item back, every gap and the guard untouched
    for d_pl, what in ((d_planes, "zero pad"), (d_loud, "0xFF pad")):
        dst = src.blank()
        d_table2 = guarded(torch, tb)
        join(d_pl, 0, pitch, dst.items(), *fam, count, 0, count, esize, chunk, d_table2, tb)
        torch.cuda.synchronize()
        got = dst.buf.cpu().numpy()
        if not np.array_equal(got, src.img):
            at = int(np.argmax(got != src.img))
            i = max(j for j, o in enumerate(src.offs) if o <= at)
            raise AssertionError("%s, %s: join(split(x)) != x, or a gap or the guard was written: byte %d of item %d (%d elements, stride %d, filter %d)"
                                 % (tag, what, at - src.offs[i], i, src.sizes[i] // esize, _of(strides, i) or 1, _of(filters, i)))
        assert (d_table2.cpu().numpy()[tb:] == 0xA5).all(), tag + ", " + what + ": join wrote behind its table"
    assert np.array_equal(d_planes.cpu().numpy(), exp) and np.array_equal(d_loud.cpu().numpy(), loud), tag + ": join changed the planes"
    if not partial:
        return
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        dst = src.blank()
        tbr = trc.lib().trc_planes_batch_table_bytes(ic, first[fi + ic] - first[fi])
        d_table3 = guarded(torch, tbr)
        items = dst.items(only)                                 # NULL outside the range
        assert all((items[i].d_ptr is None) == (i not in only) for i in range(count)), tag + ": the pointers outside (%d, %d) are not NULL" % (fi, ic)
        join(d_loud, first[fi] * chunk, pitch, items, *fam, count, fi, ic, esize, chunk, d_table3, tbr)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), tag + " items (%d, %d)" % (fi, ic)
        assert (d_table3.cpu().numpy()[tbr:] == 0xA5).all(), tag + " items (%d, %d): join wrote behind its table" % (fi, ic)


# ---- the coded calls -------------------------------------------------------------------------------------------------------
_cache = {}


def _key(datas, *rest):
    h = hashlib.sha256()
    for d in datas:
        h.update(b"%d:" % d.size)
        h.update(np.ascontiguousarray(d).tobytes())
    return (h.hexdigest(),) + tuple(tuple(int(v) for v in x) if isinstance(x, (list, tuple, np.ndarray)) else x for x in rest)


def encode_guarded(torch, pc, src, n, tag):
    """src (n bytes) through pc.encode, from an input with TRC_PAD zeros and the guard behind it, into a payload filled with 0x5A:
    no guard of the coder's buffers is touched, the input image is unchanged"""
    d_in = padded(torch, src)
    img = d_in.cpu().numpy()
    pc.payload[:pc.esize * pc.pitch] = 0x5A
    pc.encode(d_in, n)
    assert pc.guards_ok(), tag + ": encode wrote behind one of its buffers"
    assert np.array_equal(d_in.cpu().numpy(), img), tag + ": encode changed its input, the pad or the guard behind it"


def coded_flat(torch, codec, esize, chunk, d, cls=trc.PlanesCoder, model=None, **kw):
    """-> (cls(.., **kw) holding the container of d,) and, where model() gives the model-filtered input, a PlanesCoder holding that
    one's: computed once per (input bytes, codec, esize, chunk, class, arguments), shared, left unchanged"""
    key = _key([d], "flat", codec, esize, chunk, cls.__name__, repr(sorted(kw.items())), model is not None)
    if key not in _cache:
        tag = "%s esize %d chunk %d %s %r" % (trc.CODEC_NAMES[codec], esize, chunk, cls.__name__, kw)
        out = []
        for c, src, ckw in ((cls, d, kw),) + (((trc.PlanesCoder, model(), {}),) if model else ()):
            pc = c(codec, d.size, esize, chunk, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD, **ckw)
            encode_guarded(torch, pc, src, d.size, tag)
            out.append(pc)
        _cache[key] = tuple(out)
    return _cache[key]


def decodes_flat(torch, pc, d, tag):
    n = d.size
    d_out = guarded(torch, n + trc.PAD)
    pc.decode(d_out, n)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:n], d), tag + ": decode does not return the input (first difference at byte %d)" % first_diff(out[:n], d)
    assert (out[n:] == 0xA5).all(), tag + ": decode wrote behind its n bytes"
    assert pc.guards_ok(), tag + ": a guard behind the coder's buffers"


def decodes_ranges_flat(torch, pc, d, esize, chunk, chunk_ranges, tag):
    """every (first, count) of chunk_ranges: the elements of those chunks, nothing behind them"""
    n, m = d.size, d.size // esize
    for first, count in chunk_ranges:
        e0, e1 = first * chunk, min(m, (first + count) * chunk)
        size = (e1 - e0) * esize
        d_out = guarded(torch, size + trc.PAD)
        pc.decode_range(d_out, first, count, n)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:size], d[e0 * esize:e1 * esize]), "%s: chunks (%d, %d)" % (tag, first, count)
        assert (out[size:] == 0xA5).all(), "%s: chunks (%d, %d) wrote behind their elements" % (tag, first, count)
    assert pc.guards_ok(), tag + ": a guard behind the coder's buffers"


def rejected_flat(pc, d_in, d_out, n, nbytes=None, flags=0, **attrs):
    """encode, decode and decode_range with some of the coder's attributes replaced: each is TRC_E_ARG"""
    nbytes = n if nbytes is None else nbytes
    saved = {k: getattr(pc, k) for k in attrs}
    for k, v in attrs.items():
        setattr(pc, k, v)
    try:
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.encode(d_in, nbytes, flags=flags)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.decode(d_out, nbytes, flags=flags)
        with pytest.raises(trc.TrcError, match="rc=-1"):
            pc.decode_range(d_out, 0, 1, nbytes, flags=flags)
    finally:
        for k, v in saved.items():
            setattr(pc, k, v)


def coded_batch(torch, codec, esize, datas, filters=None, strides=None, chunk=CHUNK):
    """-> (Packed source with esize as seed, PlanesBatchCoder holding its coded batch): computed once per (items' bytes, codec, esize,
    chunk, filters, strides), shared, left unchanged"""
    key = _key(datas, "batch", codec, esize, chunk, filters, strides)
    if key not in _cache:
        src = Packed(torch, datas, seed=esize)
        bc = trc.PlanesBatchCoder(codec, src.views(), chunk, cdfnum=256, prm=PRM, guard=GUARD, esize=esize, filters=filters, strides=strides)
        bc.payload[:esize * bc.pitch] = 0x5A
        bc.encode()
        assert bc.guards_ok(), "%s esize %d: encode wrote behind one of its buffers" % (trc.CODEC_NAMES[codec], esize)
        assert src.unchanged(), "%s esize %d: encode changed its input" % (trc.CODEC_NAMES[codec], esize)
        _cache[key] = (src, bc)
    return _cache[key]


def assert_same_outputs(torch, bc, pc, codec, esize, tag):
    """every output of the batch call against the planes call's: directory, totals, payloads, CDFs, statuses"""
    assert (bc.nch, bc.pitch) == (pc.nch, pc.pitch), tag + ": chunks and pitch %r, the planes call %r" % ((bc.nch, bc.pitch), (pc.nch, pc.pitch))
    assert torch.equal(bc.clen[:4 * esize * bc.nch], pc.clen[:4 * esize * pc.nch]), tag + ": d_clen"
    assert torch.equal(bc.total[:8 * esize], pc.total[:8 * esize]), tag + ": d_total"
    for k in range(esize):
        clen, payload, total = bc.result(k)
        exp_clen, exp_payload, exp_total = pc.result(k)
        assert total == exp_total and np.array_equal(clen, exp_clen) and np.array_equal(payload, exp_payload), tag + ": plane %d" % k
    if codec in trc.STATIC:
        assert torch.equal(bc.cdf[:2 * esize * trc.PLANES_CDF_STRIDE], pc.cdf[:2 * esize * trc.PLANES_CDF_STRIDE]), tag + ": d_cdf"
        assert torch.equal(bc.status[:4 * esize], pc.status[:4 * esize]), tag + ": d_status"
        assert all(bc.cdf_of(k)[1] == bc.plan["m_total"] for k in range(esize)), tag + ": a cdfini status is not m_total"


def planes_reference(torch, codec, esize, data, chunk=CHUNK):
    """trc_encode_planes_dev on `data` uploaded as one buffer"""
    pc = trc.PlanesCoder(codec, data.size, esize, chunk, "cuda:0", cdfnum=256, prm=PRM, guard=GUARD)
    pc.encode(padded(torch, data), data.size)
    assert pc.guards_ok(), "%s esize %d: the reference encode wrote behind one of its buffers" % (trc.CODEC_NAMES[codec], esize)
    return pc


def encode_contract_batch(torch, src, bc, codec, esize, virtual, tag):
    """the coded batch is trc_encode_planes_dev on the model's (filtered) virtual buffer, byte for byte; 0x5A behind every payload"""
    assert virtual.size == bc.plan["n_virtual"] and bc.plan["pad_elems"] > 0, tag + ": %d virtual bytes, plan %r" % (virtual.size, bc.plan)
    assert_same_outputs(torch, bc, planes_reference(torch, codec, esize, virtual, bc.chunk), codec, esize, tag)
    for k in range(esize):
        total = bc.result(k)[2]
        assert (bc.payload[k * bc.pitch + total:k * bc.pitch + total + 64].cpu().numpy() == 0x5A).all(), tag + ": bytes behind payload %d" % k


def decodes_whole_batch(torch, src, bc, tag):
    """items [0, count) into a blank copy of the packed source: the source's image"""
    dst = src.blank()
    bc.decode(0, bc.count, out=dst.views())
    torch.cuda.synchronize()
    assert np.array_equal(dst.buf.cpu().numpy(), src.img), tag + ": decode of all items, a gap or the guard"
    assert bc.guards_ok(), tag + ": a guard behind the coder's buffers"


def decode_items_batch(torch, src, bc, codec, esize, tag):
    """every range of ranges(count), each in a fresh workspace of exactly the required size: those items, nothing else"""
    count, L = bc.count, trc.lib()
    for fi, ic in ranges(count):
        only = range(fi, fi + ic)
        dst = src.blank()
        need = L.trc_planes_batch_range_work_bytes(codec, dst.items(only), count, esize, bc.chunk, fi, ic)
        bc.range_work, bc.range_work_bytes = None, 0            # a workspace of exactly that size, guarded, for every range
        bc.decode(fi, ic, out=dst.views(only))
        assert bc.range_work_bytes == need > 0, "%s items (%d, %d): a range workspace of %d bytes, required %d" % (tag, fi, ic, bc.range_work_bytes, need)
        torch.cuda.synchronize()
        assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(only)), "%s items (%d, %d)" % (tag, fi, ic)
        assert bc.guards_ok(), "%s items (%d, %d): a guard behind the coder's buffers" % (tag, fi, ic)
    assert src.unchanged(), tag + ": decode changed the source"


def raw_encode_batch(bc, work_bytes):
    """the family's encode entry point as bc.encode() picks it, on bc's own buffers, with a workspace size of the caller's"""
    st = bc.codec in trc.STATIC
    tail = (bc.count, bc.esize, bc.chunk, bc.cdf.data_ptr() if st else None, bc.cdfnum, bc.status.data_ptr() if st else None, bc.clen.data_ptr(),
            bc.payload.data_ptr(), bc.total.data_ptr(), bc.work.data_ptr(), work_bytes, bc._stream())
    L = trc.lib()
    if bc.filters is None:
        return L.trc_encode_planes_batch_dev(bc.codec, bc.items, *tail)
    if bc.strided():
        return L.trc_encode_splanes_batch_dev(bc.codec, bc.items, bc.filters, bc.strides, *tail)
    return L.trc_encode_fplanes_batch_dev(bc.codec, bc.items, bc.filters, *tail)


def raw_decode_batch(bc, items, fi, ic, d_work, work_bytes):
    """the family's decode entry point as bc.decode() picks it, into `items`, in the workspace given"""
    tail = (bc.count, fi, ic, bc.esize, bc.chunk, bc.cdf.data_ptr() if bc.codec in trc.STATIC else None, bc.cdfnum, d_work.data_ptr(), work_bytes,
            bc._stream())
    L = trc.lib()
    if bc.filters is None:
        return L.trc_decode_planes_batch_dev(bc.codec, bc.clen.data_ptr(), bc.payload.data_ptr(), items, *tail)
    if bc.strided():
        return L.trc_decode_splanes_batch_dev(bc.codec, bc.clen.data_ptr(), bc.payload.data_ptr(), items, bc.filters, bc.strides, *tail)
    return L.trc_decode_fplanes_batch_dev(bc.codec, bc.clen.data_ptr(), bc.payload.data_ptr(), items, bc.filters, *tail)


def workspace_one_byte_short(torch, src, bc, tag):
    """the encode, the decode of all items and of item 3 alone with one byte less than required: TRC_E_WORK, nothing written"""
    L = trc.lib()
    outputs = (bc.clen, bc.payload, bc.total, bc.cdf, bc.status, bc.work)
    before = [x.clone() for x in outputs]
    rc = raw_encode_batch(bc, bc.work_bytes - 1)
    assert rc == E_WORK, tag + ": encode with one byte less returned %d" % rc
    dst = src.blank()
    for fi, ic in ((0, bc.count), (3, 1)):
        need = L.trc_planes_batch_range_work_bytes(bc.codec, dst.items(), bc.count, bc.esize, bc.chunk, fi, ic)
        d_work = guarded(torch, need)
        rc = raw_decode_batch(bc, dst.items(), fi, ic, d_work, need - 1)
        assert rc == E_WORK, "%s: decode of items (%d, %d) with one byte less returned %d" % (tag, fi, ic, rc)
        torch.cuda.synchronize()
        assert (d_work.cpu().numpy() == 0xA5).all(), tag + ": a rejected call wrote to its workspace"
    assert np.array_equal(dst.buf.cpu().numpy(), dst.expect(range(0))), tag + ": a rejected call wrote to an item, a gap or the guard"
    for x, b in zip(outputs, before):
        assert torch.equal(x, b), tag + ": a rejected call changed the coded buffers or the encode workspace"


# ---- host pointers and the harness ---------------------------------------------------------------------------------------------
def host_container_filtered(codec, d, esize, m, chunk, magic, head, encode, check, decode, decode_range, model, more_ranges=lambda c: ()):
    """the TRCF / TRCS container of d: the 16-byte prefix (magic, the bytes `head` at [4:8], the size), bytes [16:] =
    trc_encode_planes_host of model(resolved chunk), the tail, the whole decode and byte ranges around the chunk and element edges,
    a range past the end and a truncated container refused -> (the container, the resolved chunk)"""
    n, t = d.size, d.size - m * esize
    tag = "%s %s chunk %d" % (trc.CODEC_NAMES[codec], magic.decode(), chunk)
    comp = encode(d, chunk)
    check(comp, n)
    assert comp[:4].tobytes() == magic and tuple(comp[4:8]) == tuple(head), tag + ": prefix %r" % (comp[:8].tobytes(),)
    assert int(comp[8:16].view("<u8")[0]) == comp.size, tag + ": the size in the prefix"
    hdr, _, tail = trc.parse_planes(comp[16:])
    resolved = hdr["chunk"]
    assert resolved == (chunk or trc.lib().trc_auto_chunk_codec(codec, m)) and hdr["size"] == comp.size - 16 and hdr["n"] == n, tag + ": header %r" % (hdr,)
    exp = trc.host_encode_planes(codec, model(resolved), esize, chunk)
    assert np.array_equal(comp[16:], exp), tag + ": bytes [16:] are not trc_encode_planes_host of the filtered input"
    assert np.array_equal(tail, d[n - t:]), tag + ": the tail bytes"
    assert np.array_equal(decode(comp, n), d), tag + ": the whole decode"
    c = resolved * esize
    for offset, length in [(0, 1), (c - 1, 3), (c // 2, 2 * c)] + list(more_ranges(c)) + [(5, n - 5), (n - t - 1, t + 1), (n - t, t), (n - 1, 1), (0, n)]:
        if offset + length > n:
            continue
        got = decode_range(comp, offset, length)
        assert np.array_equal(got, d[offset:offset + length]), tag + ": bytes [%d, +%d)" % (offset, length)
    with pytest.raises(trc.TrcError):
        decode_range(comp, n - 1, 2)
    with pytest.raises(trc.TrcError, match="container"):
        decode(comp[:-1], n)
    return comp, resolved


def trcfile(*args, rc=0):
    """harness/trcfile with these arguments: exit code rc -> the finished process"""
    assert os.path.exists(TRCFILE), "harness/trcfile is not built"
    r = subprocess.run([TRCFILE] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == rc, (args, r.stdout, r.stderr)
    return r


def trcfile_round_trip(tmp_path, d, ext, encode_args, offset, length):
    """d through `trcfile <encode_args> in out`, `d` and `x offset length`: the decoded file and the byte range are d's -> the
    container's bytes"""
    src, comp, back, part = (str(tmp_path / f) for f in ("in.bin", "in." + ext, "out.bin", "part.bin"))
    d.tofile(src)
    trcfile(*encode_args, src, comp)
    trcfile("d", comp, back)
    trcfile("x", comp, offset, length, part)
    assert np.array_equal(np.fromfile(back, dtype=np.uint8), d), "trcfile %r: the decoded file" % (encode_args,)
    assert np.array_equal(np.fromfile(part, dtype=np.uint8), d[offset:offset + length]), "trcfile %r: bytes [%d, +%d)" % (encode_args, offset, length)
    return np.fromfile(comp, dtype=np.uint8)


# ---- the histograms --------------------------------------------------------------------------------------------------------
def device_hists(torch, esize, seg, filters, d=None, src=None, strides=None, fi=0, ic=None, null_outside=False, d_hist=None):
    """one histogram call into a buffer guarded on both sides (given, or fresh and dirty) -> (uint64 [items, 3, esize, 256], the
    buffer).  d: the flat call on these bytes, uploaded between guards (trc_planes_hist_dev; strides an int:
    trc_planes_hist_stride_dev) -- one item.  src: items [fi, fi + ic) of that Packed batch with a guarded table of exactly the
    range's size (trc_planes_hist_batch_dev; strides a list: trc_planes_hist_sbatch_dev), null_outside: every pointer outside
    the range NULL.  Checks the guards of the histograms and the table, and that the input, its gaps and its guards are unchanged"""
    what = "esize %d seg %d filters %d strides %r" % (esize, seg, filters, strides)
    if d is not None:
        ic, n = 1, d.size
        hb = trc.planes_hist_bytes(esize)
        d_hist = Guarded(torch, hb) if d_hist is None else d_hist
        d_in = Guarded(torch, n, d)
        if strides is None:
            trc.planes_hist(filters, d_in.t, n, esize, seg, d_hist.t)
        else:
            trc.planes_hist_stride(filters, strides, d_in.t, n, esize, seg, d_hist.t)
        torch.cuda.synchronize()
        back, intact = d_in.get()
        assert np.array_equal(back, d) and intact, what + ": the call changed its input or the bytes around it"
    else:
        count = len(src.sizes)
        ic = count - fi if ic is None else ic
        _, first = BL.plan(src.sizes, esize, seg)
        tb = trc.lib().trc_planes_batch_table_bytes(ic, first[fi + ic] - first[fi])
        hb = trc.planes_hist_batch_bytes(ic, esize)
        assert hb == ic * trc.planes_hist_bytes(esize) and (tb > 0) == (ic > 0), what + ": %d histogram bytes, %d table bytes for %d items" % (hb, tb, ic)
        d_hist = Guarded(torch, hb) if d_hist is None else d_hist
        d_table = guarded(torch, tb)
        items = src.items(range(fi, fi + ic)) if null_outside else src.items()
        if strides is None:
            trc.planes_hist_batch(filters, items, count, fi, ic, esize, seg, d_hist.t, d_table, tb)
        else:
            trc.planes_hist_sbatch(filters, items, strides, count, fi, ic, esize, seg, d_hist.t, d_table, tb)
        torch.cuda.synchronize()
        assert (d_table.cpu().numpy()[tb:] == 0xA5).all(), what + ": the call wrote behind its table"
        assert src.unchanged(), what + ": the call changed its input, a gap or the guard"
    raw = d_hist.whole.cpu().numpy()
    f = d_hist.front
    assert (raw[:f] == 0xA5).all() and (raw[f + hb:] == 0xA5).all(), what + ": the call wrote outside the histograms of its range"
    return raw[f:f + hb].view("<u8").reshape(ic, 3, esize, 256).copy(), d_hist


def device_order_hists(torch, d, esize, stride, seg, orders):
    """trc_planes_hist_order_dev into a dirty buffer guarded on both sides -> uint64 [4 * esize * 256]; the input and every guard
    are unchanged"""
    n, hb = d.size, trc.planes_hist_order_bytes(esize)
    assert hb == 4 * esize * 256 * 8, "trc_planes_hist_order_bytes(%d) is %d" % (esize, hb)
    d_in, d_hist = Guarded(torch, n, d), Guarded(torch, hb)
    trc.planes_hist_order(orders, stride, d_in.t, n, esize, seg, d_hist.t)
    torch.cuda.synchronize()
    back, intact = d_in.get()
    assert np.array_equal(back, d) and intact, "orders %d stride %d: the call changed its input or the bytes around it" % (orders, stride)
    got, intact = d_hist.get()
    assert intact, "orders %d stride %d: the call wrote outside its histograms" % (orders, stride)
    return got.view("<u8").copy()


def assert_order_hists(got, exp, m, orders, tag):
    """got, exp: uint64 [4, esize, 256].  A requested order's rows sum to m and equal the model's, the first differing bin named; the
    rows of an order that was not requested are zero"""
    for k in range(4):
        if orders >> k & 1:
            assert (got[k].sum(axis=1) == m).all(), tag + ": a row of order %d does not sum to m" % k
            if not np.array_equal(got[k], exp[k]):
                p, b = np.argwhere(got[k] != exp[k])[0]
                raise AssertionError("%s: order %d plane %d bin %d: %d, the model has %d" % (tag, k, p, b, got[k, p, b], exp[k, p, b]))
        else:
            assert not got[k].any(), tag + ": rows of order %d, which was not requested, are not zero" % k


def assert_hists(got, exp, ms, filters, tag):
    """got, exp: uint64 [items, 3, esize, 256]; ms: elements per item.  A requested filter's rows sum to m and equal the model's,
    the first differing bin named; the rows of a filter that was not requested are zero"""
    exp = np.asarray(exp).reshape((len(ms), 3) + got.shape[2:])
    assert got.shape == exp.shape, tag + ": %r histograms, the model has %r" % (got.shape, exp.shape)
    for i, m in enumerate(ms):
        for f in range(3):
            if filters >> f & 1:
                assert (got[i, f].sum(axis=1) == m).all(), "%s: item %d (%d elements): a row of filter %d does not sum to m" % (tag, i, m, f)
                if not np.array_equal(got[i, f], exp[i, f]):
                    k, b = np.argwhere(got[i, f] != exp[i, f])[0]
                    raise AssertionError("%s: item %d (%d elements) filter %d plane %d bin %d: %d, the model has %d"
                                         % (tag, i, m, f, k, b, got[i, f, k, b], exp[i, f, k, b]))
            else:
                assert not got[i, f].any(), "%s: item %d: rows of filter %d, which was not requested, are not zero" % (tag, i, f)
