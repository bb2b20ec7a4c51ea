// trc_planes_container.inc -- the TRCB container of a coded batch (included by trc_api.hip behind trc_planes_batch.inc): the
// host-only layout, bound and check, the pack call around the kernel of trc_planes_pack.hip, the decode of a packed container where it
// lies in device memory, and the host-pointer calls on top of them.
//
//   trc_planes_batch_hdr (48 B) | uint64 n[count] | uint8 filter[count], zero-padded to a multiple of 8 | inner
//   inner = the TRCP container of VF(items, filters, esize, chunk), byte for byte what planes_host_encode writes for it
#include "trc_planes_pack.h"

static inline size_t batch_front_bytes(size_t count) { return sizeof(trc_planes_batch_hdr) + 8 * count + up8(count); }
static inline const uint8_t *batch_filters(const void *trcb, size_t count) { return (const uint8_t *)trcb + sizeof(trc_planes_batch_hdr) + 8 * count; }

// chunk 0 -> the automatic chunk, a chunk above the coder's largest -> that one: what planes_host_encode does for n = sum n[i].
// 0 for a batch whose sizes cannot be added up (the plan says why).
static uint32_t batch_resolve_chunk(const TrcCodec &r, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    if (!chunk) {
        if (!items || !count || count > TRC_PLANES_BATCH_MAX || !planes_esize_ok(esize)) return 0;
        uint64_t m = 0;
        for (size_t i = 0; i < count; i++) {
            if (items[i].n < esize || items[i].n % esize || items[i].n / esize > ((uint64_t)1 << 62) - m) return 0;
            m += items[i].n / esize;
        }
        chunk = trc_auto_chunk_codec(r.id, (size_t)m);
        if (chunk < r.floor) chunk = r.floor;
    }
    if (chunk_ok(chunk) && chunk > r.chunk_max) chunk = r.chunk_max;
    return chunk;
}

extern "C" uint32_t trc_planes_batch_auto_chunk(int codec, const trc_planes_item *items, size_t count, unsigned esize)
{
    const TrcCodec &r = codec_row(codec);
    if (!r.enc || r.low4) return 0;
    return batch_resolve_chunk(r, items, count, esize, 0);
}

// the batch as the container calls see it: the resolved chunk, the plan, cdfnum as the header carries it; false for what they reject
struct BatchShape { uint32_t chunk; unsigned cdfnum; trc_planes_batch_plan B; };
static bool batch_shape(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, BatchShape &S)
{
    const TrcCodec &r = codec_row(codec);
    if (!r.enc || r.low4) return false;
    S.chunk = batch_resolve_chunk(r, items, count, esize, chunk);
    if (!S.chunk || trc_planes_batch_plan_quiet(items, count, esize, S.chunk, &S.B, nullptr)) return false;
    PlanesMap P;
    if (!planes_map(codec, (size_t)S.B.n_virtual, esize, S.chunk, P)) return false;
    S.cdfnum = r.cdf || r.ss ? cdfnum : 0;
    if (r.cdf && (cdfnum < 1 || cdfnum > 256)) return false;
    if (r.ss && !ss_prm_ok(cdfnum)) return false;
    return true;
}

extern "C" size_t trc_planes_batch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    BatchShape S;
    if (!batch_shape(codec, items, count, esize, chunk, cdfnum, S)) return 0;
    return batch_front_bytes(count) + trc_planes_bound((size_t)S.B.n_virtual, esize, S.chunk, S.cdfnum) + TRC_PAD;
}

extern "C" int trc_planes_batch_layout_host(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                            unsigned cdfnum, const uint64_t *total, trc_planes_batch_layout *L)
{
    BatchShape S;
    if (!total || !L) return fail(TRC_E_ARG, "planes_batch_layout: null totals or layout");
    if (!batch_shape(codec, items, count, esize, chunk, cdfnum, S)) return fail(TRC_E_ARG, "planes_batch_layout: bad (codec, items, esize, chunk, cdfnum)");
    const size_t cdfb = planes_cdf_bytes(codec_row(codec), S.cdfnum);
    memset(L, 0, sizeof *L);
    L->inner = batch_front_bytes(count);
    uint64_t pos = sizeof(trc_planes_hdr) + 8 * (uint64_t)esize;
    for (unsigned k = 0; k < esize; k++) {
        if (total[k] > S.B.m_total) return fail(TRC_E_ARG, "planes_batch_layout: plane %u states %llu payload bytes of %llu", k, (unsigned long long)total[k], (unsigned long long)S.B.m_total);
        L->off[k] = L->inner + pos;
        pos = up8((size_t)(pos + cdfb + sizeof(trc_container_hdr) + 4 * S.B.chunks + total[k]));
    }
    L->size = L->inner + pos;
    return TRC_OK;
}

// the verdict and, where it is good, the header
static int batch_verdict(const void *buf, size_t buflen, size_t count_expected, trc_planes_batch_hdr &h, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, "batch container: " __VA_ARGS__); return TRC_E_ARG; } while (0)
    if (!buf || buflen < sizeof h) BAD("%zu bytes is shorter than the header", buflen);
    memcpy(&h, buf, sizeof h);
    if (h.magic != TRC_PLANES_BATCH_MAGIC) BAD("bad magic 0x%08x", h.magic);
    if (h.version != 1) BAD("version %u (1)", h.version);
    if (h.zero || h.zero2) BAD("reserved fields are 0x%x / 0x%x, must be 0", h.zero, h.zero2);
    if (!planes_esize_ok(h.esize)) BAD("esize %u (2, 4 or 8)", h.esize);
    if (!chunk_ok(h.chunk)) BAD("chunk %u", h.chunk);
    if (h.count < 1 || h.count > TRC_PLANES_BATCH_MAX) BAD("%llu items (1 .. %u)", (unsigned long long)h.count, TRC_PLANES_BATCH_MAX);
    if (count_expected != (size_t)-1 && h.count != count_expected) BAD("holds %llu items, caller expects %zu", (unsigned long long)h.count, count_expected);
    const size_t count = (size_t)h.count, front = batch_front_bytes(count);
    if (h.inner != front) BAD("inner offset %llu, %zu items put it at %zu", (unsigned long long)h.inner, count, front);
    if (h.size > buflen) BAD("states %llu bytes, the buffer holds %zu", (unsigned long long)h.size, buflen);
    if (h.size <= h.inner) BAD("size %llu leaves no room behind the item table", (unsigned long long)h.size);
    const uint8_t *b = (const uint8_t *)buf, *fl = b + sizeof h + 8 * count;
    uint64_t bytes = 0, nc = 0, last_nc = 0, last_m = 0;
    for (size_t i = 0; i < count; i++) {
        uint64_t n;
        memcpy(&n, b + sizeof h + 8 * i, 8);
        if (n < h.esize || n % h.esize) BAD("item %zu has %llu bytes: not a whole number (at least one) of %u-byte elements", i, (unsigned long long)n, h.esize);
        if (n > ~bytes) BAD("item %zu: the sizes overflow", i);
        bytes += n;
        last_m = n / h.esize;
        last_nc = (last_m + h.chunk - 1) / h.chunk;
        nc += last_nc;
        if (nc > 0x7fffffffu) BAD("item %zu: too many chunks", i);
    }
    for (size_t i = 0; i < count; i++) if (fl[i] > TRC_FILTER_XOR) BAD("item %zu: filter %u (0 none, 1 zigzag delta, 2 xor)", i, (unsigned)fl[i]);
    for (size_t i = count; i < up8(count); i++) if (fl[i]) BAD("the filter padding must be zero bytes");
    if (h.bytes != bytes) BAD("bytes %llu, the items add up to %llu", (unsigned long long)h.bytes, (unsigned long long)bytes);
    const uint64_t M = (nc - last_nc) * h.chunk + last_m;
    trc_planes_hdr p;
    char sub[320];
    if (planes_verdict(b + front, (size_t)h.size - front, (size_t)(M * h.esize), p, sub, sizeof sub)) BAD("%s", sub);
    if (p.esize != h.esize || p.chunk != h.chunk) BAD("the inner container's esize %u / chunk %u differ from the header's", p.esize, p.chunk);
    if (p.tail) BAD("the inner container has %u tail bytes: a batch has whole elements only", p.tail);
    if (p.size != h.size - front) BAD("the inner container states %llu bytes of %llu", (unsigned long long)p.size, (unsigned long long)(h.size - front));
    return TRC_OK;
#undef BAD
}
extern "C" int trc_planes_batch_check(const void *buf, size_t buflen, size_t count_expected)
{
    trc_planes_batch_hdr h;
    char why[400];
    return batch_verdict(buf, buflen, count_expected, h, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}
extern "C" int trc_planes_batch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, size_t cap)
{
    trc_planes_batch_hdr hh;
    char why[400];
    if (!h) return fail(TRC_E_ARG, "planes_batch_info: null header");
    if (batch_verdict(buf, buflen, (size_t)-1, hh, why, sizeof why)) return fail(TRC_E_ARG, "%s", why);
    *h = hh;
    const size_t cnt = cap < hh.count ? cap : (size_t)hh.count;
    const uint8_t *b = (const uint8_t *)buf;
    if (n) memcpy(n, b + sizeof hh, 8 * cnt);
    if (filters) memcpy(filters, b + sizeof hh + 8 * (size_t)hh.count, cnt);
    return TRC_OK;
}

// ---- the pack call ------------------------------------------------------------------------------------------------------------------
// what pack and the packed decode check between the filters and the buffers (planes_common without a workspace)
static int container_common(const char *who, int codec, unsigned esize)
{
    if (codec & (TRC_TABLES_READY | TRC_DIR_READY)) return fail(TRC_E_ARG, "%s: TRC_TABLES_READY / TRC_DIR_READY do not apply to planes", who);
    if (codec_row(codec).low4) return fail(TRC_E_ARG, "%s: " PLANES_LOW4, who, codec);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "%s: esize %u (2, 4 or 8)", who, esize);
    return TRC_OK;
}

extern "C" int trc_planes_batch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, size_t count,
                                         unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                         const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                                         const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream)
{
    const char *who = "planes_batch_pack";
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, filters, count, nullptr))) return rc;
    if ((rc = container_common(who, codec, esize))) return rc;
    if ((rc = check_common(codec, (size_t)B.m_total, chunk, d_cdf, cdfnum))) return rc;
    const TrcCodec &r = codec_row(codec);
    if (r.cdf && !d_status) return fail(TRC_E_ARG, "%s: a static coder needs d_status (one int32 per plane)", who);
    if (!r.cdf && d_status) return fail(TRC_E_ARG, "%s: codec %d builds no CDF: d_status must be NULL", who, codec);
    if (!r.cdf && !r.ss) cdfnum = 0;
    if (!d_clen || !d_payload || !d_total || ((uintptr_t)d_payload & 3) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_total & 7))
        return fail(TRC_E_ARG, "%s: d_clen and d_payload must be 4-byte, d_total 8-byte aligned", who);
    if (!d_out || !d_size || ((uintptr_t)d_out & 15) || ((uintptr_t)d_size & 7)) return fail(TRC_E_ARG, "%s: d_out must be 16-byte, d_size 8-byte aligned", who);
    const size_t bound = trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
    if (!bound) return fail(TRC_E_ARG, "%s: bad (codec, items, esize, chunk, cdfnum)", who);
    if (out_bytes < bound) return fail(TRC_E_WORK, "%s: d_out holds %zu B < required %zu B (trc_planes_batch_bound)", who, out_bytes, bound);

    // the front: everything the host knows -- the header with its size still open, n[], the filters and their zero padding
    const size_t front = batch_front_bytes(count);
    std::vector<uint8_t> f(front, 0);
    trc_planes_batch_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_PLANES_BATCH_MAGIC; h.version = 1; h.esize = (uint8_t)esize; h.chunk = chunk; h.count = count; h.inner = front;
    for (size_t i = 0; i < count; i++) {
        h.bytes += items[i].n;
        memcpy(f.data() + sizeof h + 8 * i, &items[i].n, 8);
    }
    memcpy(f.data(), &h, sizeof h);
    if (filters) memcpy(f.data() + sizeof h + 8 * count, filters, count);
    hipStream_t s = (hipStream_t)stream;
    // (the host arrays are free again when this returns: the copy waits for the stream, as the batched calls' table upload does)
    const hipError_t e = hipMemcpyWithStream(d_out, f.data(), front, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(TRC_E_HIP, "%s: front upload: %s", who, hipGetErrorString(e));

    PackArgs a;
    memset(&a, 0, sizeof a);
    a.out = (uint8_t *)d_out; a.inner = front;
    a.clen = d_clen; a.payload = (const uint8_t *)d_payload; a.total = d_total;
    a.cdf = r.cdf ? d_cdf : nullptr; a.status = r.cdf ? d_status : nullptr; a.d_size = d_size;
    a.M = B.m_total; a.NC = B.chunks; a.pitch = B.pitch; a.esize = esize;
    a.cdfb = (uint32_t)planes_cdf_bytes(r, cdfnum); a.cdf_used = r.cdf ? 2 * (cdfnum + 1) : 0;
    trc_planes_hdr ph;
    memset(&ph, 0, sizeof ph);
    ph.magic = TRC_PLANES_MAGIC; ph.codec = (uint8_t)codec; ph.version = 1; ph.esize = (uint8_t)esize;
    ph.chunk = chunk; ph.cdfnum = cdfnum; ph.n = B.n_virtual;
    trc_container_hdr sh;
    memset(&sh, 0, sizeof sh);
    sh.magic = TRC_MAGIC; sh.codec = (uint8_t)codec; sh.version = 1; sh.cdfnum = (uint16_t)cdfnum;
    sh.chunk = chunk; sh.nchunks = (uint32_t)B.chunks; sh.n = B.m_total;
    static_assert(sizeof ph == sizeof a.ph && sizeof sh == sizeof a.sh, "the headers travel as four words each");
    memcpy(a.ph, &ph, sizeof ph);
    memcpy(a.sh, &sh, sizeof sh);
    return trc_planes_pack_launch(a, s);
}

// ---- decoding a packed container where it lies ------------------------------------------------------------------------------------
// both packed decoders: d_cont = the TRCB container, `lead` bytes into the buffer of cont_bytes the caller named (the TRCT prefix, or 0)
static int packed_decode(const char *who, int codec, const void *d_cont, size_t lead, size_t cont_bytes,
                         const trc_planes_item *items, const BatchPred pred, size_t count, size_t first_item, size_t item_count,
                         unsigned esize, uint32_t chunk, unsigned cdfnum, const uint64_t *total,
                         void *d_work, size_t work_bytes, void *stream)
{
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, pred.filters, count, nullptr))) return rc;
    if ((rc = trc_planes_batch_strides(who, pred.filters, pred.strides, count, nullptr))) return rc;
    if ((rc = trc_planes_batch_orders(who, pred.filters, pred.orders, count, nullptr))) return rc;
    if ((rc = container_common(who, codec & ~(TRC_TABLES_READY | TRC_DIR_READY), esize))) return rc;
    if (!d_cont || ((uintptr_t)d_cont & 7) || !total) return fail(TRC_E_ARG, "%s: d_cont must be 8-byte aligned, total a host array of %u entries", who, esize);
    const TrcCodec &r = codec_row(codec);
    trc_planes_batch_layout L;
    if ((rc = trc_planes_batch_layout_host(codec, items, count, esize, chunk, cdfnum, total, &L))) return rc;
    if (lead + L.size > cont_bytes) return fail(TRC_E_ARG, "%s: the container has %llu bytes, d_cont holds %zu", who, (unsigned long long)(lead + L.size), cont_bytes);
    const size_t cdfb = planes_cdf_bytes(r, r.cdf || r.ss ? cdfnum : 0);
    BatchCoded S;
    memset(&S, 0, sizeof S);
    for (unsigned k = 0; k < esize; k++) {
        const uint8_t *sec = (const uint8_t *)d_cont + L.off[k];
        S.cdf[k] = r.cdf ? (const uint16_t *)sec : nullptr;
        S.clen[k] = (const uint32_t *)(sec + cdfb + sizeof(trc_container_hdr));
        S.payload[k] = sec + cdfb + sizeof(trc_container_hdr) + 4 * (size_t)B.chunks;
    }
    return decode_batch(who, codec, S, 0, items, pred, count, first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}
extern "C" int trc_decode_planes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                                  const trc_planes_item *items, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                                  unsigned esize, uint32_t chunk, unsigned cdfnum, const uint64_t *total,
                                                  void *d_work, size_t work_bytes, void *stream)
{
    return packed_decode("decode_planes_batch_packed", codec, d_cont, 0, cont_bytes, items, batch_pred_strides(filters, nullptr), count, first_item, item_count,
                         esize, chunk, cdfnum, total, d_work, work_bytes, stream);
}

// ---- host pointers: the plain single-device context of planes_host_encode, no striping ----------------------------------------------
//   d_small (trc_planes.inc): CDFs | totals | statuses | tail bytes; behind them the packed container's size
#define BATCH_SMALL_SIZE (PLANES_SMALL_TAIL + 64)
#define BCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail(TRC_E_HIP, "%s -> %s", #x, hipGetErrorString(e_)); (void)hipStreamSynchronize(s); return 0; } } while (0)
static inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Host items to d_dst (c.d_in, or c.d_base for the bases of a batch), item i at offset off[i] (multiples of 16, increasing).  A pageable hipMemcpyAsync per item costs the
// runtime's staging and a round of its bookkeeping per call, whatever the item's size (profiles/planes/container_notes.md), so the
// items are gathered into the context's page-locked staging slots at the same mutual offsets and a slot is sent when the next
// item does not fit: one copy per slot's worth.  An item larger than a slot goes by a copy of its own.
static int batch_items_up(HostCtx &c, hipStream_t s, uint8_t *d_dst, const trc_planes_item *items, size_t count, const std::vector<size_t> &off)
{
    if (grow_pins(c, true)) return TRC_E_HIP;
    const size_t cap = c.cap_pin;
    int slot = 0;
    bool used[TRC_NSLOT] = {};
    size_t base = 0, fill = 0;                     // the slot holds device bytes [base, base + fill)
    auto flush = [&]() -> int {
        if (!fill) return TRC_OK;
        HIPCHK(hipMemcpyAsync(d_dst + base, c.pin_in[slot], fill, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c.ev_in[slot], s));
        used[slot] = true;
        slot = (slot + 1) % TRC_NSLOT;
        fill = 0;
        if (used[slot]) HIPCHK(hipEventSynchronize(c.ev_in[slot]));
        return TRC_OK;
    };
    for (size_t i = 0; i < count; i++) {
        const size_t n = (size_t)items[i].n;
        if (n > cap) {
            if (flush()) return TRC_E_HIP;
            HIPCHK(hipMemcpyAsync(d_dst + off[i], items[i].d_ptr, n, hipMemcpyHostToDevice, s));
            continue;
        }
        if (fill && off[i] + n - base > cap && flush()) return TRC_E_HIP;
        if (!fill) base = off[i];
        if (off[i] - base > fill) memset(c.pin_in[slot] + fill, 0, off[i] - base - fill);
        memcpy(c.pin_in[slot] + (off[i] - base), items[i].d_ptr, n);
        fill = off[i] - base + n;
    }
    return flush();
}

// The bases of items [first_item, first_item + item_count) that want[i] asks for, to c.d_base (host bases) -> dev[i], NULL elsewhere.
// items_on == TRC_ITEMS_DEV: the caller's pointers as they are.  The staging slots are the items': the stream is drained first.
static int batch_bases_up(HostCtx &c, hipStream_t s, const trc_planes_item *items, const void *const *bases, const std::vector<bool> &want,
                          size_t count, size_t first_item, size_t item_count, int items_on, std::vector<const void *> &dev)
{
    dev.assign(count, nullptr);
    std::vector<trc_planes_item> up;
    std::vector<size_t> off, idx;
    size_t pos = 0;
    for (size_t i = first_item; i < first_item + item_count; i++) {
        if (!want[i]) continue;
        if (items_on == TRC_ITEMS_DEV) { dev[i] = bases[i]; continue; }
        up.push_back(trc_planes_item{ const_cast<void *>(bases[i]), items[i].n });
        off.push_back(pos);
        idx.push_back(i);
        pos += up16((size_t)items[i].n);
    }
    if (up.empty()) return TRC_OK;
    if (grow(&c.d_base, &c.cap_base, pos)) return TRC_E_HIP;
    HIPCHK(hipStreamSynchronize(s));
    if (batch_items_up(c, s, c.d_base, up.data(), up.size(), off)) return TRC_E_HIP;
    for (size_t k = 0; k < idx.size(); k++) dev[idx[k]] = c.d_base + off[k];
    return TRC_OK;
}
extern "C" size_t trc_planes_bbatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum);      // trc_planes_bcontainer.inc

// strides given: the TRCT container (trc_encode_splanes_batch_host); it refuses a batch that is a TRCB container's.
// based: the TRCE container (trc_encode_bplanes_batch_host, trc_planes_bcontainer.inc), the bases lying where the items lie; it refuses an
// all-NONE batch likewise, and with `choose` an item without a base is never given a filter and an all-NONE choice is a TRCB container.
// choose: the batch advisor sets the filters (to filters_out as well, where given).  orders given: the TRCU container
// (trc_encode_oplanes_batch_host, trc_planes_ocontainer.inc); it refuses a batch that is a TRCT or TRCB container's.  choose ==
// BATCH_CHOOSE_ORDER: the order advisor sets filters and orders under pred.strides (to filters_out / orders_out as well), and the
// container is the one of that choice: TRCU, TRCT or TRCB.
#define BATCH_CHOOSE_ORDER 2
static size_t batch_host_encode(const char *who, int codec, const trc_planes_item *items, BatchPred pred, int choose, uint8_t *filters_out,
                                size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on, void *out, size_t outcap,
                                uint8_t *orders_out = nullptr)
{
    if (!codec_ok(codec)) { fail(TRC_E_ARG, "codec %d not available", codec); return 0; }
    if (codec_row(codec).low4) { fail(TRC_E_ARG, "%s: " PLANES_LOW4, who, codec); return 0; }          // before anything is uploaded
    if (!items || !out || (items_on != TRC_ITEMS_HOST && items_on != TRC_ITEMS_DEV)) { fail(TRC_E_ARG, "%s: bad arguments (items, out, items_on %d)", who, items_on); return 0; }
    const TrcCodec &r = codec_row(codec);
    chunk = batch_resolve_chunk(r, items, count, esize, chunk);
    trc_planes_batch_plan B;
    if (trc_planes_batch_plan_host(items, count, esize, chunk ? chunk : TRC_CHUNK_AUTO_MIN, &B, nullptr)) return 0;     // (chunk 0 here: a bad batch, and the plan says why)
    bool any = false;
    if (trc_planes_batch_filters(who, pred.filters, count, &any)) return 0;
    if (pred.based && !choose) {
        if (!any) { fail(TRC_E_ARG, "%s: no item has a filter: that batch is a TRCB container (trc_encode_planes_batch_host)", who); return 0; }
        for (size_t i = 0; i < count; i++)
            if (pred.filters[i] != TRC_FILTER_NONE && (!pred.bases || !pred.bases[i])) { fail(TRC_E_ARG, "%s: item %zu: a filter against a base needs the base", who, i); return 0; }
    }
    bool strided = false;
    if (trc_planes_batch_strides(who, pred.filters, pred.strides, count, &strided)) return 0;
    bool ordered = false;
    if (trc_planes_batch_orders(who, pred.filters, pred.orders, count, &ordered)) return 0;
    if (pred.orders && !ordered) {
        fail(TRC_E_ARG, "%s: no zigzag-delta item has an order above 1: that batch is a TRCT or TRCB container (trc_encode_splanes_batch_host / trc_encode_planes_batch_host)", who);
        return 0;
    }
    if (pred.strides && !strided && !ordered && choose != BATCH_CHOOSE_ORDER) { fail(TRC_E_ARG, "%s: no item with a filter has a stride above 1: that batch is a TRCB container (trc_encode_planes_batch_host)", who); return 0; }
    if (!r.cdf && !r.ss) cdfnum = 0;
    const size_t bound = pred.based ? trc_planes_bbatch_bound(codec, items, count, esize, chunk, cdfnum) :
                         pred.orders || choose == BATCH_CHOOSE_ORDER ? trc_planes_obatch_bound(codec, items, count, esize, chunk, cdfnum) :
                         pred.strides ? trc_planes_sbatch_bound(codec, items, count, esize, chunk, cdfnum) : trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
    PlanesMap P;
    if (!bound || !planes_map(codec, (size_t)B.n_virtual, esize, chunk, P)) { fail(TRC_E_ARG, "%s: bad (codec, items, esize, chunk %u, cdfnum 0x%x)", who, chunk, cdfnum); return 0; }
    for (size_t i = 0; i < count; i++)
        if (!items[i].d_ptr) { fail(TRC_E_ARG, "%s: item %zu: null pointer", who, i); return 0; }
    HostCtx *cp = nullptr;
    std::unique_lock<std::mutex> lk;
    if (planes_ctx(cp, lk)) return 0;
    HostCtx &c = *cp;
    hipStream_t s = c.s_k[0];
    // the items on the device
    std::vector<trc_planes_item> dev(items, items + count);
    if (items_on == TRC_ITEMS_HOST) {
        std::vector<size_t> off(count);
        size_t pos = 0;
        for (size_t i = 0; i < count; i++) { off[i] = pos; pos += up16((size_t)items[i].n); }
        if (grow(&c.d_in, &c.cap_in, pos)) return 0;
        for (size_t i = 0; i < count; i++) dev[i].d_ptr = c.d_in + off[i];
        if (batch_items_up(c, s, c.d_in, items, count, off)) { (void)hipStreamSynchronize(s); return 0; }
    }
    std::vector<const void *> devb;
    if (pred.based) {
        std::vector<bool> want(count);
        for (size_t i = 0; i < count; i++) want[i] = choose ? pred.bases && pred.bases[i] : pred.filters[i] != TRC_FILTER_NONE;
        if (batch_bases_up(c, s, items, pred.bases, want, count, 0, count, items_on, devb)) { (void)hipStreamSynchronize(s); return 0; }
        pred.bases = devb.data();
    }
    const size_t fp_table = pred.based ? trc_base_fingerprint_batch_table_bytes(count) : 0;
    const size_t work = esize * P.slice + batch_pred_table_bytes(pred, count, B.chunks);
    const size_t awork = choose == BATCH_CHOOSE_ORDER ? TRC_PLANES_ADVISE_SLAB_BYTES + advise_otable_bytes(dev.data(), count, esize, chunk) :
                         choose ? TRC_PLANES_ADVISE_SLAB_BYTES + advise_table_bytes(dev.data(), count, esize, chunk) : 0;
    const size_t dirsz = up256(esize * 4 * P.nc + 256);
    if (grow(&c.d_cont, &c.cap_cont, dirsz + esize * P.buf) || grow(&c.d_work[0], &c.cap_work[0], work > awork ? work : awork) ||
        grow(&c.d_work[1], &c.cap_work[1], up256(bound) + fp_table)) { (void)hipStreamSynchronize(s); return 0; }
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + dirsz;
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    uint64_t *d_total = (uint64_t *)(c.d_small + PLANES_SMALL_TOT);
    int32_t *d_status = (int32_t *)(c.d_small + PLANES_SMALL_STATUS);
    uint64_t *d_size = (uint64_t *)(c.d_small + BATCH_SMALL_SIZE);
    std::vector<uint8_t> chosen, chosen_orders;
    if (choose == BATCH_CHOOSE_ORDER) {
        chosen.resize(count);
        chosen_orders.resize(count);
        if (trc_planes_advise_obatch_dev(15, dev.data(), pred.strides, count, esize, chunk, chosen.data(), chosen_orders.data(), nullptr, c.d_work[0], c.cap_work[0], s)) {
            (void)hipStreamSynchronize(s);
            return 0;
        }
        (void)trc_planes_batch_orders(who, chosen.data(), chosen_orders.data(), count, &ordered);
        (void)trc_planes_batch_strides(who, chosen.data(), pred.strides, count, &strided);
        pred = ordered ? batch_pred_orders(chosen.data(), pred.strides, chosen_orders.data()) : batch_pred_strides(chosen.data(), strided ? pred.strides : nullptr);
    } else if (choose) {
        chosen.resize(count);
        if (pred.based ? trc_planes_advise_bbatch_dev(7, dev.data(), pred.bases, count, esize, chunk, chosen.data(), nullptr, c.d_work[0], c.cap_work[0], s)
                       : trc_planes_advise_batch_dev(7, dev.data(), count, esize, chunk, chosen.data(), nullptr, c.d_work[0], c.cap_work[0], s)) { (void)hipStreamSynchronize(s); return 0; }
        pred.filters = chosen.data();
        any = false;
        for (size_t i = 0; i < count; i++) any |= chosen[i] != TRC_FILTER_NONE;
        if (pred.based && !any) pred = batch_pred_strides(chosen.data(), nullptr);      // no filter anywhere: the TRCB container
    }
    if (encode_batch(pred.based ? "encode_bplanes_batch" : "encode_splanes_batch", codec, dev.data(), pred, count, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                     d_clen, d_payload, d_total, c.d_work[0], c.cap_work[0], s) ||
        (pred.based ? trc_planes_bbatch_pack_dev(codec, dev.data(), pred.bases, pred.filters, count, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                                                d_clen, d_payload, d_total, c.d_work[1], up256(bound), d_size, c.d_work[1] + up256(bound), fp_table, s) :
         pred.orders ? trc_planes_obatch_pack_dev(codec, dev.data(), pred.filters, pred.strides, pred.orders, count, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                                              d_clen, d_payload, d_total, c.d_work[1], c.cap_work[1], d_size, s) :
         pred.strides ? trc_planes_sbatch_pack_dev(codec, dev.data(), pred.filters, pred.strides, count, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                                              d_clen, d_payload, d_total, c.d_work[1], c.cap_work[1], d_size, s)
                 : trc_planes_batch_pack_dev(codec, dev.data(), pred.filters, count, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                                             d_clen, d_payload, d_total, c.d_work[1], c.cap_work[1], d_size, s))) { (void)hipStreamSynchronize(s); return 0; }
    uint64_t size = 0;
    BCHK(hipMemcpyAsync(&size, d_size, sizeof size, hipMemcpyDeviceToHost, s));
    BCHK(hipStreamSynchronize(s));
    if (!size || size > bound) { fail(TRC_E_CDF, "%s: a plane has a distribution the 15-bit CDF cannot hold, or an impossible payload size", who); return 0; }
    if (outcap < size) { fail(TRC_E_ARG, "%s: out holds %zu bytes, the container needs %llu (trc_planes_batch_bound)", who, outcap, (unsigned long long)size); return 0; }
    BCHK(hipMemcpyAsync(out, c.d_work[1], (size_t)size, hipMemcpyDeviceToHost, s));
    BCHK(hipStreamSynchronize(s));
    if (choose && filters_out) memcpy(filters_out, chosen.data(), count);
    if (choose == BATCH_CHOOSE_ORDER && orders_out) memcpy(orders_out, chosen_orders.data(), count);
    return (size_t)size;
}

extern "C" size_t trc_encode_planes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters, size_t count, unsigned esize,
                                               uint32_t chunk, unsigned cdfnum, int items_on, void *out, size_t outcap)
{
    return batch_host_encode("encode_planes_batch_host", codec, items, batch_pred_strides(filters, nullptr), false, nullptr, count, esize, chunk, cdfnum, items_on, out, outcap);
}
extern "C" size_t trc_encode_aplanes_batch_host(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                                unsigned cdfnum, int items_on, void *out, size_t outcap, uint8_t *filters_out)
{
    return batch_host_encode("encode_aplanes_batch_host", codec, items, batch_pred_none(), true, filters_out, count, esize, chunk, cdfnum, items_on, out, outcap);
}

// the host decoders behind their checks: in = a checked TRCB container; pred = its filters, with the TRCT prefix's strides where it has one,
// or -- based -- the caller's bases, lying where the items lie, and want_fp = the TRCE prefix's fingerprints: the requested items' bases
// are fingerprinted and compared BEFORE anything is decoded (a batch range holds whole items, so each is seen whole)
static size_t batch_host_decode(const char *who, const void *in, BatchPred pred, const trc_planes_item *items, size_t count,
                                size_t first_item, size_t item_count, int items_on, const uint8_t *want_fp = nullptr)
{
    const uint8_t *b = (const uint8_t *)in;
    trc_planes_batch_hdr h;
    memcpy(&h, b, sizeof h);
    for (size_t i = 0; i < count; i++) {
        uint64_t n;
        memcpy(&n, b + sizeof h + 8 * i, 8);
        if (items[i].n != n) { fail(TRC_E_ARG, "%s: item %zu: the caller states %llu bytes, the container holds %llu", who, i, (unsigned long long)items[i].n, (unsigned long long)n); return 0; }
    }
    if (first_item > count || item_count > count - first_item) { fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count); return 0; }
    if (!item_count) return 0;
    for (size_t i = first_item; i < first_item + item_count; i++)
        if (!items[i].d_ptr) { fail(TRC_E_ARG, "%s: item %zu: null pointer", who, i); return 0; }
    const uint8_t *inner = b + h.inner;
    trc_planes_hdr p;
    memcpy(&p, inner, sizeof p);
    const TrcCodec &r = codec_row(p.codec);
    const unsigned esize = h.esize;
    const uint32_t chunk = h.chunk;
    trc_planes_batch_plan B;
    if (trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr)) return 0;
    // the covering chunks of every section travel as a coded batch of their own: `cnt` chunks from c0 on, the last one at the length
    // it was coded at -- a full chunk with its zero pad unless it is the batch's last
    size_t c0, cnt;
    batch_chunk_range(items, first_item, item_count, esize, chunk, c0, cnt);
    const size_t e0 = c0 * (size_t)chunk, e1 = (c0 + cnt) * (size_t)chunk;
    const size_t elems = (e1 < B.m_total ? e1 : (size_t)B.m_total) - e0;
    PlanesMap P;
    if (!planes_range_map(p.codec, elems * esize, esize, chunk, cnt, P)) { fail(TRC_E_ARG, "%s: bad (codec, items, esize, chunk)", who); return 0; }
    HostCtx *cp = nullptr;
    std::unique_lock<std::mutex> lk;
    if (planes_ctx(cp, lk)) return 0;
    HostCtx &c = *cp;
    hipStream_t s = c.s_k[0];
    std::vector<trc_planes_item> dev(items, items + count);
    size_t bytes = 0;
    std::vector<size_t> off(item_count);
    for (size_t i = 0; i < item_count; i++) { off[i] = bytes; bytes += up16((size_t)items[first_item + i].n); }
    if (items_on == TRC_ITEMS_HOST) {
        if (grow(&c.d_in, &c.cap_in, bytes)) return 0;
        for (size_t i = 0; i < count; i++) dev[i].d_ptr = i >= first_item && i < first_item + item_count ? c.d_in + off[i - first_item] : nullptr;
    }
    std::vector<const void *> devb;
    if (pred.based) {
        std::vector<bool> want(count);
        for (size_t i = 0; i < count; i++) want[i] = pred.filters[i] != TRC_FILTER_NONE;
        for (size_t i = first_item; i < first_item + item_count; i++)
            if (want[i] && (!pred.bases || !pred.bases[i])) { fail(TRC_E_ARG, "%s: item %zu: a filter against a base needs the base", who, i); return 0; }
        if (batch_bases_up(c, s, items, pred.bases, want, count, first_item, item_count, items_on, devb)) { (void)hipStreamSynchronize(s); return 0; }
        pred.bases = devb.data();
        const size_t tb = trc_base_fingerprint_batch_table_bytes(item_count);
        if (grow(&c.d_work[1], &c.cap_work[1], tb + 8 * item_count)) return 0;
        uint64_t *d_fp = (uint64_t *)(c.d_work[1] + tb);
        if (trc_base_fingerprint_batch_dev(items, pred.bases, pred.filters, count, first_item, item_count, d_fp, c.d_work[1], tb, s)) { (void)hipStreamSynchronize(s); return 0; }
        std::vector<uint64_t> got(item_count);
        BCHK(hipMemcpyAsync(got.data(), d_fp, 8 * item_count, hipMemcpyDeviceToHost, s));
        BCHK(hipStreamSynchronize(s));
        for (size_t j = 0; j < item_count; j++) {
            uint64_t stored;
            memcpy(&stored, want_fp + 8 * (first_item + j), 8);
            if (got[j] != stored) {
                fail(TRC_E_ARG, "%s: item %zu: base fingerprint 0x%016llx, the container was coded against 0x%016llx", who, first_item + j,
                     (unsigned long long)got[j], (unsigned long long)stored);
                return 0;
            }
        }
    }
    const size_t dirsz = up256(esize * 4 * cnt + 256);
    if (grow(&c.d_cont, &c.cap_cont, dirsz + esize * P.buf) || grow(&c.d_work[0], &c.cap_work[0], esize * P.slice + batch_pred_table_bytes(pred, item_count, cnt))) return 0;
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + dirsz;
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    PlanesSec S[8];
    planes_sections(inner, p, S);
    BatchCoded D;
    memset(&D, 0, sizeof D);
    for (unsigned k = 0; k < esize; k++) {
        trc_container_hdr sh;
        memcpy(&sh, S[k].cont, sizeof sh);
        trc_range R;
        range_plan(S[k].cont, sh, e0, elems, &R);
        const uint8_t *dir = S[k].cont + sizeof sh, *pay = dir + 4 * (size_t)B.chunks;
        if (r.cdf) BCHK(hipMemcpyAsync(d_cdf + k * TRC_PLANES_CDF_STRIDE, S[k].cdf, 2 * ((size_t)p.cdfnum + 1), hipMemcpyHostToDevice, s));
        BCHK(hipMemcpyAsync(d_clen + k * cnt, dir + 4 * c0, 4 * cnt, hipMemcpyHostToDevice, s));
        if (R.payload_len) BCHK(hipMemcpyAsync(d_payload + k * P.buf, pay + R.payload_off, (size_t)R.payload_len, hipMemcpyHostToDevice, s));
        D.cdf[k] = r.cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr;
        D.clen[k] = d_clen + k * cnt;
        D.payload[k] = d_payload + k * P.buf;
    }
    if (decode_batch(who, p.codec, D, elems, dev.data(), pred, count, first_item, item_count, esize, chunk, p.cdfnum, c.d_work[0], c.cap_work[0], s)) {
        (void)hipStreamSynchronize(s);
        return 0;
    }
    size_t delivered = 0;
    for (size_t i = first_item; i < first_item + item_count; i++) {
        if (items_on == TRC_ITEMS_HOST) BCHK(hipMemcpyAsync(items[i].d_ptr, dev[i].d_ptr, (size_t)items[i].n, hipMemcpyDeviceToHost, s));
        delivered += (size_t)items[i].n;
    }
    BCHK(hipStreamSynchronize(s));
    return delivered;
}
#undef BCHK

extern "C" size_t trc_decode_planes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                               size_t first_item, size_t item_count, int items_on)
{
    const char *who = "decode_planes_batch_host";
    if (!in || !items || (items_on != TRC_ITEMS_HOST && items_on != TRC_ITEMS_DEV)) { fail(TRC_E_ARG, "%s: bad arguments", who); return 0; }
    if (trc_planes_batch_check(in, inlen, count)) return 0;
    return batch_host_decode(who, in, batch_pred_strides(batch_filters(in, count), nullptr), items, count, first_item, item_count, items_on);
}

// ---- the TRCT container: the strides of a batch in front of its TRCB container ---------------------------------------------------
//   trc_planes_sbatch_hdr (16 B) | uint8 stride[count], zero-padded to a multiple of 16 | the TRCB container of (items, filters), inner = VS
static inline size_t sbatch_prefix_bytes(size_t count) { return sizeof(trc_planes_sbatch_hdr) + ((count + 15) & ~(size_t)15); }

extern "C" size_t trc_planes_sbatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
    return b ? sbatch_prefix_bytes(count) + b : 0;
}

// the verdict and, where it is good, the TRCB header and the prefix's length
static int sbatch_verdict(const void *buf, size_t buflen, size_t count_expected, trc_planes_batch_hdr &h, size_t &prefix, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, "strided batch container: " __VA_ARGS__); return TRC_E_ARG; } while (0)
    trc_planes_sbatch_hdr t;
    if (!buf || buflen < sizeof t) BAD("%zu bytes is shorter than the header", buflen);
    memcpy(&t, buf, sizeof t);
    if (t.magic != TRC_PLANES_SBATCH_MAGIC) BAD("bad magic 0x%08x", t.magic);
    if (t.version != 1) BAD("version %u (1)", t.version);
    if (t.zero || t.zero2) BAD("reserved fields are 0x%x / 0x%x, must be 0", t.zero, t.zero2);
    if (t.count < 1 || t.count > TRC_PLANES_BATCH_MAX) BAD("%llu items (1 .. %u)", (unsigned long long)t.count, TRC_PLANES_BATCH_MAX);
    if (count_expected != (size_t)-1 && t.count != count_expected) BAD("holds %llu items, caller expects %zu", (unsigned long long)t.count, count_expected);
    const size_t count = (size_t)t.count;
    prefix = sbatch_prefix_bytes(count);
    if (buflen < prefix) BAD("%zu bytes is shorter than the strides of %zu items", buflen, count);
    const uint8_t *b = (const uint8_t *)buf, *st = b + sizeof t;
    for (size_t i = 0; i < count; i++) if (st[i] < 1 || st[i] > TRC_STRIDE_MAX) BAD("item %zu: stride %u (1 .. %d)", i, (unsigned)st[i], TRC_STRIDE_MAX);
    for (size_t i = count; i < prefix - sizeof t; i++) if (st[i]) BAD("the stride padding must be zero bytes");
    char sub[400];
    if (batch_verdict(b + prefix, buflen - prefix, (size_t)-1, h, sub, sizeof sub)) BAD("%s", sub);
    if (h.count != t.count) BAD("%llu strides in front of a batch container of %llu items", (unsigned long long)t.count, (unsigned long long)h.count);
    const uint8_t *fl = b + prefix + sizeof h + 8 * count;
    for (size_t i = 0; i < count; i++)
        if (fl[i] == TRC_FILTER_NONE && st[i] != 1) BAD("item %zu: stride %u on an item without a filter (1)", i, (unsigned)st[i]);
    return TRC_OK;
#undef BAD
}
extern "C" int trc_planes_sbatch_check(const void *buf, size_t buflen, size_t count_expected)
{
    trc_planes_batch_hdr h;
    size_t prefix;
    char why[500];
    return sbatch_verdict(buf, buflen, count_expected, h, prefix, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}
extern "C" int trc_planes_sbatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint8_t *strides, size_t cap)
{
    trc_planes_batch_hdr hh;
    size_t prefix;
    char why[500];
    if (!h) return fail(TRC_E_ARG, "planes_sbatch_info: null header");
    if (sbatch_verdict(buf, buflen, (size_t)-1, hh, prefix, why, sizeof why)) return fail(TRC_E_ARG, "%s", why);
    *h = hh;
    const size_t cnt = cap < hh.count ? cap : (size_t)hh.count;
    const uint8_t *b = (const uint8_t *)buf;
    if (n) memcpy(n, b + prefix + sizeof hh, 8 * cnt);
    if (filters) memcpy(filters, b + prefix + sizeof hh + 8 * (size_t)hh.count, cnt);
    if (strides) memcpy(strides, b + sizeof(trc_planes_sbatch_hdr), cnt);
    return TRC_OK;
}

extern "C" int trc_planes_sbatch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                          unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                          const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                                          const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream)
{
    const char *who = "planes_sbatch_pack";
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, filters, count, nullptr))) return rc;
    bool strided;
    if ((rc = trc_planes_batch_strides(who, filters, strides, count, &strided))) return rc;
    if (!strided) return fail(TRC_E_ARG, "%s: no item with a filter has a stride above 1: that batch is a TRCB container (trc_planes_batch_pack_dev)", who);
    const size_t prefix = sbatch_prefix_bytes(count);
    if (d_out && out_bytes < prefix) return fail(TRC_E_WORK, "%s: d_out holds %zu B < required %zu B (trc_planes_sbatch_bound)", who, out_bytes,
                                                 trc_planes_sbatch_bound(codec, items, count, esize, chunk, cdfnum));
    // the TRCB part: every other check, its front and the pack kernel; it enqueues nothing unless all of them pass
    if ((rc = trc_planes_batch_pack_dev(codec, items, filters, count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                                        d_out ? (uint8_t *)d_out + prefix : nullptr, d_out ? out_bytes - prefix : 0, d_size, stream))) return rc;
    std::vector<uint8_t> f(prefix, 0);
    trc_planes_sbatch_hdr t;
    memset(&t, 0, sizeof t);
    t.magic = TRC_PLANES_SBATCH_MAGIC; t.version = 1; t.count = count;
    memcpy(f.data(), &t, sizeof t);
    for (size_t i = 0; i < count; i++) f[sizeof t + i] = filters[i] == TRC_FILTER_NONE ? 1 : strides[i];
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemcpyWithStream(d_out, f.data(), prefix, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(TRC_E_HIP, "%s: prefix upload: %s", who, hipGetErrorString(e));
    return trc_planes_pack_lead_launch(d_size, prefix, s);
}

extern "C" int trc_decode_splanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                                   const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                                   size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                                   const uint64_t *total, void *d_work, size_t work_bytes, void *stream)
{
    const size_t prefix = sbatch_prefix_bytes(count <= TRC_PLANES_BATCH_MAX ? count : 0);     // (a bad count: the plan says so before d_cont is looked at)
    return packed_decode("decode_splanes_batch_packed", codec, d_cont ? (const uint8_t *)d_cont + prefix : nullptr, prefix, cont_bytes, items,
                         batch_pred_strides(filters, strides), count, first_item, item_count, esize, chunk, cdfnum, total, d_work, work_bytes, stream);
}

extern "C" size_t trc_encode_splanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                                                size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                                void *out, size_t outcap)
{
    const char *who = "encode_splanes_batch_host";
    if (!strides) { fail(TRC_E_ARG, "%s: no strides: that batch is a TRCB container (trc_encode_planes_batch_host)", who); return 0; }
    return batch_host_encode(who, codec, items, batch_pred_strides(filters, strides), false, nullptr, count, esize, chunk, cdfnum, items_on, out, outcap);
}

extern "C" size_t trc_decode_splanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                                size_t first_item, size_t item_count, int items_on)
{
    const char *who = "decode_splanes_batch_host";
    if (!in || !items || (items_on != TRC_ITEMS_HOST && items_on != TRC_ITEMS_DEV)) { fail(TRC_E_ARG, "%s: bad arguments", who); return 0; }
    if (trc_planes_sbatch_check(in, inlen, count)) return 0;
    const size_t prefix = sbatch_prefix_bytes(count);
    const uint8_t *trcb = (const uint8_t *)in + prefix;
    return batch_host_decode(who, trcb, batch_pred_strides(batch_filters(trcb, count), (const uint8_t *)in + sizeof(trc_planes_sbatch_hdr)), items, count, first_item, item_count, items_on);
}
