// trc_planes_bcontainer.inc -- the TRCE container (included by trc_api.hip behind trc_planes_container.inc): a batch coded against a
// base per item in one piece.  The TRCB container has no place for a base, and a decode against the wrong base is silently wrong, so
// -- as TRCT does for the strides -- a prefix in front of an unchanged TRCB container names every item's base by its fingerprint:
//   trc_planes_bbatch_hdr (16 B) | uint64 base_fp[count], zero-padded to a multiple of 16 | the TRCB container of (items, filters), inner = VD
// base_fp[i] = trc_base_fingerprint_host(bases[i], n[i]) where filters[i] is not NONE, else 0.  A base's length is its item's.
static inline size_t bbatch_prefix_bytes(size_t count) { return sizeof(trc_planes_bbatch_hdr) + ((8 * count + 15) & ~(size_t)15); }

extern "C" size_t trc_planes_bbatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
    return b ? bbatch_prefix_bytes(count) + b : 0;
}

// the verdict and, where it is good, the TRCB header and the prefix's length
static int bbatch_verdict(const void *buf, size_t buflen, size_t count_expected, trc_planes_batch_hdr &h, size_t &prefix, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, "based batch container: " __VA_ARGS__); return TRC_E_ARG; } while (0)
    trc_planes_bbatch_hdr t;
    if (!buf || buflen < sizeof t) BAD("%zu bytes is shorter than the header", buflen);
    memcpy(&t, buf, sizeof t);
    if (t.magic != TRC_PLANES_BBATCH_MAGIC) BAD("bad magic 0x%08x", t.magic);
    if (t.version != 1) BAD("version %u (1)", t.version);
    if (t.zero || t.zero2) BAD("reserved fields are 0x%x / 0x%x, must be 0", t.zero, t.zero2);
    if (t.count < 1 || t.count > TRC_PLANES_BATCH_MAX) BAD("%llu items (1 .. %u)", (unsigned long long)t.count, TRC_PLANES_BATCH_MAX);
    if (count_expected != (size_t)-1 && t.count != count_expected) BAD("holds %llu items, caller expects %zu", (unsigned long long)t.count, count_expected);
    const size_t count = (size_t)t.count;
    prefix = bbatch_prefix_bytes(count);
    if (buflen < prefix) BAD("%zu bytes is shorter than the fingerprints of %zu items", buflen, count);
    const uint8_t *b = (const uint8_t *)buf, *fps = b + sizeof t;
    for (size_t i = 8 * count; i < prefix - sizeof t; i++) if (fps[i]) BAD("the fingerprint padding must be zero bytes");
    char sub[400];
    if (batch_verdict(b + prefix, buflen - prefix, (size_t)-1, h, sub, sizeof sub)) BAD("%s", sub);
    if (h.count != t.count) BAD("%llu fingerprints in front of a batch container of %llu items", (unsigned long long)t.count, (unsigned long long)h.count);
    const uint8_t *fl = batch_filters(b + prefix, count);
    bool any = false;
    for (size_t i = 0; i < count; i++) {
        uint64_t fp;
        memcpy(&fp, fps + 8 * i, 8);
        if (fl[i] == TRC_FILTER_NONE && fp) BAD("item %zu: base fingerprint 0x%016llx on an item without a filter (0)", i, (unsigned long long)fp);
        any |= fl[i] != TRC_FILTER_NONE;
    }
    if (!any) BAD("no item has a filter: that batch is a TRCB container");
    return TRC_OK;
#undef BAD
}
extern "C" int trc_planes_bbatch_check(const void *buf, size_t buflen, size_t count_expected)
{
    trc_planes_batch_hdr h;
    size_t prefix;
    char why[500];
    return bbatch_verdict(buf, buflen, count_expected, h, prefix, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}
extern "C" int trc_planes_bbatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint64_t *base_fp, size_t cap)
{
    trc_planes_batch_hdr hh;
    size_t prefix;
    char why[500];
    if (!h) return fail(TRC_E_ARG, "planes_bbatch_info: null header");
    if (bbatch_verdict(buf, buflen, (size_t)-1, hh, prefix, why, sizeof why)) return fail(TRC_E_ARG, "%s", why);
    *h = hh;
    const size_t cnt = cap < hh.count ? cap : (size_t)hh.count;
    const uint8_t *b = (const uint8_t *)buf;
    if (n) memcpy(n, b + prefix + sizeof hh, 8 * cnt);
    if (filters) memcpy(filters, batch_filters(b + prefix, (size_t)hh.count), cnt);
    if (base_fp) memcpy(base_fp, b + sizeof(trc_planes_bbatch_hdr), 8 * cnt);
    return TRC_OK;
}

extern "C" int trc_planes_bbatch_pack_dev(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                          unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                          const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                                          const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size,
                                          void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "planes_bbatch_pack";
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    bool any;
    if ((rc = trc_planes_batch_filters(who, filters, count, &any))) return rc;
    if (!any) return fail(TRC_E_ARG, "%s: no item has a filter: that batch is a TRCB container (trc_planes_batch_pack_dev)", who);
    if ((rc = trc_planes_bbatch_bases(who, bases, filters, 0, count))) return rc;
    const size_t prefix = bbatch_prefix_bytes(count);
    if (d_out && out_bytes < prefix) return fail(TRC_E_WORK, "%s: d_out holds %zu B < required %zu B (trc_planes_bbatch_bound)", who, out_bytes,
                                                 trc_planes_bbatch_bound(codec, items, count, esize, chunk, cdfnum));
    if (!d_table || ((uintptr_t)d_table & 255)) return fail(TRC_E_ARG, "%s: the table must be 256-byte aligned", who);
    const size_t need = trc_base_fingerprint_batch_table_bytes(count);
    if (table_bytes < need) return fail(TRC_E_WORK, "%s: table %zu B < required %zu B", who, table_bytes, need);
    // the TRCB part: every other check, its front and the pack kernel; it enqueues nothing unless all of them pass
    if ((rc = trc_planes_batch_pack_dev(codec, items, filters, count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                                        d_out ? (uint8_t *)d_out + prefix : nullptr, d_out ? out_bytes - prefix : 0, d_size, stream))) return rc;
    trc_planes_bbatch_hdr t;
    memset(&t, 0, sizeof t);
    t.magic = TRC_PLANES_BBATCH_MAGIC; t.version = 1; t.count = count;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyWithStream(d_out, &t, sizeof t, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(TRC_E_HIP, "%s: header upload: %s", who, hipGetErrorString(e));
    uint8_t *d_fp = (uint8_t *)d_out + sizeof t;
    if (prefix > sizeof t + 8 * count && (e = hipMemsetAsync(d_fp + 8 * count, 0, prefix - sizeof t - 8 * count, s)) != hipSuccess)
        return fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
    if ((rc = trc_base_fingerprint_batch_dev(items, bases, filters, count, 0, count, (uint64_t *)d_fp, d_table, table_bytes, stream))) return rc;
    return trc_planes_pack_lead_launch(d_size, prefix, s);
}

// Why the decode does not wait for trc_base_verify_batch_dev: see include/trc_hip.h (the join kernels stay as they are).
extern "C" int trc_decode_bplanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                                   const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                                   size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                                   const uint64_t *total, void *d_work, size_t work_bytes, void *stream)
{
    const size_t prefix = bbatch_prefix_bytes(count <= TRC_PLANES_BATCH_MAX ? count : 0);     // (a bad count: the plan says so before d_cont is looked at)
    return packed_decode("decode_bplanes_batch_packed", codec, d_cont ? (const uint8_t *)d_cont + prefix : nullptr, prefix, cont_bytes, items,
                         batch_pred_bases(filters, bases), count, first_item, item_count, esize, chunk, cdfnum, total, d_work, work_bytes, stream);
}

// ---- through host pointers: the bases lie where the items lie ----------------------------------------------------------------------
extern "C" size_t trc_encode_bplanes_batch_host(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters,
                                                size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                                void *out, size_t outcap)
{
    return batch_host_encode("encode_bplanes_batch_host", codec, items, BatchPred{ filters, nullptr, bases, true }, false, nullptr, count, esize, chunk, cdfnum,
                             items_on, out, outcap);
}
// the advisor against the bases first (trc_planes_advise_bbatch_dev, all three filters; bases[i] == NULL: no base, no filter), then
// exactly what the explicit call writes for that list: TRCE, or TRCB where no filter was chosen anywhere
extern "C" size_t trc_encode_abplanes_batch_host(int codec, const trc_planes_item *items, const void *const *bases, size_t count, unsigned esize,
                                                 uint32_t chunk, unsigned cdfnum, int items_on, void *out, size_t outcap, uint8_t *filters_out)
{
    return batch_host_encode("encode_abplanes_batch_host", codec, items, BatchPred{ nullptr, nullptr, bases, true }, true, filters_out, count, esize, chunk, cdfnum,
                             items_on, out, outcap);
}

extern "C" size_t trc_decode_bplanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, const void *const *bases, size_t count,
                                                size_t first_item, size_t item_count, int items_on)
{
    const char *who = "decode_bplanes_batch_host";
    if (!in || !items || (items_on != TRC_ITEMS_HOST && items_on != TRC_ITEMS_DEV)) { fail(TRC_E_ARG, "%s: bad arguments", who); return 0; }
    uint32_t magic = 0;
    if (inlen >= 4) memcpy(&magic, in, 4);
    if (magic == TRC_PLANES_BATCH_MAGIC)           // a plain TRCB container: no item has a base, `bases` is not looked at
        return trc_decode_planes_batch_host(in, inlen, items, count, first_item, item_count, items_on);
    if (trc_planes_bbatch_check(in, inlen, count)) return 0;
    const size_t prefix = bbatch_prefix_bytes(count);
    const uint8_t *trcb = (const uint8_t *)in + prefix;
    return batch_host_decode(who, trcb, batch_pred_bases(batch_filters(trcb, count), bases), items, count, first_item, item_count, items_on,
                             (const uint8_t *)in + sizeof(trc_planes_bbatch_hdr));
}
