// trc_planes_ocontainer.inc -- the TRCU container (included by trc_api.hip behind trc_planes_container.inc): the strides and the
// predictor orders of a batch in front of its TRCB container, as TRCT carries the strides alone.
//   trc_planes_obatch_hdr (16 B) | uint8 stride[count], zero-padded to a multiple of 16 | uint8 order[count], likewise
//   | the TRCB container of (items, filters), inner = the TRCP container of VO
// The stored stride of an item without a filter is 1, the stored order of an item whose filter is not ZDELTA is 1.  One layout per
// content: a batch in which no ZDELTA item has an order above 1 is a TRCT or TRCB container and is refused here.
static inline size_t obatch_prefix_bytes(size_t count) { return sizeof(trc_planes_obatch_hdr) + 2 * ((count + 15) & ~(size_t)15); }

extern "C" size_t trc_planes_obatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
    return b ? obatch_prefix_bytes(count) + b : 0;
}

// the verdict and, where it is good, the TRCB header and the prefix's length
static int obatch_verdict(const void *buf, size_t buflen, size_t count_expected, trc_planes_batch_hdr &h, size_t &prefix, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, "ordered batch container: " __VA_ARGS__); return TRC_E_ARG; } while (0)
    trc_planes_obatch_hdr t;
    if (!buf || buflen < sizeof t) BAD("%zu bytes is shorter than the header", buflen);
    memcpy(&t, buf, sizeof t);
    if (t.magic != TRC_PLANES_OBATCH_MAGIC) BAD("bad magic 0x%08x", t.magic);
    if (t.version != 1) BAD("version %u (1)", t.version);
    if (t.zero || t.zero2) BAD("reserved fields are 0x%x / 0x%x, must be 0", t.zero, t.zero2);
    if (t.count < 1 || t.count > TRC_PLANES_BATCH_MAX) BAD("%llu items (1 .. %u)", (unsigned long long)t.count, TRC_PLANES_BATCH_MAX);
    if (count_expected != (size_t)-1 && t.count != count_expected) BAD("holds %llu items, caller expects %zu", (unsigned long long)t.count, count_expected);
    const size_t count = (size_t)t.count, row = (count + 15) & ~(size_t)15;
    prefix = obatch_prefix_bytes(count);
    if (buflen < prefix) BAD("%zu bytes is shorter than the strides and orders of %zu items", buflen, count);
    const uint8_t *b = (const uint8_t *)buf, *st = b + sizeof t, *od = st + row;
    for (size_t i = 0; i < count; i++) if (st[i] < 1 || st[i] > TRC_STRIDE_MAX) BAD("item %zu: stride %u (1 .. %d)", i, (unsigned)st[i], TRC_STRIDE_MAX);
    for (size_t i = 0; i < count; i++) if (od[i] < 1 || od[i] > TRC_ORDER_MAX) BAD("item %zu: order %u (1 .. %d)", i, (unsigned)od[i], TRC_ORDER_MAX);
    for (size_t i = count; i < row; i++) if (st[i]) BAD("the stride padding must be zero bytes");
    for (size_t i = count; i < row; i++) if (od[i]) BAD("the order padding must be zero bytes");
    char sub[400];
    if (batch_verdict(b + prefix, buflen - prefix, (size_t)-1, h, sub, sizeof sub)) BAD("%s", sub);
    if (h.count != t.count) BAD("%llu strides and orders in front of a batch container of %llu items", (unsigned long long)t.count, (unsigned long long)h.count);
    const uint8_t *fl = b + prefix + sizeof h + 8 * count;
    bool ordered = false;
    for (size_t i = 0; i < count; i++) {
        if (fl[i] == TRC_FILTER_NONE && st[i] != 1) BAD("item %zu: stride %u on an item without a filter (1)", i, (unsigned)st[i]);
        if (fl[i] != TRC_FILTER_ZDELTA && od[i] != 1) BAD("item %zu: order %u on an item without the zigzag delta (1)", i, (unsigned)od[i]);
        ordered |= od[i] > 1;
    }
    if (!ordered) BAD("no item has an order above 1: that batch is a TRCT or TRCB container");
    return TRC_OK;
#undef BAD
}
extern "C" int trc_planes_obatch_check(const void *buf, size_t buflen, size_t count_expected)
{
    trc_planes_batch_hdr h;
    size_t prefix;
    char why[500];
    return obatch_verdict(buf, buflen, count_expected, h, prefix, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}
extern "C" int trc_planes_obatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint8_t *strides, uint8_t *orders, size_t cap)
{
    trc_planes_batch_hdr hh;
    size_t prefix;
    char why[500];
    if (!h) return fail(TRC_E_ARG, "planes_obatch_info: null header");
    if (obatch_verdict(buf, buflen, (size_t)-1, hh, prefix, why, sizeof why)) return fail(TRC_E_ARG, "%s", why);
    *h = hh;
    const size_t cnt = cap < hh.count ? cap : (size_t)hh.count, row = ((size_t)hh.count + 15) & ~(size_t)15;
    const uint8_t *b = (const uint8_t *)buf;
    if (n) memcpy(n, b + prefix + sizeof hh, 8 * cnt);
    if (filters) memcpy(filters, b + prefix + sizeof hh + 8 * (size_t)hh.count, cnt);
    if (strides) memcpy(strides, b + sizeof(trc_planes_obatch_hdr), cnt);
    if (orders) memcpy(orders, b + sizeof(trc_planes_obatch_hdr) + row, cnt);
    return TRC_OK;
}

extern "C" int trc_planes_obatch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                          size_t count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                          const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                                          const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream)
{
    const char *who = "planes_obatch_pack";
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, filters, count, nullptr))) return rc;
    if ((rc = trc_planes_batch_strides(who, filters, strides, count, nullptr))) return rc;
    bool ordered;
    if ((rc = trc_planes_batch_orders(who, filters, orders, count, &ordered))) return rc;
    if (!ordered)
        return fail(TRC_E_ARG, "%s: no zigzag-delta item has an order above 1: that batch is a TRCT or TRCB container (trc_planes_sbatch_pack_dev / trc_planes_batch_pack_dev)", who);
    const size_t prefix = obatch_prefix_bytes(count), row = (count + 15) & ~(size_t)15;
    if (d_out && out_bytes < prefix) return fail(TRC_E_WORK, "%s: d_out holds %zu B < required %zu B (trc_planes_obatch_bound)", who, out_bytes,
                                                 trc_planes_obatch_bound(codec, items, count, esize, chunk, cdfnum));
    // the TRCB part: every other check, its front and the pack kernel; it enqueues nothing unless all of them pass
    if ((rc = trc_planes_batch_pack_dev(codec, items, filters, count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                                        d_out ? (uint8_t *)d_out + prefix : nullptr, d_out ? out_bytes - prefix : 0, d_size, stream))) return rc;
    std::vector<uint8_t> f(prefix, 0);
    trc_planes_obatch_hdr t;
    memset(&t, 0, sizeof t);
    t.magic = TRC_PLANES_OBATCH_MAGIC; t.version = 1; t.count = count;
    memcpy(f.data(), &t, sizeof t);
    for (size_t i = 0; i < count; i++) {
        f[sizeof t + i] = filters[i] == TRC_FILTER_NONE || !strides ? 1 : strides[i];
        f[sizeof t + row + i] = filters[i] == TRC_FILTER_ZDELTA ? orders[i] : 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemcpyWithStream(d_out, f.data(), prefix, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(TRC_E_HIP, "%s: prefix upload: %s", who, hipGetErrorString(e));
    return trc_planes_pack_lead_launch(d_size, prefix, s);
}

extern "C" int trc_decode_oplanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                                   const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders, size_t count,
                                                   size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                                   const uint64_t *total, void *d_work, size_t work_bytes, void *stream)
{
    const size_t prefix = obatch_prefix_bytes(count <= TRC_PLANES_BATCH_MAX ? count : 0);     // (a bad count: the plan says so before d_cont is looked at)
    return packed_decode("decode_oplanes_batch_packed", codec, d_cont ? (const uint8_t *)d_cont + prefix : nullptr, prefix, cont_bytes, items,
                         batch_pred_orders(filters, strides, orders), count, first_item, item_count, esize, chunk, cdfnum, total, d_work, work_bytes, stream);
}

extern "C" size_t trc_encode_oplanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                                size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                                void *out, size_t outcap)
{
    const char *who = "encode_oplanes_batch_host";
    if (!orders) { fail(TRC_E_ARG, "%s: no orders: that batch is a TRCT or TRCB container (trc_encode_splanes_batch_host / trc_encode_planes_batch_host)", who); return 0; }
    return batch_host_encode(who, codec, items, batch_pred_orders(filters, strides, orders), false, nullptr, count, esize, chunk, cdfnum, items_on, out, outcap);
}

// the order advisor under the caller's strides (NULL: 1), then the container of its choice: TRCU, TRCT or TRCB
extern "C" size_t trc_encode_aoplanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize, uint32_t chunk,
                                                 unsigned cdfnum, int items_on, void *out, size_t outcap, uint8_t *filters_out, uint8_t *orders_out)
{
    return batch_host_encode("encode_aoplanes_batch_host", codec, items, batch_pred_strides(nullptr, strides), BATCH_CHOOSE_ORDER, filters_out, count, esize, chunk, cdfnum,
                             items_on, out, outcap, orders_out);
}

extern "C" size_t trc_decode_oplanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                                size_t first_item, size_t item_count, int items_on)
{
    const char *who = "decode_oplanes_batch_host";
    if (!in || !items || (items_on != TRC_ITEMS_HOST && items_on != TRC_ITEMS_DEV)) { fail(TRC_E_ARG, "%s: bad arguments", who); return 0; }
    if (trc_planes_obatch_check(in, inlen, count)) return 0;
    const size_t prefix = obatch_prefix_bytes(count), row = (count + 15) & ~(size_t)15;
    const uint8_t *trcb = (const uint8_t *)in + prefix, *st = (const uint8_t *)in + sizeof(trc_planes_obatch_hdr);
    return batch_host_decode(who, trcb, batch_pred_orders(batch_filters(trcb, count), st, st + row), items, count, first_item, item_count, items_on);
}
