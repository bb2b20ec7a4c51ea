// trc_planes_batch.inc -- the coded planes calls over a BATCH of separate allocations (included by trc_api.hip behind
// trc_planes.inc): the batched split / join kernels (trc_planes_batch.hip) around the per-plane loop of trc_planes.inc.
//
// The planes of the virtual buffer V(items, esize, chunk) (include/trc_hip.h) are ordinary planes of M elements, so everything here
// is the unbatched call on (M * esize, esize, chunk) with another split in front or another join behind; item i is the chunk range
// [first[i], first[i] + nc[i]) of every plane.  Nothing here knows a coder.
//   workspace: the planes workspace of (M * esize, esize, chunk) -- planes_map / planes_range_map -- followed by the table
#include "trc_planes_pred.h"                      // BatchPred, its table, split_batch / join_batch (trc_planes_batch.hip)
int trc_planes_batch_plan_quiet(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, trc_planes_batch_plan *plan, uint64_t *first_chunk);
int trc_planes_batch_ptrs_ok(const trc_planes_item *items, size_t first_item, size_t item_count);
int trc_planes_batch_filters(const char *who, const uint8_t *filters, size_t count, bool *any);      // trc_fplanes_batch.inc
int trc_planes_batch_strides(const char *who, const uint8_t *filters, const uint8_t *strides, size_t count, bool *strided);      // trc_splanes_batch.inc
int trc_planes_batch_orders(const char *who, const uint8_t *filters, const uint8_t *orders, size_t count, bool *ordered);        // trc_oplanes_batch.inc
int trc_planes_bbatch_bases(const char *who, const void *const *bases, const uint8_t *filters, size_t first_item, size_t item_count);      // trc_bplanes_batch.inc

// the workspaces of a call whose table is `pred`'s
static size_t batch_work_bytes(const BatchPred &pred, int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    trc_planes_batch_plan B;
    PlanesMap P;
    if (trc_planes_batch_plan_quiet(items, count, esize, chunk, &B, nullptr) || !trc_planes_batch_ptrs_ok(items, 0, count)) return 0;
    if (!planes_map(codec, (size_t)B.n_virtual, esize, chunk, P)) return 0;
    return esize * P.slice + batch_pred_table_bytes(pred, count, B.chunks);
}
extern "C" size_t trc_planes_batch_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    return batch_work_bytes(batch_pred_none(), codec, items, count, esize, chunk);
}

// the chunk range of items [first_item, first_item + item_count) of a planned batch
static void batch_chunk_range(const trc_planes_item *items, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, size_t &c0, size_t &cnt)
{
    c0 = cnt = 0;
    for (size_t i = 0; i < first_item + item_count; i++) {
        const size_t nc = (size_t)((items[i].n / esize + chunk - 1) / chunk);
        if (i < first_item) c0 += nc; else cnt += nc;
    }
}
static size_t batch_range_work_bytes(const BatchPred &pred, int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                     size_t first_item, size_t item_count)
{
    trc_planes_batch_plan B;
    PlanesMap P;
    if (trc_planes_batch_plan_quiet(items, count, esize, chunk, &B, nullptr)) return 0;
    if (first_item > count || item_count > count - first_item || !item_count || !trc_planes_batch_ptrs_ok(items, first_item, item_count)) return 0;
    size_t c0, cnt;
    batch_chunk_range(items, first_item, item_count, esize, chunk, c0, cnt);
    if (!planes_range_map(codec, (size_t)B.n_virtual, esize, chunk, cnt, P)) return 0;
    return esize * P.slice + batch_pred_table_bytes(pred, item_count, cnt);
}
extern "C" size_t trc_planes_batch_range_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                                    size_t first_item, size_t item_count)
{
    return batch_range_work_bytes(batch_pred_none(), codec, items, count, esize, chunk, first_item, item_count);
}

// the encoders of every kind of batch (BatchPred, trc_planes_pred.h): the split hands an all-NONE batch to the unfiltered kernels and
// a batch without a stride above 1 to the filtered ones; against bases the table holds the base pointers behind the map
static int encode_batch(const char *who, int codec, const trc_planes_item *items, const BatchPred pred, size_t count, unsigned esize, uint32_t chunk,
                        uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status, uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                        void *d_work, size_t work_bytes, void *stream)
{
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, pred.filters, count, nullptr))) return rc;      // a bad filter id: after the plan, before anything else
    if ((rc = trc_planes_batch_strides(who, pred.filters, pred.strides, count, nullptr))) return rc;      // then a bad stride
    if ((rc = trc_planes_batch_orders(who, pred.filters, pred.orders, count, nullptr))) return rc;        // then a bad order
    const size_t n = (size_t)B.n_virtual;
    if ((rc = planes_common(who, codec, n, esize, d_work))) return rc;
    if ((rc = check_common(codec, n / esize, chunk, d_cdf, cdfnum))) return rc;
    const TrcCodec &r = codec_row(codec);
    if (r.cdf && !d_status) return fail(TRC_E_ARG, "%s: a static coder needs d_status (one int32 per plane)", who);
    if (!r.cdf && d_status) return fail(TRC_E_ARG, "%s: codec %d builds no CDF: d_status must be NULL", who, codec);
    PlanesMap P;
    if (!planes_map(codec, n, esize, chunk, P)) return fail(TRC_E_ARG, "%s: bad (codec, items, esize, chunk)", who);
    if (!trc_planes_batch_ptrs_ok(items, 0, count)) return fail(TRC_E_ARG, "%s: every item's pointer must be non-null and 16-byte aligned", who);
    if (pred.based && (rc = trc_planes_bbatch_bases(who, pred.bases, pred.filters, 0, count))) return rc;
    const size_t table = batch_pred_table_bytes(pred, count, B.chunks), need = esize * P.slice + table;
    if (work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    if (!d_clen || !d_payload || !d_total || ((uintptr_t)d_payload & 1) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_total & 7))
        return fail(TRC_E_ARG, "%s: d_clen must be 4-byte, d_payload 2-byte, d_total 8-byte aligned", who);
    uint8_t *w = (uint8_t *)d_work;
    if ((rc = split_batch(pred.based ? "planes_split_bbatch" : "planes_split_sbatch", items, pred, count, esize, chunk, w, P.slice, w + esize * P.slice, table, stream))) return rc;
    for (unsigned k = 0; k < esize; k++) {         // as trc_encode_fplanes_dev
        uint8_t *plane = w + k * P.slice, *pw = plane + P.buf;
        uint16_t *cdf = r.cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr;
        if (r.cdf && (rc = trc_cdfini_dev(plane, P.m, cdf, cdfnum, d_status + k, pw, stream))) return rc;
        if ((rc = trc_encode_dev(codec, plane, P.m, chunk, cdf, cdfnum, d_clen + k * P.nc, (uint8_t *)d_payload + k * P.buf, d_total + k,
                                 pw, P.work, stream))) return rc;
    }
    return TRC_OK;
}

extern "C" int trc_encode_planes_batch_dev(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                           uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                           uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                           void *d_work, size_t work_bytes, void *stream)
{
    return encode_batch("encode_planes_batch", codec, items, batch_pred_none(), count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                        d_work, work_bytes, stream);
}
extern "C" int trc_encode_fplanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, size_t count, unsigned esize, uint32_t chunk,
                                            uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                            uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return encode_batch("encode_fplanes_batch", codec, items, batch_pred_strides(filters, nullptr), count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                        d_work, work_bytes, stream);
}
extern "C" int trc_encode_splanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                            unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                            uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return encode_batch("encode_splanes_batch", codec, items, batch_pred_strides(filters, strides), count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total,
                        d_work, work_bytes, stream);
}

// a predictor order per ZDELTA item behind the strides (orders == NULL, or no such item with an order above 1: the splanes call)
extern "C" int trc_encode_oplanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                            size_t count, unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                            uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return encode_batch("encode_oplanes_batch", codec, items, batch_pred_orders(filters, strides, orders), count, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload,
                        d_total, d_work, work_bytes, stream);
}

// the coded buffers of a batch, plane by plane: wherever the directories, payloads and CDFs (static coders; else NULL) of the planes lie
struct BatchCoded { const uint32_t *clen[8]; const uint8_t *payload[8]; const uint16_t *cdf[8]; };
// ... of the batched calls' flat buffers: directories NC entries, payloads `pitch` bytes, CDFs TRC_PLANES_CDF_STRIDE entries apart
// (a batch the plan rejects: plane 0 alone, which is all decode_batch looks at before it says why)
static BatchCoded coded_flat(const uint32_t *d_clen, const void *d_payload, const uint16_t *d_cdf,
                             const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    BatchCoded S;
    memset(&S, 0, sizeof S);
    trc_planes_batch_plan B;
    const bool ok = !trc_planes_batch_plan_quiet(items, count, esize, chunk, &B, nullptr);
    for (unsigned k = 0; k < (ok ? esize : 1u); k++) {
        S.clen[k] = d_clen ? d_clen + k * (size_t)(ok ? B.chunks : 0) : nullptr;
        S.payload[k] = d_payload ? (const uint8_t *)d_payload + k * (size_t)(ok ? B.pitch : 0) : nullptr;
        S.cdf[k] = d_cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr;
    }
    return S;
}

// sub_m != 0: the coded buffers hold the covering chunks of the requested items alone, as a coded buffer of sub_m elements (the
// host-pointer decoder, trc_planes_container.inc); else they hold the whole batch
static int decode_batch(const char *who, int codec, const BatchCoded &S, size_t sub_m,
                        const trc_planes_item *items, const BatchPred pred, size_t count, size_t first_item, size_t item_count,
                        unsigned esize, uint32_t chunk, unsigned cdfnum, void *d_work, size_t work_bytes, void *stream)
{
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if ((rc = trc_planes_batch_filters(who, pred.filters, count, nullptr))) return rc;      // a bad filter id: after the plan, before anything else
    if ((rc = trc_planes_batch_strides(who, pred.filters, pred.strides, count, nullptr))) return rc;      // then a bad stride
    if ((rc = trc_planes_batch_orders(who, pred.filters, pred.orders, count, nullptr))) return rc;        // then a bad order
    const size_t m = sub_m ? sub_m : (size_t)B.m_total, n = m * esize;
    if ((rc = planes_common(who, codec, n, esize, d_work))) return rc;
    if ((rc = check_common(codec, m, chunk, S.cdf[0], cdfnum))) return rc;
    if (first_item > count || item_count > count - first_item)
        return fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    if (!trc_planes_batch_ptrs_ok(items, first_item, item_count)) return fail(TRC_E_ARG, "%s: every requested item's pointer must be non-null and 16-byte aligned", who);
    size_t c0, cnt;
    batch_chunk_range(items, first_item, item_count, esize, chunk, c0, cnt);
    PlanesMap P;
    if (!planes_range_map(codec, n, esize, chunk, cnt, P)) return fail(TRC_E_ARG, "%s: bad (codec, items, esize, chunk)", who);
    if (pred.based && (rc = trc_planes_bbatch_bases(who, pred.bases, pred.filters, first_item, item_count))) return rc;
    const size_t table = batch_pred_table_bytes(pred, item_count, cnt), need = esize * P.slice + table;
    if (work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    if (!S.clen[0] || !S.payload[0] || ((uintptr_t)S.payload[0] & 1) || ((uintptr_t)S.clen[0] & 3))
        return fail(TRC_E_ARG, "%s: d_clen must be 4-byte, d_payload 2-byte aligned", who);
    const TrcCodec &r = codec_row(codec);
    uint8_t *w = (uint8_t *)d_work;
    for (unsigned k = 0; k < esize; k++) {         // as trc_decode_fplanes_range_dev; the pad behind an item is decoded with it
        uint8_t *plane = w + k * P.slice;
        if ((rc = trc_decode_range_dev(codec, S.clen[k], S.payload[k], m, chunk, sub_m ? 0 : c0, cnt,
                                       r.cdf ? S.cdf[k] : nullptr, cdfnum, plane, plane + P.buf, P.work, stream))) return rc;
    }
    return join_batch(pred.based ? "planes_join_bbatch" : "planes_join_sbatch", w, P.slice, items, pred, count, first_item, item_count, esize, chunk,
                      w + esize * P.slice, table, stream);
}

extern "C" int trc_decode_planes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                           const trc_planes_item *items, size_t count, size_t first_item, size_t item_count,
                                           unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                           void *d_work, size_t work_bytes, void *stream)
{
    return decode_batch("decode_planes_batch", codec, coded_flat(d_clen, d_payload, d_cdf, items, count, esize, chunk), 0, items, batch_pred_none(), count,
                        first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}
extern "C" int trc_decode_fplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                            const trc_planes_item *items, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                            unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return decode_batch("decode_fplanes_batch", codec, coded_flat(d_clen, d_payload, d_cdf, items, count, esize, chunk), 0, items, batch_pred_strides(filters, nullptr),
                        count, first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}
extern "C" int trc_decode_splanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                            const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                            size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return decode_batch("decode_splanes_batch", codec, coded_flat(d_clen, d_payload, d_cdf, items, count, esize, chunk), 0, items, batch_pred_strides(filters, strides),
                        count, first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}

extern "C" int trc_decode_oplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                            const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders, size_t count,
                                            size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return decode_batch("decode_oplanes_batch", codec, coded_flat(d_clen, d_payload, d_cdf, items, count, esize, chunk), 0, items,
                        batch_pred_orders(filters, strides, orders), count, first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}

// ---- a base per item: the filters are against bases[i] (trc_bplanes_batch.inc); the workspace holds the base pointers as well ------
// (filters == NULL: the unfiltered call, under its own name)
extern "C" size_t trc_planes_bbatch_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    return batch_work_bytes(BATCH_PRED_BASED, codec, items, count, esize, chunk);
}
extern "C" size_t trc_planes_bbatch_range_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                                     size_t first_item, size_t item_count)
{
    return batch_range_work_bytes(BATCH_PRED_BASED, codec, items, count, esize, chunk, first_item, item_count);
}
extern "C" int trc_encode_bplanes_batch_dev(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                            unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                            uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return encode_batch(filters ? "encode_bplanes_batch" : "encode_planes_batch", codec, items, batch_pred_bases(filters, bases), count, esize, chunk,
                        d_cdf, cdfnum, d_status, d_clen, d_payload, d_total, d_work, work_bytes, stream);
}
extern "C" int trc_decode_bplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload, const trc_planes_item *items,
                                            const void *const *bases, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                            unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_work, size_t work_bytes, void *stream)
{
    return decode_batch(filters ? "decode_bplanes_batch" : "decode_planes_batch", codec, coded_flat(d_clen, d_payload, d_cdf, items, count, esize, chunk), 0,
                        items, batch_pred_bases(filters, bases), count, first_item, item_count, esize, chunk, cdfnum, d_work, work_bytes, stream);
}

// ---- the batch advisor: a filter per item from the histograms of trc_planes_hist_batch_dev ---------------------------------------
int trc_planes_hist_batch_run(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t first_item, size_t item_count,
                              unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);      // trc_planes_hist_batch.inc
int trc_planes_hist_bbatch_run(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t first_item, size_t item_count,
                               unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);     // likewise

// trc_planes_advise on items [base, base + count) of a batch, hist = the first one's slice: choice[i] and advice[i] (may be NULL)
// count from `base` as well; the index in an error's text is the item's index in the batch.  based: the filters are against
// bases[i] (of the whole batch), and an item without a base is judged under the unfiltered row alone
static int advise_items(const uint64_t *hist, unsigned filters, unsigned esize, const trc_planes_item *items, size_t base, size_t count,
                        uint8_t *choice, trc_planes_advice *advice, bool based = false, const void *const *bases = nullptr)
{
    const size_t slice = (size_t)3 * esize * 256;
    for (size_t i = 0; i < count; i++) {
        const uint64_t n = items[base + i].n;
        if (n < esize || n % esize)
            return fail(TRC_E_ARG, "planes_advise_batch: item %zu has %llu bytes: not a whole number (at least one) of %u-byte elements", base + i, (unsigned long long)n, esize);
        trc_planes_advice a;
        if (trc_planes_advise(hist + i * slice, based && !(bases && bases[base + i]) ? filters & 1u : filters, esize, (size_t)(n / esize), &a)) {
            char why[400];
            snprintf(why, sizeof why, "%s", g_err);
            return fail(TRC_E_ARG, "planes_advise_batch: item %zu: %s", base + i, why);
        }
        choice[base + i] = (uint8_t)a.filter;
        if (advice) advice[base + i] = a;
    }
    return TRC_OK;
}

// host only.  The choices reach filters_out only when every item has passed.
extern "C" int trc_planes_advise_batch(const uint64_t *hist, unsigned filters, unsigned esize, const trc_planes_item *items, size_t count,
                                       uint8_t *filters_out, trc_planes_advice *advice)
{
    if (!hist || !items || !filters_out) return fail(TRC_E_ARG, "planes_advise_batch: null histograms, items or filters_out");
    if (count == 0 || count > TRC_PLANES_BATCH_MAX) return fail(TRC_E_ARG, "planes_advise_batch: %zu items (1 .. %u)", count, TRC_PLANES_BATCH_MAX);
    if (filters < 1 || filters > 7) return fail(TRC_E_ARG, "planes_advise_batch: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", filters);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "planes_advise_batch: esize %u (2, 4 or 8)", esize);
    std::vector<uint8_t> choice(count);
    const int rc = advise_items(hist, filters, esize, items, 0, count, choice.data(), advice);
    if (rc) return rc;
    memcpy(filters_out, choice.data(), count);
    return TRC_OK;
}

// the same against a base per item: item i under the bit set filters & (bases[i] ? 7 : 1), so an item without a base is never given a
// filter (and is an error where `filters` does not hold the unfiltered row)
extern "C" int trc_planes_advise_bbatch(const uint64_t *hist, unsigned filters, unsigned esize, const trc_planes_item *items,
                                        const void *const *bases, size_t count, uint8_t *filters_out, trc_planes_advice *advice)
{
    if (!hist || !items || !filters_out) return fail(TRC_E_ARG, "planes_advise_batch: null histograms, items or filters_out");
    if (count == 0 || count > TRC_PLANES_BATCH_MAX) return fail(TRC_E_ARG, "planes_advise_batch: %zu items (1 .. %u)", count, TRC_PLANES_BATCH_MAX);
    if (filters < 1 || filters > 7) return fail(TRC_E_ARG, "planes_advise_batch: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", filters);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "planes_advise_batch: esize %u (2, 4 or 8)", esize);
    std::vector<uint8_t> choice(count);
    const int rc = advise_items(hist, filters, esize, items, 0, count, choice.data(), advice, true, bases);
    if (rc) return rc;
    memcpy(filters_out, choice.data(), count);
    return TRC_OK;
}

// items per slab of trc_planes_advise_batch_dev: what TRC_PLANES_ADVISE_SLAB_BYTES of histograms hold; TRC_PLANES_ADVISE_SLAB_ITEMS
// in the environment lowers it (test aid: a small batch in several slabs)
static size_t advise_slab_items(unsigned esize)
{
    size_t s = TRC_PLANES_ADVISE_SLAB_BYTES / trc_planes_hist_bytes(esize);
    const char *e = getenv("TRC_PLANES_ADVISE_SLAB_ITEMS");
    if (e) { const long x = strtol(e, 0, 10); if (x >= 1 && (size_t)x < s) s = (size_t)x; }
    return s;
}
// the table of the largest slab of a planned batch
static size_t advise_table_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    const size_t slab = advise_slab_items(esize);
    size_t table = 0;
    for (size_t i0 = 0; i0 < count; i0 += slab) {
        const size_t cnt = count - i0 < slab ? count - i0 : slab;
        uint64_t chunks = 0;
        for (size_t i = i0; i < i0 + cnt; i++) chunks += (items[i].n / esize + chunk - 1) / chunk;
        const size_t t = trc_planes_batch_table_bytes(cnt, chunks);
        if (t > table) table = t;
    }
    return table;
}
// the slab's histograms | the table of the largest slab
extern "C" size_t trc_planes_advise_batch_work_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    if (trc_planes_batch_plan_quiet(items, count, esize, chunk, nullptr, nullptr) || !trc_planes_batch_ptrs_ok(items, 0, count)) return 0;
    return TRC_PLANES_ADVISE_SLAB_BYTES + advise_table_bytes(items, count, esize, chunk);
}

// all three advisors: strides == NULL and !based is trc_planes_advise_batch_dev; based: against bases[i] (NULL entries, or bases NULL: no base)
static int advise_batch_dev(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize, uint32_t chunk,
                            uint8_t *filters_out, trc_planes_advice *advice, void *d_work, size_t work_bytes, void *stream,
                            bool based = false, const void *const *bases = nullptr)
{
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if (filters < 1 || filters > 7) return fail(TRC_E_ARG, "planes_advise_batch: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", filters);
    if ((rc = trc_planes_batch_strides("planes_advise_sbatch", nullptr, strides, count, nullptr))) return rc;
    if (!filters_out) return fail(TRC_E_ARG, "planes_advise_batch: null filters_out");
    if (!trc_planes_batch_ptrs_ok(items, 0, count)) return fail(TRC_E_ARG, "planes_advise_batch: every item's pointer must be non-null and 16-byte aligned");
    if (!d_work || ((uintptr_t)d_work & 255)) return fail(TRC_E_ARG, "planes_advise_batch: the workspace must be 256-byte aligned");
    const size_t table = advise_table_bytes(items, count, esize, chunk), need = TRC_PLANES_ADVISE_SLAB_BYTES + table;
    if (work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    const size_t slab = advise_slab_items(esize), slice = (size_t)3 * esize * 256;
    hipStream_t s = (hipStream_t)stream;
    uint64_t *d_hist = (uint64_t *)d_work;
    std::vector<uint64_t> hist((count < slab ? count : slab) * slice);
    std::vector<uint8_t> choice(count);
    for (size_t i0 = 0; i0 < count; i0 += slab) {
        const size_t cnt = count - i0 < slab ? count - i0 : slab;
        if ((rc = based ? trc_planes_hist_bbatch_run(filters, items, bases, i0, cnt, esize, chunk, d_hist, (uint8_t *)d_work + TRC_PLANES_ADVISE_SLAB_BYTES, table, s)
                        : trc_planes_hist_batch_run(filters, items, strides, i0, cnt, esize, chunk, d_hist, (uint8_t *)d_work + TRC_PLANES_ADVISE_SLAB_BYTES, table, s))) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        HIPCHK(hipMemcpyAsync(hist.data(), d_hist, cnt * slice * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if ((rc = advise_items(hist.data(), filters, esize, items, i0, cnt, choice.data(), advice, based, bases))) return rc;
    }
    memcpy(filters_out, choice.data(), count);
    return TRC_OK;
}

extern "C" int trc_planes_advise_batch_dev(unsigned filters, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                           uint8_t *filters_out, trc_planes_advice *advice, void *d_work, size_t work_bytes, void *stream)
{
    return advise_batch_dev(filters, items, nullptr, count, esize, chunk, filters_out, advice, d_work, work_bytes, stream);
}
// the filter per item under the caller's strides: the slab walk above over trc_planes_hist_sbatch_dev's histograms
extern "C" int trc_planes_advise_sbatch_dev(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize,
                                            uint32_t chunk, uint8_t *filters_out, trc_planes_advice *advice, void *d_work, size_t work_bytes, void *stream)
{
    return advise_batch_dev(filters, items, strides, count, esize, chunk, filters_out, advice, d_work, work_bytes, stream);
}
// the filter per item against bases[i]: the slab walk above over trc_planes_hist_bbatch_dev's histograms, same workspace function
extern "C" int trc_planes_advise_bbatch_dev(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t count, unsigned esize,
                                            uint32_t chunk, uint8_t *filters_out, trc_planes_advice *advice, void *d_work, size_t work_bytes, void *stream)
{
    return advise_batch_dev(filters, items, nullptr, count, esize, chunk, filters_out, advice, d_work, work_bytes, stream, true, bases);
}

// ---- the order advisor of a batch: a filter and an order per item from the histograms of trc_planes_hist_obatch_dev --------------
int trc_planes_hist_obatch_run(unsigned orders, const trc_planes_item *items, const uint8_t *strides, size_t first_item, size_t item_count,
                               unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);     // trc_oplanes_batch.inc

// trc_planes_advise_order on items [base, base + count) of a batch, hist = the first one's slice: choice[i] (the order, 0 .. 3) and
// advice[i] (may be NULL) count from `base` as well; the index in an error's text is the item's index in the batch
static int advise_order_items(const uint64_t *hist, unsigned orders, unsigned esize, const trc_planes_item *items, size_t base, size_t count,
                              uint8_t *choice, trc_planes_order_advice *advice)
{
    const size_t slice = (size_t)4 * esize * 256;
    for (size_t i = 0; i < count; i++) {
        const uint64_t n = items[base + i].n;
        if (n < esize || n % esize)
            return fail(TRC_E_ARG, "planes_advise_obatch: item %zu has %llu bytes: not a whole number (at least one) of %u-byte elements", base + i, (unsigned long long)n, esize);
        trc_planes_order_advice a;
        if (trc_planes_advise_order(hist + i * slice, orders, esize, (size_t)(n / esize), &a)) {
            char why[400];
            snprintf(why, sizeof why, "%s", g_err);
            return fail(TRC_E_ARG, "planes_advise_obatch: item %zu: %s", base + i, why);
        }
        choice[base + i] = (uint8_t)a.order;
        if (advice) advice[base + i] = a;
    }
    return TRC_OK;
}
// the choices as the ordered batch calls take them: order 0 is no filter (and order 1 in orders_out), else the zigzag delta
static void advise_order_out(const std::vector<uint8_t> &choice, uint8_t *filters_out, uint8_t *orders_out)
{
    for (size_t i = 0; i < choice.size(); i++) {
        filters_out[i] = choice[i] ? TRC_FILTER_ZDELTA : TRC_FILTER_NONE;
        orders_out[i] = choice[i] ? choice[i] : 1;
    }
}

// host only.  The choices reach filters_out and orders_out only when every item has passed.
extern "C" int trc_planes_advise_obatch(const uint64_t *hist, unsigned orders, unsigned esize, const trc_planes_item *items, size_t count,
                                        uint8_t *filters_out, uint8_t *orders_out, trc_planes_order_advice *advice)
{
    if (!hist || !items || !filters_out || !orders_out) return fail(TRC_E_ARG, "planes_advise_obatch: null histograms, items, filters_out or orders_out");
    if (count == 0 || count > TRC_PLANES_BATCH_MAX) return fail(TRC_E_ARG, "planes_advise_obatch: %zu items (1 .. %u)", count, TRC_PLANES_BATCH_MAX);
    if (orders < 1 || orders > 15) return fail(TRC_E_ARG, "planes_advise_obatch: orders 0x%x (a bit set: bit k = order k, 1 .. 15)", orders);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "planes_advise_obatch: esize %u (2, 4 or 8)", esize);
    std::vector<uint8_t> choice(count);
    std::vector<trc_planes_order_advice> adv(advice ? count : 0);        // (what decided reaches the caller with the choices, not before)
    const int rc = advise_order_items(hist, orders, esize, items, 0, count, choice.data(), advice ? adv.data() : nullptr);
    if (rc) return rc;
    if (advice) memcpy(advice, adv.data(), count * sizeof *advice);
    advise_order_out(choice, filters_out, orders_out);
    return TRC_OK;
}

// items per slab of trc_planes_advise_obatch_dev: a slice is 4/3 of a filter slice, so a slab holds 3/4 of the items
static size_t advise_oslab_items(unsigned esize)
{
    size_t s = TRC_PLANES_ADVISE_SLAB_BYTES / trc_planes_hist_order_bytes(esize);
    const char *e = getenv("TRC_PLANES_ADVISE_SLAB_ITEMS");
    if (e) { const long x = strtol(e, 0, 10); if (x >= 1 && (size_t)x < s) s = (size_t)x; }
    return s;
}
static size_t advise_otable_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    const size_t slab = advise_oslab_items(esize);
    size_t table = 0;
    for (size_t i0 = 0; i0 < count; i0 += slab) {
        const size_t cnt = count - i0 < slab ? count - i0 : slab;
        uint64_t chunks = 0;
        for (size_t i = i0; i < i0 + cnt; i++) chunks += (items[i].n / esize + chunk - 1) / chunk;
        const size_t t = trc_planes_batch_table_bytes(cnt, chunks);
        if (t > table) table = t;
    }
    return table;
}
// the slab's histograms | the table of the largest slab
extern "C" size_t trc_planes_advise_obatch_work_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk)
{
    if (trc_planes_batch_plan_quiet(items, count, esize, chunk, nullptr, nullptr) || !trc_planes_batch_ptrs_ok(items, 0, count)) return 0;
    return TRC_PLANES_ADVISE_SLAB_BYTES + advise_otable_bytes(items, count, esize, chunk);
}

// the order per item under the caller's strides: the slab walk of advise_batch_dev over trc_planes_hist_obatch_dev's histograms
extern "C" int trc_planes_advise_obatch_dev(unsigned orders, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize,
                                            uint32_t chunk, uint8_t *filters_out, uint8_t *orders_out, trc_planes_order_advice *advice,
                                            void *d_work, size_t work_bytes, void *stream)
{
    trc_planes_batch_plan B;
    int rc = trc_planes_batch_plan_host(items, count, esize, chunk, &B, nullptr);
    if (rc) return rc;
    if (orders < 1 || orders > 15) return fail(TRC_E_ARG, "planes_advise_obatch: orders 0x%x (a bit set: bit k = order k, 1 .. 15)", orders);
    if ((rc = trc_planes_batch_strides("planes_advise_obatch", nullptr, strides, count, nullptr))) return rc;
    if (!filters_out || !orders_out) return fail(TRC_E_ARG, "planes_advise_obatch: null filters_out or orders_out");
    if (!trc_planes_batch_ptrs_ok(items, 0, count)) return fail(TRC_E_ARG, "planes_advise_obatch: every item's pointer must be non-null and 16-byte aligned");
    if (!d_work || ((uintptr_t)d_work & 255)) return fail(TRC_E_ARG, "planes_advise_obatch: the workspace must be 256-byte aligned");
    const size_t table = advise_otable_bytes(items, count, esize, chunk), need = TRC_PLANES_ADVISE_SLAB_BYTES + table;
    if (work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    const size_t slab = advise_oslab_items(esize), slice = (size_t)4 * esize * 256;
    hipStream_t s = (hipStream_t)stream;
    uint64_t *d_hist = (uint64_t *)d_work;
    std::vector<uint64_t> hist((count < slab ? count : slab) * slice);
    std::vector<uint8_t> choice(count);
    std::vector<trc_planes_order_advice> adv(advice ? count : 0);
    for (size_t i0 = 0; i0 < count; i0 += slab) {
        const size_t cnt = count - i0 < slab ? count - i0 : slab;
        if ((rc = trc_planes_hist_obatch_run(orders, items, strides, i0, cnt, esize, chunk, d_hist, (uint8_t *)d_work + TRC_PLANES_ADVISE_SLAB_BYTES, table, s))) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        HIPCHK(hipMemcpyAsync(hist.data(), d_hist, cnt * slice * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if ((rc = advise_order_items(hist.data(), orders, esize, items, i0, cnt, choice.data(), advice ? adv.data() : nullptr))) return rc;
    }
    if (advice) memcpy(advice, adv.data(), count * sizeof *advice);
    advise_order_out(choice, filters_out, orders_out);
    return TRC_OK;
}
