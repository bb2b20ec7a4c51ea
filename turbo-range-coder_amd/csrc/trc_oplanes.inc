// trc_oplanes.inc -- the coded planes calls behind a predictor of ORDER 0 .. 3 (included by trc_api.hip behind trc_splanes.inc): the
// device-resident calls, which are those of trc_planes.inc with the split / join of trc_oplanes.hip where the order is 2 or 3, the
// order advisor's host half, and the TRCO container, which is the TRCS container with the order where that one has its filter.
// Nothing here knows a coder or a kernel.
int trc_planes_order_arg(const char *who, int order, int stride);       // trc_oplanes.hip: the order, then the stride, ahead of everything else

// order 0 is the unfiltered call, order 1 the strided zigzag delta
static PlanesPred pred_order(int order, int stride)
{
    if (order == 0) return pred_none();
    PlanesPred p = pred_stride(TRC_FILTER_ZDELTA, stride);
    p.order = order;
    return p;
}

extern "C" int trc_encode_oplanes_dev(int codec, int order, int stride, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                                      uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                      uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                                      void *d_work, size_t work_bytes, void *stream)
{
    const int rc = trc_planes_order_arg("encode_oplanes", order, stride);
    if (rc) return rc;
    return planes_encode_dev(codec, pred_order(order, stride), d_in, n, esize, chunk, d_cdf, cdfnum, d_status,
                             d_clen, d_payload, d_total, d_tail, d_work, work_bytes, stream);
}

extern "C" int trc_decode_oplanes_dev(int codec, int order, int stride, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                                      size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                      void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const int rc = trc_planes_order_arg("decode_oplanes", order, stride);
    if (rc) return rc;
    return planes_decode_dev(codec, pred_order(order, stride), d_clen, d_payload, d_tail, n, esize, chunk, d_cdf, cdfnum,
                             d_out, d_work, work_bytes, stream);
}

extern "C" int trc_decode_oplanes_range_dev(int codec, int order, int stride, const uint32_t *d_clen, const void *d_payload,
                                            size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                            const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const int rc = trc_planes_order_arg("decode_oplanes_range", order, stride);
    if (rc) return rc;
    return planes_decode_range_dev(codec, pred_order(order, stride), d_clen, d_payload, n, esize, chunk, first_chunk, count,
                                   d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}

// ---- the order advisor's host half: the estimates of trc_planes_advise over the rows of trc_planes_hist_order_dev, and a choice ----
extern "C" int trc_planes_advise_order(const uint64_t *hist, unsigned orders, unsigned esize, size_t m, trc_planes_order_advice *a)
{
    if (!hist || !a) return fail(TRC_E_ARG, "planes_advise_order: null histogram or advice");
    if (orders < 1 || orders > 15) return fail(TRC_E_ARG, "planes_advise_order: orders 0x%x (a bit set: bit k = order k, 1 .. 15)", orders);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "planes_advise_order: esize %u (2, 4 or 8)", esize);
    if (!m) return fail(TRC_E_ARG, "planes_advise_order: no element");
    memset(a, 0, sizeof *a);
    a->esize = esize; a->orders = orders; a->m = m;
    int best = -1;
    for (unsigned f = 0; f <= TRC_ORDER_MAX; f++) {
        if (!(orders >> f & 1)) continue;
        for (unsigned k = 0; k < esize; k++) {
            const uint64_t *row = hist + ((size_t)f * esize + k) * 256;
            uint64_t sum = 0;
            double bits = 0;
            for (unsigned b = 0; b < 256; b++) {
                const uint64_t c = row[b];
                if (c > m - sum) return fail(TRC_E_ARG, "planes_advise_order: order %u plane %u counts more than the %zu elements", f, k, m);
                sum += c;
                if (c) bits += (double)c * log2((double)m / (double)c);
            }
            if (sum != m) return fail(TRC_E_ARG, "planes_advise_order: order %u plane %u counts %llu elements of %zu", f, k, (unsigned long long)sum, m);
            a->bits[f][k] = bits;
            a->total_bits[f] += bits;
        }
        if (best < 0 || a->total_bits[f] < a->total_bits[best]) best = (int)f;       // (ties: the lower order)
    }
    // an order is never a default: it has to save 1/64 of the unfiltered total to be chosen over no filter
    if ((orders & 1) && best != 0 && a->total_bits[0] - a->total_bits[best] < a->total_bits[0] / 64) best = 0;
    a->order = best;
    return TRC_OK;
}

// ---- the TRCO container: trc_oplanes_hdr (16 B) | the TRCP container of O(order, stride, chunk, esize, in) -------------------------
extern "C" size_t trc_oplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_bound(n, esize, chunk, cdfnum);
    return b ? b + sizeof(trc_oplanes_hdr) : 0;
}

// the prefix alone: 0 and the header, or TRC_E_ARG with the reason set
static int oplanes_prefix(const void *buf, size_t buflen, trc_oplanes_hdr &h)
{
    const char *noun = "order planes container";
    if (!buf || buflen < sizeof h) return fail(TRC_E_ARG, "%s: %zu bytes is shorter than the header", noun, buflen);
    memcpy(&h, buf, sizeof h);
    if (h.magic != TRC_OPLANES_MAGIC || h.version != 1) return fail(TRC_E_ARG, "%s: bad magic/version", noun);
    if (h.order < 2 || h.order > TRC_ORDER_MAX) return fail(TRC_E_ARG, "%s: order %u (2 .. %d)", noun, h.order, TRC_ORDER_MAX);
    if (h.stride < 1 || h.stride > TRC_STRIDE_MAX) return fail(TRC_E_ARG, "%s: stride %u (1 .. %d)", noun, h.stride, TRC_STRIDE_MAX);
    if (h.size > buflen) return fail(TRC_E_ARG, "%s: states %llu bytes, the buffer holds %zu", noun, (unsigned long long)h.size, buflen);
    if (h.size <= sizeof h) return fail(TRC_E_ARG, "%s: size %llu leaves no room behind the header", noun, (unsigned long long)h.size);
    return TRC_OK;
}
extern "C" int trc_oplanes_check(const void *buf, size_t buflen, size_t outlen)
{
    trc_oplanes_hdr h;
    const int rc = oplanes_prefix(buf, buflen, h);
    return rc ? rc : trc_planes_check((const uint8_t *)buf + sizeof h, (size_t)h.size - sizeof h, outlen);
}

extern "C" size_t trc_encode_oplanes_host(int codec, int order, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                          void *out, size_t outcap, unsigned cdfnum)
{
    if (trc_planes_order_arg("encode_oplanes_host", order, stride)) return 0;
    if (order == 0) { fail(TRC_E_ARG, "encode_oplanes_host: order 0 is unfiltered data, which goes through trc_encode_planes_host (one layout per content)"); return 0; }
    if (order == 1) {
        fail(TRC_E_ARG, "encode_oplanes_host: order 1 is the zigzag delta, which goes through %s (one layout per content)",
             stride == 1 ? "trc_encode_fplanes_host" : "trc_encode_splanes_host");
        return 0;
    }
    if (!out || outcap <= sizeof(trc_oplanes_hdr)) { fail(TRC_E_ARG, "encode_oplanes_host: out holds %zu bytes (trc_oplanes_bound)", outcap); return 0; }
    const PlanesPred pred = pred_order(order, stride);
    const size_t inner = planes_host_encode(codec, pred, false, in, n, esize, chunk, (uint8_t *)out + sizeof(trc_oplanes_hdr), outcap - sizeof(trc_oplanes_hdr), cdfnum,
                                            nullptr, nullptr);
    if (!inner) return 0;
    planes_lead_write(pred, (uint8_t *)out, sizeof(trc_oplanes_hdr) + inner);
    return sizeof(trc_oplanes_hdr) + inner;
}

// (the prefix is checked here, the inner container by the planes decoders: together trc_oplanes_check, ahead of anything else)
extern "C" size_t trc_decode_oplanes_host(const void *in, size_t inlen, void *out, size_t outlen)
{
    trc_oplanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_oplanes_host: bad arguments"); return 0; }
    if (oplanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_all(pred_order(h.order, h.stride), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, out, outlen, nullptr);
}

extern "C" size_t trc_decode_oplanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out)
{
    trc_oplanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_oplanes_range_host: bad arguments"); return 0; }
    if (oplanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_bytes(pred_order(h.order, h.stride), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, offset, len, out);
}

// the advisor among the orders at the caller's stride: one upload, the histograms of orders 0 .. 3, the coded call on the bytes on
// the device, behind the prefix of the explicit call for the choice
extern "C" size_t trc_encode_aoplanes_host(int codec, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                           void *out, size_t outcap, unsigned cdfnum, trc_planes_order_advice *advice)
{
    if (stride_common("encode_aoplanes_host", stride)) return 0;
    return planes_host_encode(codec, pred_stride(TRC_FILTER_ZDELTA, stride), true, in, n, esize, chunk, out, outcap, cdfnum, nullptr, nullptr, advice, true);
}
