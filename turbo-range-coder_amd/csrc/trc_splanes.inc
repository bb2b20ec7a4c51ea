// trc_splanes.inc -- the coded planes calls behind a STRIDED predictor filter (included by trc_api.hip behind trc_planes.inc): the
// device-resident calls, which are those of trc_planes.inc with the strided split / join of trc_fplanes.hip, and the TRCS container, which
// is the TRCF container with the stride where that one has its reserved field.  Nothing here knows a coder or a kernel.

// the stride is looked at ahead of everything else, pointers included
static int stride_common(const char *who, int stride)
{
    if (stride < 1 || stride > TRC_STRIDE_MAX) return fail(TRC_E_ARG, "%s: stride %d (1 .. %d)", who, stride, TRC_STRIDE_MAX);
    return TRC_OK;
}

extern "C" int trc_encode_splanes_dev(int codec, int filter, int stride, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                                      uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                      uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                                      void *d_work, size_t work_bytes, void *stream)
{
    const int rc = stride_common("encode_splanes", stride);
    if (rc) return rc;
    return planes_encode_dev(codec, pred_stride(filter, stride), d_in, n, esize, chunk, d_cdf, cdfnum, d_status,
                             d_clen, d_payload, d_total, d_tail, d_work, work_bytes, stream);
}

extern "C" int trc_decode_splanes_dev(int codec, int filter, int stride, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                                      size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                      void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const int rc = stride_common("decode_splanes", stride);
    if (rc) return rc;
    return planes_decode_dev(codec, pred_stride(filter, stride), d_clen, d_payload, d_tail, n, esize, chunk, d_cdf, cdfnum,
                             d_out, d_work, work_bytes, stream);
}

extern "C" int trc_decode_splanes_range_dev(int codec, int filter, int stride, const uint32_t *d_clen, const void *d_payload,
                                            size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                            const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const int rc = stride_common("decode_splanes_range", stride);
    if (rc) return rc;
    return planes_decode_range_dev(codec, pred_stride(filter, stride), d_clen, d_payload, n, esize, chunk, first_chunk, count,
                                   d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}

// ---- the TRCS container: trc_splanes_hdr (16 B) | the TRCP container of the strided-filtered data ---------------------------------
extern "C" size_t trc_splanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_bound(n, esize, chunk, cdfnum);
    return b ? b + sizeof(trc_splanes_hdr) : 0;
}

// the prefix alone: 0 and the header, or TRC_E_ARG with the reason set
static int splanes_prefix(const void *buf, size_t buflen, trc_splanes_hdr &h)
{
    return planes_prefix("strided planes container", TRC_SPLANES_MAGIC, buf, buflen, h, [](const trc_splanes_hdr &t) {
        return t.stride < 2 || t.stride > TRC_STRIDE_MAX ? fail(TRC_E_ARG, "strided planes container: stride %u (2 .. %d)", t.stride, TRC_STRIDE_MAX) : (int)TRC_OK; });
}
extern "C" int trc_splanes_check(const void *buf, size_t buflen, size_t outlen)
{
    trc_splanes_hdr h;
    const int rc = splanes_prefix(buf, buflen, h);
    return rc ? rc : trc_planes_check((const uint8_t *)buf + sizeof h, (size_t)h.size - sizeof h, outlen);
}

extern "C" size_t trc_encode_splanes_host(int codec, int filter, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                          void *out, size_t outcap, unsigned cdfnum)
{
    if (stride_common("encode_splanes_host", stride)) return 0;
    if (filter != TRC_FILTER_ZDELTA && filter != TRC_FILTER_XOR) {
        fail(TRC_E_ARG, "encode_splanes_host: filter %d (1 zigzag delta, 2 xor; unfiltered data goes through trc_encode_planes_host)", filter);
        return 0;
    }
    if (stride == 1) { fail(TRC_E_ARG, "encode_splanes_host: stride 1 goes through trc_encode_fplanes_host (one layout per content)"); return 0; }
    if (!out || outcap <= sizeof(trc_splanes_hdr)) { fail(TRC_E_ARG, "encode_splanes_host: out holds %zu bytes (trc_splanes_bound)", outcap); return 0; }
    const size_t inner = planes_host_encode(codec, pred_stride(filter, stride), false, in, n, esize, chunk, (uint8_t *)out + sizeof(trc_splanes_hdr), outcap - sizeof(trc_splanes_hdr), cdfnum, nullptr, nullptr);
    if (!inner) return 0;
    trc_splanes_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_SPLANES_MAGIC; h.filter = (uint8_t)filter; h.version = 1; h.stride = (uint16_t)stride; h.size = sizeof h + inner;
    memcpy(out, &h, sizeof h);
    return (size_t)h.size;
}

// (the prefix is checked here, the inner container by the planes decoders: together trc_splanes_check, ahead of anything else)
extern "C" size_t trc_decode_splanes_host(const void *in, size_t inlen, void *out, size_t outlen)
{
    trc_splanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_splanes_host: bad arguments"); return 0; }
    if (splanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_all(pred_stride(h.filter, h.stride), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, out, outlen, nullptr);
}

extern "C" size_t trc_decode_splanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out)
{
    trc_splanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_splanes_range_host: bad arguments"); return 0; }
    if (splanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_bytes(pred_stride(h.filter, h.stride), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, offset, len, out);
}
