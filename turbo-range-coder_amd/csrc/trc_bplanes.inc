// trc_bplanes.inc -- the coded planes calls behind a filter against a BASE buffer (included by trc_api.hip behind trc_splanes.inc): the
// device-resident calls, which are those of trc_planes.inc with the elementwise split / join of trc_bplanes.hip, and the TRCD
// container, which is the TRCP container of D(filter, esize, in, base) behind a prefix that names the base by length and
// fingerprint.  Nothing here knows a coder or a kernel.

// (TRC_FILTER_NONE: the unfiltered call, which is told nothing of the base)
extern "C" int trc_encode_bplanes_dev(int codec, int filter, const void *d_in, const void *d_base, size_t n, unsigned esize, uint32_t chunk,
                                      uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                      uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                                      void *d_work, size_t work_bytes, void *stream)
{
    return planes_encode_dev(codec, pred_base(filter, d_base), d_in, n, esize, chunk, d_cdf, cdfnum, d_status,
                             d_clen, d_payload, d_total, d_tail, d_work, work_bytes, stream);
}

extern "C" int trc_decode_bplanes_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                                      const void *d_base, size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                      void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return planes_decode_dev(codec, pred_base(filter, d_base), d_clen, d_payload, d_tail, n, esize, chunk, d_cdf, cdfnum,
                             d_out, d_work, work_bytes, stream);
}

extern "C" int trc_decode_bplanes_range_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_base,
                                            size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                            const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return planes_decode_range_dev(codec, pred_base(filter, d_base), d_clen, d_payload, n, esize, chunk, first_chunk, count,
                                   d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}

// ---- the TRCD container: trc_bplanes_hdr (32 B) | the TRCP container of the data filtered against the base -------------------------
extern "C" size_t trc_bplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_bound(n, esize, chunk, cdfnum);
    return b ? b + sizeof(trc_bplanes_hdr) : 0;
}

// the whole check: 0 and the prefix, or TRC_E_ARG with the reason set
static int bplanes_verdict(const void *buf, size_t buflen, size_t outlen, trc_bplanes_hdr &h)
{
    int rc = planes_prefix("base planes container", TRC_BPLANES_MAGIC, buf, buflen, h, [](const trc_bplanes_hdr &d) {
        return d.zero ? fail(TRC_E_ARG, "base planes container: reserved field is 0x%x, must be 0", d.zero) : (int)TRC_OK; });
    if (rc) return rc;
    rc = trc_planes_check((const uint8_t *)buf + sizeof h, (size_t)h.size - sizeof h, outlen);
    if (rc) return rc;
    trc_planes_hdr p;
    memcpy(&p, (const uint8_t *)buf + sizeof h, sizeof p);
    if (h.base_bytes != p.n - p.tail)
        return fail(TRC_E_ARG, "base planes container: base_bytes %llu, the elements take %llu", (unsigned long long)h.base_bytes, (unsigned long long)(p.n - p.tail));
    return TRC_OK;
}
extern "C" int trc_bplanes_check(const void *buf, size_t buflen, size_t outlen)
{
    trc_bplanes_hdr h;
    return bplanes_verdict(buf, buflen, outlen, h);
}

extern "C" size_t trc_encode_bplanes_host(int codec, int filter, const void *in, const void *base, size_t n, unsigned esize, uint32_t chunk,
                                          void *out, size_t outcap, unsigned cdfnum)
{
    if (filter != TRC_FILTER_ZDELTA && filter != TRC_FILTER_XOR) {
        fail(TRC_E_ARG, "encode_bplanes_host: filter %d (1 zigzag delta, 2 xor; unfiltered data goes through trc_encode_planes_host)", filter);
        return 0;
    }
    if (!base) { fail(TRC_E_ARG, "encode_bplanes_host: no base"); return 0; }
    if (!out || outcap <= sizeof(trc_bplanes_hdr)) { fail(TRC_E_ARG, "encode_bplanes_host: out holds %zu bytes (trc_bplanes_bound)", outcap); return 0; }
    uint64_t fp = 0;
    const size_t inner = planes_host_encode(codec, pred_base(filter, base), false, in, n, esize, chunk, (uint8_t *)out + sizeof(trc_bplanes_hdr), outcap - sizeof(trc_bplanes_hdr), cdfnum, nullptr, &fp);
    if (!inner) return 0;
    trc_bplanes_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_BPLANES_MAGIC; h.filter = (uint8_t)filter; h.version = 1; h.size = sizeof h + inner;
    h.base_bytes = n - n % esize; h.base_fp = fp;
    memcpy(out, &h, sizeof h);
    return (size_t)h.size;
}

// what both decoders look at before a device: the container, then the base
static int bplanes_decode_args(const char *who, const void *in, size_t inlen, const void *base, size_t base_len, const void *out, size_t outlen, trc_bplanes_hdr &h)
{
    if (!in || !out) return fail(TRC_E_ARG, "%s: bad arguments", who);
    const int rc = bplanes_verdict(in, inlen, outlen, h);
    if (rc) return rc;
    if (!base || base_len < h.base_bytes)
        return fail(TRC_E_ARG, "%s: the base holds %zu bytes, the container was made against %llu", who, base ? base_len : (size_t)0, (unsigned long long)h.base_bytes);
    return TRC_OK;
}

extern "C" size_t trc_decode_bplanes_host(const void *in, size_t inlen, const void *base, size_t base_len, void *out, size_t outlen)
{
    trc_bplanes_hdr h;
    if (bplanes_decode_args("decode_bplanes_host", in, inlen, base, base_len, out, outlen, h)) return 0;
    return planes_host_decode_all(pred_base(h.filter, base), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, out, outlen, &h.base_fp);
}

// (no fingerprint here: the call uploads the covering elements of the base and never sees the rest)
extern "C" size_t trc_decode_bplanes_range_host(const void *in, size_t inlen, const void *base, size_t base_len,
                                                size_t offset, size_t len, void *out)
{
    trc_bplanes_hdr h;
    if (bplanes_decode_args("decode_bplanes_range_host", in, inlen, base, base_len, out, (size_t)-1, h)) return 0;
    return planes_host_decode_bytes(pred_base(h.filter, base), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, offset, len, out);
}
