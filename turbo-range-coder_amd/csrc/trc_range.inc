// trc_range.inc -- a byte range of a TRC1 container through host pointers (included by trc_api.hip behind trc_host.inc and the
// container checks): the plan on the host, then only the covering chunks' directory entries and payload cross the link.

// the plan for bytes [offset, offset + len) of a container that container_verdict has accepted; 0 < len, offset + len <= h.n
static void range_plan(const uint8_t *buf, const trc_container_hdr &h, size_t offset, size_t len, trc_range *r)
{
    const uint64_t first = offset / h.chunk, last = (offset + len - 1) / h.chunk;
    const uint8_t *d = buf + sizeof h;
    uint64_t sum = 0, before = 0;
    for (uint64_t c = 0; c <= last; c++) {
        if (c == first) before = sum;
        uint32_t l; memcpy(&l, d + 4 * (size_t)c, 4);
        const uint64_t clen = (c + 1 == h.nchunks) ? h.n - c * h.chunk : h.chunk;
        sum += l < clen ? l : clen;                             // the clamp of container_verdict and of the decoders
    }
    const uint64_t end = (last + 1) * h.chunk < h.n ? (last + 1) * h.chunk : h.n;
    r->first_chunk = first; r->nchunks = last - first + 1;
    r->payload_off = before; r->payload_len = sum - before;
    r->out_skip = offset - first * h.chunk; r->out_bytes = end - first * h.chunk;
}

extern "C" int trc_container_range(const void *buf, size_t buflen, int codec, size_t offset, size_t len, trc_range *r)
{
    if (!r) return fail(TRC_E_ARG, "container_range: bad arguments");
    if (trc_container_check(buf, buflen, codec, (size_t)-1)) return TRC_E_ARG;
    trc_container_hdr h;
    memcpy(&h, buf, sizeof h);
    if (!len || offset > h.n || len > h.n - offset)
        return fail(TRC_E_ARG, "container_range: bytes [%zu, %zu + %zu) of %llu", offset, offset, len, (unsigned long long)h.n);
    range_plan((const uint8_t *)buf, h, offset, len, r);
    return TRC_OK;
}

// The covering chunks travel as a container of their own: clen[first .. first + nchunks) and their payload_len payload bytes go up,
// one plain trc_decode_dev of (out_bytes, chunk) runs on the caller's current device (its context of the host-pointer calls: its
// buffers, its first coder stream), `len` bytes come back.  One copy each way and one launch: no slices, no staging threads.
static size_t host_decode_range(int codec, const uint8_t *in, const trc_container_hdr &h, const trc_range &R, size_t len, uint8_t *out,
                                const cdf_t *cdf, int cdfnum, unsigned prm)
{
    HostCtx *cp = nullptr;
    int dev = 0;
    if (ctx_get(cp)) return 0;
    if (hipGetDevice(&dev) != hipSuccess) { fail(TRC_E_HIP, "hipGetDevice failed"); return 0; }
    HostCtx &c = *cp;
    std::lock_guard<std::mutex> lk(c.mu);
    if (ctx_init(c, dev)) return 0;
    const size_t dirsz = up256(4 * (size_t)R.nchunks + 256);
    if (grow(&c.d_in, &c.cap_in, (size_t)R.out_bytes) || grow(&c.d_cont, &c.cap_cont, dirsz + (size_t)R.payload_len + 64) ||
        grow(&c.d_work[0], &c.cap_work[0], trc_work_bytes(codec, (size_t)R.out_bytes, h.chunk))) return 0;
    hipStream_t s = c.s_k[0];
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + dirsz;
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    const uint8_t *dir = in + sizeof h, *pay = dir + 4 * (size_t)h.nchunks;
    // (a failure leaves with the stream drained: the copies below read and write the caller's memory)
#define RCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail(TRC_E_HIP, "%s -> %s", #x, hipGetErrorString(e_)); (void)hipStreamSynchronize(s); return 0; } } while (0)
    if (cdfnum) RCHK(hipMemcpyAsync(d_cdf, cdf, (cdfnum + 1) * sizeof(cdf_t), hipMemcpyHostToDevice, s));
    RCHK(hipMemcpyAsync(d_clen, dir + 4 * (size_t)R.first_chunk, 4 * (size_t)R.nchunks, hipMemcpyHostToDevice, s));
    if (R.payload_len) RCHK(hipMemcpyAsync(d_payload, pay + R.payload_off, (size_t)R.payload_len, hipMemcpyHostToDevice, s));
    if (trc_decode_dev(codec, d_clen, d_payload, (size_t)R.out_bytes, h.chunk, cdfnum ? d_cdf : nullptr, cdfnum ? (unsigned)cdfnum : prm,
                       c.d_in, c.d_work[0], c.cap_work[0], s)) { (void)hipStreamSynchronize(s); return 0; }
    RCHK(hipMemcpyAsync(out, c.d_in + R.out_skip, len, hipMemcpyDeviceToHost, s));
    RCHK(hipStreamSynchronize(s));
#undef RCHK
    return len;
}

extern "C" size_t trc_decode_range_host(int codec, const void *in, size_t inlen, size_t n, size_t offset, size_t len, void *out,
                                        const uint16_t *cdf, unsigned cdfnum)
{
    if (!codec_ok(codec)) { fail(TRC_E_ARG, "codec %d not available", codec); return 0; }
    if (!in || !out) { fail(TRC_E_ARG, "decode_range_host: bad arguments"); return 0; }
    if (!len || offset > n || len > n - offset) { fail(TRC_E_ARG, "decode_range_host: bytes [%zu, %zu + %zu) of %zu", offset, offset, len, n); return 0; }
    // inlen == n: stored raw unless it validates as a container of this coder and length (trc_decode_host has the reasons)
    char why[200];
    if (inlen == n && container_verdict(in, inlen, codec, n, why, sizeof why)) { memcpy(out, (const uint8_t *)in + offset, len); return len; }
    if (inlen != n && trc_container_check(in, inlen, codec, n)) return 0;
    trc_container_hdr h;
    memcpy(&h, in, sizeof h);
    int ncdf = 0;
    if (codec_row(codec).cdf) {
        ncdf = (int)cdfnum > 0 ? (int)cdfnum : host_cdfnum((const cdf_t *)cdf);
        if (!cdf || ncdf <= 0 || ncdf > 256) { fail(TRC_E_CDF, "bad CDF"); return 0; }
    }
    unsigned prm = 0;
    if (codec_row(codec).ss) {                                  // the header's parameters; a caller that states its own must state the same
        if (cdfnum && cdfnum != h.cdfnum) { fail(TRC_E_ARG, "codec %d: the container was coded with parameters 0x%x, the caller states 0x%x", codec, h.cdfnum, cdfnum); return 0; }
        prm = h.cdfnum;
    }
    trc_range R;
    range_plan((const uint8_t *)in, h, offset, len, &R);
    return host_decode_range(codec, (const uint8_t *)in, h, R, len, (uint8_t *)out, (const cdf_t *)cdf, ncdf, prm);
}
