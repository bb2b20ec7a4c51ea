// trc_planes.inc -- byte-plane containers of 16 / 32 / 64-bit elements (included by trc_api.hip behind trc_range.inc): the
// device-resident calls that put the split / join kernels (trc_planes.hip) around one trc_encode_dev / trc_decode_dev /
// trc_decode_range_dev PER PLANE, the TRCP container check, and the plain host-pointer calls on top of them.
//
// Nothing here knows a coder: plane k's (clen, payload, total) is what trc_encode_dev returns for the m bytes of plane k, so every
// contract of the per-plane calls (chunk parity, raw fallback, random access) holds for each plane as it stands.
// One property of a coder is asked for: the seven low-nibble coders (TrcCodec::low4) code in[i] & 15 and never store raw, so planes
// coded with them would come back without their high nibbles.  Every entry point here refuses them, with PLANES_LOW4 as the reason.
#include <math.h>
#define PLANES_LOW4 "codec %d keeps only the low four bits of a byte: the byte-plane calls do not take it"

// ---- workspace -------------------------------------------------------------------------------------------------------------------
// esize slices, `slice` bytes apart (a multiple of 256, so the slices are the planes of the split / join kernels with pitch = slice):
//   plane k: [ plane buffer: `buf` bytes = the plane + TRC_PAD, rounded up to 256 | the per-plane call's own workspace: `work` bytes ]
struct PlanesMap { size_t m, nc, buf, work, slice; };
static bool planes_esize_ok(unsigned esize) { return esize == 2 || esize == 4 || esize == 8; }
static bool planes_map(int codec, size_t n, unsigned esize, uint32_t chunk, PlanesMap &P)
{
    const TrcCodec &r = codec_row(codec);
    if (!r.enc || r.low4 || !planes_esize_ok(esize) || n < esize || !chunk_ok(chunk) || chunk > r.chunk_max) return false;
    P.m = n / esize;
    P.nc = (P.m + chunk - 1) / chunk;
    if (P.nc > 0x7fffffffu) return false;
    P.buf = trc_planes_pitch(n, esize);
    P.work = up256(trc_work_bytes(codec, P.m, chunk));
    P.slice = P.buf + P.work;
    return true;
}
extern "C" size_t trc_planes_work_bytes(int codec, size_t n, unsigned esize, uint32_t chunk)
{
    PlanesMap P;
    return planes_map(codec, n, esize, chunk, P) ? esize * P.slice : 0;
}
// the range form: the plane buffer holds `count` chunks, the per-plane workspace is the one of trc_decode_range_dev
static bool planes_range_map(int codec, size_t n, unsigned esize, uint32_t chunk, size_t count, PlanesMap &P)
{
    if (codec_row(codec).low4 || !planes_esize_ok(esize) || n < esize) return false;
    P.m = n / esize;
    P.work = up256(trc_range_work_bytes(codec, P.m, chunk, count));
    if (!P.work) return false;
    P.nc = (P.m + chunk - 1) / chunk;
    P.buf = up256(count * (size_t)chunk + TRC_PAD);
    P.slice = P.buf + P.work;
    return true;
}
extern "C" size_t trc_planes_range_work_bytes(int codec, size_t n, unsigned esize, uint32_t chunk, size_t count)
{
    PlanesMap P;
    return planes_range_map(codec, n, esize, chunk, count, P) ? esize * P.slice : 0;
}

// what the three planar calls check themselves; everything else is checked by the per-plane calls
static int planes_common(const char *who, int codec, size_t n, unsigned esize, const void *d_work)
{
    if (codec & (TRC_TABLES_READY | TRC_DIR_READY)) return fail(TRC_E_ARG, "%s: TRC_TABLES_READY / TRC_DIR_READY do not apply to planes", who);
    if (codec_row(codec).low4) return fail(TRC_E_ARG, "%s: " PLANES_LOW4, who, codec);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "%s: esize %u (2, 4 or 8)", who, esize);
    if (n < esize) return fail(TRC_E_ARG, "%s: %zu bytes hold no element of %u bytes", who, n, esize);
    if (!d_work || ((uintptr_t)d_work & 255)) return fail(TRC_E_ARG, "%s: workspace must be 256-byte aligned", who);
    return TRC_OK;
}

// The three calls with a filter (trc_fplanes.hip) between the elements and the planes; with TRC_FILTER_NONE the filter forms of split
// and join are the plain ones.  The restart length is the chunk, which check_common has vetted by the time split or join see it.
int trc_planes_filter_arg(const char *who, int filter);     // trc_fplanes.hip: the filter id, with the text of the split / join calls

// How a flat call predicts its elements.  The strided forms (trc_fplanes.hip, trc_splanes.inc) are the same three calls with another
// split / join: stride 1 is the fplanes call, whose kernels it launches, and the stride itself is vetted by trc_splanes.inc before it
// gets here.  based: the filter is against a BASE buffer (trc_bplanes.hip), whose split and join are elementwise and have no restart;
// what can be said about the base is said before anything is enqueued.  `base` is a device pointer for the *_dev calls and a host
// pointer for the host-pointer calls, which upload it.  An unfiltered call is told nothing of stride or base.  order: how many times
// the strided zigzag delta is taken (trc_oplanes.hip has the kernels of orders 2 and 3); every filter above is of order 1.
struct PlanesPred { int filter, stride; const void *base; bool based; int order = 1; };
static PlanesPred pred_none() { return PlanesPred{ TRC_FILTER_NONE, 1, nullptr, false }; }
static PlanesPred pred_stride(int filter, int stride) { return PlanesPred{ filter, filter == TRC_FILTER_NONE ? 1 : stride, nullptr, false }; }
static PlanesPred pred_base(int filter, const void *base)
{
    const bool none = filter == TRC_FILTER_NONE;
    return PlanesPred{ filter, 1, none ? nullptr : base, !none };
}
// the same predictor for the elements that start `bytes` into the buffer
static PlanesPred pred_from(PlanesPred p, size_t bytes) { if (p.base) p.base = (const uint8_t *)p.base + bytes; return p; }

int trc_bplanes_base_arg(const char *who, const void *d_base);          // trc_bplanes.hip
int trc_bplanes_overlap_arg(const char *who, const void *d_base, size_t base_bytes, const void *d_out, size_t n);
static int split_any(PlanesPred p, const void *d_in, size_t n, unsigned esize, uint32_t seg, void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    if (p.based) return trc_planes_split_base_dev(p.filter, d_in, p.base, n, esize, d_planes, pitch, d_tail, stream);
    if (p.order >= 2) return trc_planes_split_ofilter_dev(p.order, p.stride, d_in, n, esize, seg, d_planes, pitch, d_tail, stream);
    return p.stride == 1 ? trc_planes_split_filter_dev(p.filter, d_in, n, esize, seg, d_planes, pitch, d_tail, stream)
                         : trc_planes_split_sfilter_dev(p.filter, p.stride, d_in, n, esize, seg, d_planes, pitch, d_tail, stream);
}
static int join_any(PlanesPred p, const void *d_planes, size_t pitch, const void *d_tail, size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream)
{
    if (p.based) return trc_planes_join_base_dev(p.filter, d_planes, pitch, d_tail, p.base, n, esize, d_out, stream);
    if (p.order >= 2) return trc_planes_join_ofilter_dev(p.order, p.stride, d_planes, pitch, d_tail, n, esize, seg, d_out, stream);
    return p.stride == 1 ? trc_planes_join_filter_dev(p.filter, d_planes, pitch, d_tail, n, esize, seg, d_out, stream)
                         : trc_planes_join_sfilter_dev(p.filter, p.stride, d_planes, pitch, d_tail, n, esize, seg, d_out, stream);
}

static int planes_encode_dev(int codec, PlanesPred pred, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                             uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                             uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                             void *d_work, size_t work_bytes, void *stream)
{
    int rc = trc_planes_filter_arg("encode_planes", pred.filter);
    if (rc) return rc;
    if (pred.based && (rc = trc_bplanes_base_arg("encode_planes", pred.base))) return rc;
    if ((rc = planes_common("encode_planes", codec, n, esize, d_work))) return rc;
    PlanesMap P;
    if ((rc = check_common(codec, n / esize, chunk, d_cdf, cdfnum))) return rc;
    const TrcCodec &r = codec_row(codec);
    if (r.cdf && !d_status) return fail(TRC_E_ARG, "encode_planes: a static coder needs d_status (one int32 per plane)");
    if (!r.cdf && d_status) return fail(TRC_E_ARG, "encode_planes: codec %d builds no CDF: d_status must be NULL", codec);
    if (!planes_map(codec, n, esize, chunk, P)) return fail(TRC_E_ARG, "encode_planes: bad (codec, n, esize, chunk)");
    if (work_bytes < esize * P.slice) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, esize * P.slice);
    if (!d_clen || !d_payload || !d_total || ((uintptr_t)d_payload & 1) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_total & 7))
        return fail(TRC_E_ARG, "encode_planes: d_clen must be 4-byte, d_payload 2-byte, d_total 8-byte aligned");
    uint8_t *w = (uint8_t *)d_work;
    if ((rc = split_any(pred, d_in, n, esize, chunk, w, P.slice, d_tail, stream))) return rc;
    for (unsigned k = 0; k < esize; k++) {
        uint8_t *plane = w + k * P.slice, *pw = plane + P.buf;
        uint16_t *cdf = r.cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr;
        if (r.cdf && (rc = trc_cdfini_dev(plane, P.m, cdf, cdfnum, d_status + k, pw, stream))) return rc;    // (the histogram bins open the plane's workspace; the encode's tables replace them)
        if ((rc = trc_encode_dev(codec, plane, P.m, chunk, cdf, cdfnum, d_clen + k * P.nc, (uint8_t *)d_payload + k * P.buf, d_total + k,
                                 pw, P.work, stream))) return rc;
    }
    return TRC_OK;
}
extern "C" int trc_encode_fplanes_dev(int codec, int filter, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                                      uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                      uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                                      void *d_work, size_t work_bytes, void *stream)
{
    return planes_encode_dev(codec, pred_stride(filter, 1), d_in, n, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total, d_tail, d_work, work_bytes, stream);
}

extern "C" int trc_encode_planes_dev(int codec, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                                     uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                     uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                                     void *d_work, size_t work_bytes, void *stream)
{
    return trc_encode_fplanes_dev(codec, TRC_FILTER_NONE, d_in, n, esize, chunk, d_cdf, cdfnum, d_status, d_clen, d_payload, d_total, d_tail,
                                  d_work, work_bytes, stream);
}

static int planes_decode_dev(int codec, PlanesPred pred, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                             size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                             void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    int rc = trc_planes_filter_arg("decode_planes", pred.filter);
    if (rc) return rc;
    if (pred.based && (rc = trc_bplanes_base_arg("decode_planes", pred.base))) return rc;
    if ((rc = planes_common("decode_planes", codec, n, esize, d_work))) return rc;
    PlanesMap P;
    if ((rc = check_common(codec, n / esize, chunk, d_cdf, cdfnum))) return rc;
    if (!planes_map(codec, n, esize, chunk, P)) return fail(TRC_E_ARG, "decode_planes: bad (codec, n, esize, chunk)");
    if (work_bytes < esize * P.slice) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, esize * P.slice);
    if (!d_out || ((uintptr_t)d_out & 15)) return fail(TRC_E_ARG, "decode_planes: d_out must be 16-byte aligned");
    if (n % esize && !d_tail) return fail(TRC_E_ARG, "decode_planes: %zu tail bytes and no tail buffer", n % esize);
    if (pred.based && (rc = trc_bplanes_overlap_arg("decode_planes", pred.base, P.m * esize, d_out, n))) return rc;
    const TrcCodec &r = codec_row(codec);
    uint8_t *w = (uint8_t *)d_work;
    for (unsigned k = 0; k < esize; k++) {
        uint8_t *plane = w + k * P.slice;
        if ((rc = trc_decode_dev(codec, d_clen + k * P.nc, (const uint8_t *)d_payload + k * P.buf, P.m, chunk,
                                 r.cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr, cdfnum, plane, plane + P.buf, P.work, stream))) return rc;
    }
    return join_any(pred, w, P.slice, d_tail, n, esize, chunk, d_out, stream);
}
extern "C" int trc_decode_fplanes_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                                      size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                      void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return planes_decode_dev(codec, pred_stride(filter, 1), d_clen, d_payload, d_tail, n, esize, chunk, d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}
extern "C" int trc_decode_planes_dev(int codec, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                                     size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                     void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return trc_decode_fplanes_dev(codec, TRC_FILTER_NONE, d_clen, d_payload, d_tail, n, esize, chunk, d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}

static int planes_decode_range_dev(int codec, PlanesPred pred, const uint32_t *d_clen, const void *d_payload,
                                   size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                   const uint16_t *d_cdf, unsigned cdfnum,
                                   void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    int rc = trc_planes_filter_arg("decode_planes_range", pred.filter);
    if (rc) return rc;
    if (pred.based && (rc = trc_bplanes_base_arg("decode_planes_range", pred.base))) return rc;
    if ((rc = planes_common("decode_planes_range", codec, n, esize, d_work))) return rc;
    const size_t m = n / esize;
    if ((rc = check_common(codec, m, chunk, d_cdf, cdfnum))) return rc;
    const size_t nc = (m + chunk - 1) / chunk;
    if (first_chunk > nc || count > nc - first_chunk)
        return fail(TRC_E_ARG, "decode_planes_range: chunks [%zu, %zu + %zu) of %zu", first_chunk, first_chunk, count, nc);
    if (count == 0) return TRC_OK;
    PlanesMap P;
    if (!planes_range_map(codec, n, esize, chunk, count, P)) return fail(TRC_E_ARG, "decode_planes_range: bad (codec, n, esize, chunk, count)");
    if (work_bytes < esize * P.slice) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, esize * P.slice);
    if (!d_out || ((uintptr_t)d_out & 15)) return fail(TRC_E_ARG, "decode_planes_range: d_out must be 16-byte aligned");
    const TrcCodec &r = codec_row(codec);
    const size_t pitch = trc_planes_pitch(n, esize);                     // the payload areas of the WHOLE container lie this far apart
    const size_t e0 = first_chunk * (size_t)chunk, e1 = (first_chunk + count) * (size_t)chunk;
    const size_t elems = (e1 < m ? e1 : m) - e0;
    const PlanesPred part = pred_from(pred, e0 * esize);                 // (the whole base is given: the range's part of it)
    if (part.based && (rc = trc_bplanes_overlap_arg("decode_planes_range", part.base, elems * esize, d_out, elems * esize))) return rc;
    uint8_t *w = (uint8_t *)d_work;
    for (unsigned k = 0; k < esize; k++) {
        uint8_t *plane = w + k * P.slice;
        if ((rc = trc_decode_range_dev(codec, d_clen + k * nc, (const uint8_t *)d_payload + k * pitch, m, chunk, first_chunk, count,
                                       r.cdf ? d_cdf + k * TRC_PLANES_CDF_STRIDE : nullptr, cdfnum, plane, plane + P.buf, P.work, stream))) return rc;
    }
    return join_any(part, w, P.slice, nullptr, elems * esize, esize, chunk, d_out, stream);       // (the range opens a segment)
}
extern "C" int trc_decode_fplanes_range_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload,
                                            size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                            const uint16_t *d_cdf, unsigned cdfnum,
                                            void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return planes_decode_range_dev(codec, pred_stride(filter, 1), d_clen, d_payload, n, esize, chunk, first_chunk, count, d_cdf, cdfnum, d_out, d_work, work_bytes, stream);
}
extern "C" int trc_decode_planes_range_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                           size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                           const uint16_t *d_cdf, unsigned cdfnum,
                                           void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    return trc_decode_fplanes_range_dev(codec, TRC_FILTER_NONE, d_clen, d_payload, n, esize, chunk, first_chunk, count, d_cdf, cdfnum,
                                        d_out, d_work, work_bytes, stream);
}

// ---- the TRCP container ----------------------------------------------------------------------------------------------------------
//   trc_planes_hdr (32 B) | uint64 off[esize] | section 0 .. esize - 1 | tail bytes
//   section k = [uint16 cdf[cdfnum + 1], zero-padded to a multiple of 8: static coders] | TRC1 container of plane k
static inline size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }
static inline size_t planes_cdf_bytes(const TrcCodec &r, unsigned cdfnum) { return r.cdf ? up8(2 * ((size_t)cdfnum + 1)) : 0; }

extern "C" size_t trc_planes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    if (!planes_esize_ok(esize) || n < esize || (chunk && !chunk_ok(chunk))) return 0;
    const size_t one = trc_container_bound(n / esize, chunk ? chunk : TRC_CHUNK_MIN);       // chunk 0: whatever the automatic rule picks
    const size_t cdf = cdfnum ? up8(2 * ((size_t)(cdfnum < 256 ? cdfnum : 256) + 1)) : 0;   // (an ss coder's parameters reserve a table nobody writes)
    return sizeof(trc_planes_hdr) + 8 * (size_t)esize + esize * (cdf + up8(one)) + 8;
}

// the verdict and, where it is good, the header; `why` as for container_verdict
static int planes_verdict(const void *buf, size_t buflen, size_t outlen, trc_planes_hdr &h, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, "planes container: " __VA_ARGS__); return TRC_E_ARG; } while (0)
    if (!buf || buflen < sizeof h) BAD("%zu bytes is shorter than the header", buflen);
    memcpy(&h, buf, sizeof h);
    if (h.magic != TRC_PLANES_MAGIC || h.version != 1) BAD("bad magic/version");
    if (!planes_esize_ok(h.esize)) BAD("esize %u (2, 4 or 8)", h.esize);
    if (!codec_ok(h.codec)) BAD("codec %u", h.codec);
    if (codec_row(h.codec).low4) BAD(PLANES_LOW4, (int)h.codec);      // (a section names the header's coder or is refused below)
    const TrcCodec &r = codec_row(h.codec);
    if (h.n < h.esize || h.tail != h.n % h.esize) BAD("tail %u of n = %llu, esize %u", h.tail, (unsigned long long)h.n, h.esize);
    if (outlen != (size_t)-1 && h.n != outlen) BAD("holds %llu bytes, caller expects %zu", (unsigned long long)h.n, outlen);
    if (!chunk_ok(h.chunk)) BAD("chunk %u", h.chunk);
    if (r.cdf ? (h.cdfnum < 1 || h.cdfnum > 256) : r.ss ? !ss_prm_ok(h.cdfnum) : h.cdfnum != 0) BAD("codec %u with cdfnum 0x%x", h.codec, h.cdfnum);
    const size_t front = sizeof h + 8 * (size_t)h.esize;
    if (h.size > buflen) BAD("states %llu bytes, the buffer holds %zu", (unsigned long long)h.size, buflen);
    if (h.size < front + h.tail) BAD("size %llu is shorter than header, offsets and tail", (unsigned long long)h.size);
    const uint8_t *b = (const uint8_t *)buf;
    const size_t m = (size_t)(h.n / h.esize), end = (size_t)h.size - h.tail, cdfb = planes_cdf_bytes(r, h.cdfnum);
    uint64_t off[8];
    memcpy(off, b + sizeof h, 8 * (size_t)h.esize);
    for (unsigned k = 0; k < h.esize; k++) {
        if (off[k] & 7) BAD("offset %u (%llu) is not a multiple of 8", k, (unsigned long long)off[k]);
        if (off[k] < (k ? off[k - 1] + sizeof(trc_container_hdr) : front) || off[k] > end) BAD("offset %u (%llu) out of order or outside the container", k, (unsigned long long)off[k]);
    }
    for (unsigned k = 0; k < h.esize; k++) {
        const size_t ext = (size_t)((k + 1 < h.esize ? off[k + 1] : end) - off[k]);
        const uint8_t *sec = b + off[k];
        if (ext < cdfb) BAD("section %u is shorter than its CDF", k);
        if (r.cdf) {
            uint16_t cdf[257];
            memcpy(cdf, sec, 2 * ((size_t)h.cdfnum + 1));
            if (cdf[0] != 0 || cdf[h.cdfnum] != TRC_PROB_ONE_HOST) BAD("section %u: the CDF must run from 0 to 32768", k);
            for (unsigned i = 1; i <= h.cdfnum; i++) if (cdf[i] <= cdf[i - 1]) BAD("section %u: the CDF is not strictly increasing at %u", k, i);
        }
        char sub[200];
        if (container_verdict(sec + cdfb, ext - cdfb, h.codec, m, sub, sizeof sub)) BAD("section %u: %s", k, sub);
        trc_container_hdr s;
        memcpy(&s, sec + cdfb, sizeof s);
        if (s.chunk != h.chunk || s.cdfnum != h.cdfnum) BAD("section %u: chunk %u / cdfnum 0x%x differ from the header's", k, s.chunk, s.cdfnum);
    }
    return TRC_OK;
#undef BAD
}
extern "C" int trc_planes_check(const void *buf, size_t buflen, size_t outlen)
{
    trc_planes_hdr h;
    char why[320];
    return planes_verdict(buf, buflen, outlen, h, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}

// ---- host pointers: plain calls on the caller's current device ---------------------------------------------------------------------
// One context (the one of the host-pointer calls: its buffers, its first coder stream), one copy up, the planar device call, the
// results back: no slices, no staging threads, no device list.
//   d_small: CDFs of the planes at 0 (8 x 528 B) | totals at 8192 | cdfini status at 8448 | tail bytes at 8704 | a base's fingerprint at 8960
#define PLANES_SMALL_TOT 8192
#define PLANES_SMALL_STATUS 8448
#define PLANES_SMALL_TAIL 8704
#define PLANES_SMALL_FP 8960                        // the fingerprint of a base (the calls against a base, trc_bplanes.inc)
#define PCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail(TRC_E_HIP, "%s -> %s", #x, hipGetErrorString(e_)); (void)hipStreamSynchronize(s); return 0; } } while (0)

// the context of the calling thread's current device, locked by the caller through `lk`
static int planes_ctx(HostCtx *&cp, std::unique_lock<std::mutex> &lk)
{
    int dev = 0;
    if (ctx_get(cp)) return TRC_E_NODEV;
    if (hipGetDevice(&dev) != hipSuccess) return fail(TRC_E_HIP, "hipGetDevice failed");
    lk = std::unique_lock<std::mutex>(cp->mu);
    return ctx_init(*cp, dev);
}

// ---- the advisor's host half: estimates and a choice from the histograms of trc_planes_hist_dev (no device involved) ----------------
extern "C" int trc_planes_advise(const uint64_t *hist, unsigned filters, unsigned esize, size_t m, trc_planes_advice *a)
{
    if (!hist || !a) return fail(TRC_E_ARG, "planes_advise: null histogram or advice");
    if (filters < 1 || filters > 7) return fail(TRC_E_ARG, "planes_advise: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", filters);
    if (!planes_esize_ok(esize)) return fail(TRC_E_ARG, "planes_advise: esize %u (2, 4 or 8)", esize);
    if (!m) return fail(TRC_E_ARG, "planes_advise: no element");
    memset(a, 0, sizeof *a);
    a->esize = esize; a->filters = filters; a->m = m;
    int best = -1;
    for (unsigned f = 0; f < 3; f++) {
        if (!(filters >> f & 1)) continue;
        for (unsigned k = 0; k < esize; k++) {
            const uint64_t *row = hist + ((size_t)f * esize + k) * 256;
            uint64_t sum = 0;
            double bits = 0;
            for (unsigned b = 0; b < 256; b++) {
                const uint64_t c = row[b];
                if (c > m - sum) return fail(TRC_E_ARG, "planes_advise: filter %u plane %u counts more than the %zu elements", f, k, m);
                sum += c;
                if (c) bits += (double)c * log2((double)m / (double)c);
            }
            if (sum != m) return fail(TRC_E_ARG, "planes_advise: filter %u plane %u counts %llu elements of %zu", f, k, (unsigned long long)sum, m);
            a->bits[f][k] = bits;
            a->total_bits[f] += bits;
        }
        if (best < 0 || a->total_bits[f] < a->total_bits[best]) best = (int)f;       // (ties: the lower id)
    }
    // a filter is never a default: it has to save 1/64 of the unfiltered total to be chosen over no filter
    if ((filters & 1) && best != TRC_FILTER_NONE && a->total_bits[TRC_FILTER_NONE] - a->total_bits[best] < a->total_bits[TRC_FILTER_NONE] / 64)
        best = TRC_FILTER_NONE;
    a->filter = best;
    return TRC_OK;
}

// the prefix that the explicit host call for a predictor puts in front of the TRCP container: none for unfiltered data, else the 16
// bytes of TRCF (stride 1), TRCS (a stride above 1) or TRCO (an order above 1)
static size_t planes_lead(PlanesPred pred)
{
    return pred.filter == TRC_FILTER_NONE ? 0 : sizeof(trc_fplanes_hdr);
}
static void planes_lead_write(PlanesPred pred, uint8_t *at, size_t size)
{
    if (pred.order >= 2) {
        trc_oplanes_hdr oh;
        memset(&oh, 0, sizeof oh);
        oh.magic = TRC_OPLANES_MAGIC; oh.order = (uint8_t)pred.order; oh.version = 1; oh.stride = (uint16_t)pred.stride; oh.size = size;
        memcpy(at, &oh, sizeof oh);
    } else if (pred.stride > 1) {
        trc_splanes_hdr sh;
        memset(&sh, 0, sizeof sh);
        sh.magic = TRC_SPLANES_MAGIC; sh.filter = (uint8_t)pred.filter; sh.version = 1; sh.stride = (uint16_t)pred.stride; sh.size = size;
        memcpy(at, &sh, sizeof sh);
    } else {
        trc_fplanes_hdr fh;
        memset(&fh, 0, sizeof fh);
        fh.magic = TRC_FPLANES_MAGIC; fh.filter = (uint8_t)pred.filter; fh.version = 1; fh.size = size;
        memcpy(at, &fh, sizeof fh);
    }
}

// the TRCP container of F(pred, chunk, esize, in) -- of `in` itself with TRC_FILTER_NONE.  choose: the advisor sets the filter
// from the bytes on the device (*advice, where given, says how), and `out` receives what the explicit host call writes for
// that choice: the TRCP container, behind the 16-byte TRCF prefix where the choice is a filter.
// pred.based: the container of D(filter, esize, in, base); the m * esize bytes of the host buffer pred.base go to the context's
// second buffer, and *base_fp receives their fingerprint, computed on the device.
// by_order (trc_encode_aoplanes_host, with choose): the choice is among the predictor orders 0 .. 3 at pred.stride, not among the
// filters; *oadvice, where given, says how, and the prefix is the one of the explicit call for that choice (planes_lead_write).
static PlanesPred pred_order(int order, int stride);                     // trc_oplanes.inc
static size_t planes_host_encode(int codec, PlanesPred pred, bool choose, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                 void *out, size_t outcap, unsigned cdfnum, trc_planes_advice *advice, uint64_t *base_fp,
                                 trc_planes_order_advice *oadvice = nullptr, bool by_order = false)
{
    if (!codec_ok(codec)) { fail(TRC_E_ARG, "codec %d not available", codec); return 0; }
    if (codec_row(codec).low4) { fail(TRC_E_ARG, "encode_planes_host: " PLANES_LOW4, codec); return 0; }      // before anything is uploaded
    if (!in || !out || !planes_esize_ok(esize) || n < esize) { fail(TRC_E_ARG, "encode_planes_host: bad arguments (esize %u, %zu bytes)", esize, n); return 0; }
    const TrcCodec &r = codec_row(codec);
    const size_t m = n / esize;
    const unsigned t = (unsigned)(n % esize);
    if (!chunk) { chunk = trc_auto_chunk_codec(codec, m); if (chunk < r.floor) chunk = r.floor; }
    if (chunk_ok(chunk) && chunk > r.chunk_max) chunk = r.chunk_max;                     // as trc_encode_host does
    if (!r.cdf && !r.ss) cdfnum = 0;
    PlanesMap P;
    if (!planes_map(codec, n, esize, chunk, P)) { fail(TRC_E_ARG, "encode_planes_host: bad (codec, n, esize, chunk %u)", chunk); return 0; }
    HostCtx *cp = nullptr;
    std::unique_lock<std::mutex> lk;
    if (planes_ctx(cp, lk)) return 0;
    HostCtx &c = *cp;
    const size_t dirsz = up256(4 * P.nc + 256);
    const size_t histb = !choose ? 0 : by_order ? trc_planes_hist_order_bytes(esize) : trc_planes_hist_bytes(esize);       // (in the workspace, ahead of the encode)
    if (grow(&c.d_in, &c.cap_in, n) || grow(&c.d_cont, &c.cap_cont, esize * (dirsz + P.buf)) ||
        grow(&c.d_work[0], &c.cap_work[0], esize * P.slice > histb ? esize * P.slice : histb)) return 0;
    hipStream_t s = c.s_k[0];
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + up256(esize * 4 * P.nc + 256);
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    uint64_t *d_total = (uint64_t *)(c.d_small + PLANES_SMALL_TOT);
    int32_t *d_status = (int32_t *)(c.d_small + PLANES_SMALL_STATUS);
    uint8_t *d_tail = c.d_small + PLANES_SMALL_TAIL;
    PCHK(hipMemcpyAsync(c.d_in, in, n, hipMemcpyHostToDevice, s));
    uint64_t *d_fp = (uint64_t *)(c.d_small + PLANES_SMALL_FP);
    if (pred.based) {
        if (grow(&c.d_base, &c.cap_base, m * esize)) return 0;
        PCHK(hipMemcpyAsync(c.d_base, pred.base, m * esize, hipMemcpyHostToDevice, s));
        if (trc_base_fingerprint_dev(c.d_base, m * esize, d_fp, s)) { (void)hipStreamSynchronize(s); return 0; }
        pred.base = c.d_base;
    }
    size_t lead = 0;                                                     // bytes of TRCF prefix in front of the container
    if (choose) {
        std::vector<uint64_t> hist(histb / sizeof(uint64_t));
        if (by_order ? trc_planes_hist_order_dev(15, pred.stride, c.d_in, n, esize, chunk, (uint64_t *)c.d_work[0], s)
                     : trc_planes_hist_dev(7, c.d_in, n, esize, chunk, (uint64_t *)c.d_work[0], s)) { (void)hipStreamSynchronize(s); return 0; }
        PCHK(hipMemcpyAsync(hist.data(), c.d_work[0], histb, hipMemcpyDeviceToHost, s));
        PCHK(hipStreamSynchronize(s));
        if (by_order) {
            trc_planes_order_advice adv;
            if (trc_planes_advise_order(hist.data(), 15, esize, m, &adv)) return 0;
            if (oadvice) *oadvice = adv;
            pred = pred_order(adv.order, pred.stride);
        } else {
            trc_planes_advice adv;
            if (trc_planes_advise(hist.data(), 7, esize, m, &adv)) return 0;
            if (advice) *advice = adv;
            pred.filter = adv.filter;
        }
        if ((lead = planes_lead(pred))) {
            if (outcap <= lead) { fail(TRC_E_ARG, "%s: out holds %zu bytes (%s)", by_order ? "encode_aoplanes_host" : "encode_aplanes_host", outcap, by_order ? "trc_oplanes_bound" : "trc_fplanes_bound"); return 0; }
            out = (uint8_t *)out + lead; outcap -= lead;
        }
    }
    if (planes_encode_dev(codec, pred, c.d_in, n, esize, chunk, r.cdf ? d_cdf : nullptr, cdfnum, r.cdf ? d_status : nullptr,
                          d_clen, d_payload, d_total, d_tail, c.d_work[0], c.cap_work[0], s)) { (void)hipStreamSynchronize(s); return 0; }
    if (pred.based) PCHK(hipMemcpyAsync(base_fp, d_fp, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    uint64_t total[8];
    int32_t status[8];
    uint16_t cdf[8 * TRC_PLANES_CDF_STRIDE];
    PCHK(hipMemcpyAsync(total, d_total, 8 * esize, hipMemcpyDeviceToHost, s));
    if (r.cdf) {
        PCHK(hipMemcpyAsync(status, d_status, 4 * esize, hipMemcpyDeviceToHost, s));
        PCHK(hipMemcpyAsync(cdf, d_cdf, 2 * TRC_PLANES_CDF_STRIDE * (size_t)esize, hipMemcpyDeviceToHost, s));
    }
    PCHK(hipStreamSynchronize(s));
    // the layout, now that every plane's size is known
    const size_t cdfb = planes_cdf_bytes(r, cdfnum), front = sizeof(trc_planes_hdr) + 8 * (size_t)esize;
    uint64_t off[8];
    size_t pos = up8(front);
    for (unsigned k = 0; k < esize; k++) {
        if (r.cdf && status[k] < 0) { fail(TRC_E_CDF, "encode_planes_host: plane %u has a distribution the 15-bit CDF cannot hold", k); return 0; }
        if (total[k] > P.m) { fail(TRC_E_HIP, "encode_planes_host: plane %u reports %llu payload bytes of %zu", k, (unsigned long long)total[k], P.m); return 0; }
        off[k] = pos;
        pos = up8(pos + cdfb + sizeof(trc_container_hdr) + 4 * P.nc + (size_t)total[k]);
    }
    const size_t size = pos + t;
    if (outcap < size) { fail(TRC_E_ARG, "encode_planes_host: out holds %zu bytes, the container needs %zu (trc_planes_bound)", outcap, size); return 0; }
    uint8_t *o = (uint8_t *)out;
    trc_planes_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_PLANES_MAGIC; h.codec = (uint8_t)codec; h.version = 1; h.esize = (uint8_t)esize; h.tail = (uint8_t)t;
    h.chunk = chunk; h.cdfnum = cdfnum; h.n = n; h.size = size;
    memcpy(o, &h, sizeof h);
    memcpy(o + sizeof h, off, 8 * (size_t)esize);
    memset(o + front, 0, (size_t)off[0] - front);
    for (unsigned k = 0; k < esize; k++) {
        uint8_t *sec = o + off[k];
        const size_t endk = k + 1 < esize ? (size_t)off[k + 1] : pos;
        if (r.cdf) { memset(sec, 0, cdfb); memcpy(sec, cdf + k * TRC_PLANES_CDF_STRIDE, 2 * ((size_t)cdfnum + 1)); sec += cdfb; }
        trc_container_hdr sh;
        memset(&sh, 0, sizeof sh);
        sh.magic = TRC_MAGIC; sh.codec = (uint8_t)codec; sh.version = 1; sh.cdfnum = (uint16_t)cdfnum;
        sh.chunk = chunk; sh.nchunks = (uint32_t)P.nc; sh.n = P.m; sh.payload = total[k];
        memcpy(sec, &sh, sizeof sh);
        PCHK(hipMemcpyAsync(sec + sizeof sh, d_clen + k * P.nc, 4 * P.nc, hipMemcpyDeviceToHost, s));
        if (total[k]) PCHK(hipMemcpyAsync(sec + sizeof sh + 4 * P.nc, d_payload + k * P.buf, (size_t)total[k], hipMemcpyDeviceToHost, s));
        uint8_t *pe = sec + sizeof sh + 4 * P.nc + (size_t)total[k];
        memset(pe, 0, (size_t)(o + endk - pe));
    }
    if (t) PCHK(hipMemcpyAsync(o + pos, d_tail, t, hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    if (lead) planes_lead_write(pred, o - lead, lead + size);
    return lead + size;
}
extern "C" size_t trc_encode_planes_host(int codec, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                         void *out, size_t outcap, unsigned cdfnum)
{
    return planes_host_encode(codec, pred_none(), false, in, n, esize, chunk, out, outcap, cdfnum, nullptr, nullptr);
}

// sections of a container that planes_verdict has accepted: where plane k's CDF and TRC1 container lie and how far the latter may reach
struct PlanesSec { const uint8_t *cdf, *cont; size_t ext; };
static void planes_sections(const uint8_t *b, const trc_planes_hdr &h, PlanesSec *S)
{
    const size_t end = (size_t)h.size - h.tail, cdfb = planes_cdf_bytes(codec_row(h.codec), h.cdfnum);
    uint64_t off[8];
    memcpy(off, b + sizeof h, 8 * (size_t)h.esize);
    for (unsigned k = 0; k < h.esize; k++) {
        S[k].cdf = b + off[k]; S[k].cont = b + off[k] + cdfb;
        S[k].ext = (size_t)((k + 1 < h.esize ? off[k + 1] : end) - off[k]) - cdfb;
    }
}

// elements [first_chunk * chunk, ...) of `count` chunks -- or, whole = true, everything with the tail -- decoded to c.d_in.
// pred.based: pred.base = those elements of the base, in host memory; they go to the context's second buffer.  fp, where
// given, is what their fingerprint must be: it is computed on the device and compared before anything is decoded.
static size_t planes_host_decode(HostCtx &c, PlanesPred pred, const uint8_t *b, const trc_planes_hdr &h, bool whole, size_t first_chunk, size_t count, size_t elems,
                                 const uint64_t *fp)
{
    const TrcCodec &r = codec_row(h.codec);
    const unsigned esize = h.esize;
    const size_t m = (size_t)(h.n / esize), nc = (m + h.chunk - 1) / h.chunk;
    const size_t nsub = elems * esize + (whole ? h.tail : 0);            // the covering chunks are a planar container of their own
    PlanesMap P;
    if (!planes_map(h.codec, nsub, esize, h.chunk, P)) { fail(TRC_E_ARG, "decode_planes_host: bad (codec, n, esize, chunk)"); return 0; }
    PlanesSec S[8];
    planes_sections(b, h, S);
    if (grow(&c.d_in, &c.cap_in, nsub) || grow(&c.d_cont, &c.cap_cont, up256(esize * 4 * count + 256) + esize * P.buf) ||
        grow(&c.d_work[0], &c.cap_work[0], esize * P.slice)) return 0;
    hipStream_t s = c.s_k[0];
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + up256(esize * 4 * count + 256);
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    uint8_t *d_tail = c.d_small + PLANES_SMALL_TAIL;
    if (pred.based) {
        uint64_t *d_fp = (uint64_t *)(c.d_small + PLANES_SMALL_FP), got = 0;
        if (grow(&c.d_base, &c.cap_base, elems * esize)) return 0;
        PCHK(hipMemcpyAsync(c.d_base, pred.base, elems * esize, hipMemcpyHostToDevice, s));
        pred.base = c.d_base;
        if (fp) {
            if (trc_base_fingerprint_dev(c.d_base, elems * esize, d_fp, s)) { (void)hipStreamSynchronize(s); return 0; }
            PCHK(hipMemcpyAsync(&got, d_fp, sizeof got, hipMemcpyDeviceToHost, s));
            PCHK(hipStreamSynchronize(s));
            if (got != *fp) {
                fail(TRC_E_ARG, "decode_planes_host: base fingerprint %016llx, the container was made against %016llx: this is not its base",
                     (unsigned long long)got, (unsigned long long)*fp);
                return 0;
            }
        }
    }
    for (unsigned k = 0; k < esize; k++) {
        trc_container_hdr sh;
        memcpy(&sh, S[k].cont, sizeof sh);
        trc_range R;
        range_plan(S[k].cont, sh, first_chunk * (size_t)h.chunk, elems, &R);
        const uint8_t *dir = S[k].cont + sizeof sh, *pay = dir + 4 * nc;
        if (r.cdf) PCHK(hipMemcpyAsync(d_cdf + k * TRC_PLANES_CDF_STRIDE, S[k].cdf, 2 * ((size_t)h.cdfnum + 1), hipMemcpyHostToDevice, s));
        PCHK(hipMemcpyAsync(d_clen + k * count, dir + 4 * first_chunk, 4 * count, hipMemcpyHostToDevice, s));
        if (R.payload_len) PCHK(hipMemcpyAsync(d_payload + k * P.buf, pay + R.payload_off, (size_t)R.payload_len, hipMemcpyHostToDevice, s));
    }
    if (whole && h.tail) PCHK(hipMemcpyAsync(d_tail, b + h.size - h.tail, h.tail, hipMemcpyHostToDevice, s));
    if (planes_decode_dev(h.codec, pred, d_clen, d_payload, d_tail, nsub, esize, h.chunk, r.cdf ? d_cdf : nullptr, h.cdfnum,
                          c.d_in, c.d_work[0], c.cap_work[0], s)) { (void)hipStreamSynchronize(s); return 0; }
    return nsub;
}

// the two decoders of a TRCP container whose content is F(pred, chunk, esize, original); pred.base and fp as planes_host_decode, for
// the whole buffer
static size_t planes_host_decode_all(PlanesPred pred, const void *in, size_t inlen, void *out, size_t outlen, const uint64_t *fp)
{
    if (trc_planes_check(in, inlen, outlen)) return 0;
    trc_planes_hdr h;
    memcpy(&h, in, sizeof h);
    HostCtx *cp = nullptr;
    std::unique_lock<std::mutex> lk;
    if (planes_ctx(cp, lk)) return 0;
    const size_t m = (size_t)(h.n / h.esize);
    if (!planes_host_decode(*cp, pred, (const uint8_t *)in, h, true, 0, (m + h.chunk - 1) / h.chunk, m, fp)) return 0;
    hipStream_t s = cp->s_k[0];
    PCHK(hipMemcpyAsync(out, cp->d_in, (size_t)h.n, hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    return (size_t)h.n;
}

extern "C" size_t trc_decode_planes_host(const void *in, size_t inlen, void *out, size_t outlen)
{
    if (!in || !out) { fail(TRC_E_ARG, "decode_planes_host: bad arguments"); return 0; }
    return planes_host_decode_all(pred_none(), in, inlen, out, outlen, nullptr);
}

static size_t planes_host_decode_bytes(PlanesPred pred, const void *in, size_t inlen, size_t offset, size_t len, void *out)
{
    if (trc_planes_check(in, inlen, (size_t)-1)) return 0;
    trc_planes_hdr h;
    memcpy(&h, in, sizeof h);
    if (!len || offset > h.n || len > h.n - offset) { fail(TRC_E_ARG, "decode_planes_range_host: bytes [%zu, %zu + %zu) of %llu", offset, offset, len, (unsigned long long)h.n); return 0; }
    const uint8_t *b = (const uint8_t *)in;
    const size_t body = (size_t)h.n - h.tail;                            // bytes of whole elements
    const size_t lb = offset < body ? (offset + len < body ? len : body - offset) : 0;       // ... of the range; the rest is tail
    if (lb) {
        const size_t e0 = offset / h.esize, e1 = (offset + lb - 1) / h.esize;                // first and last element
        const size_t c0 = e0 / h.chunk, c1 = e1 / h.chunk, m = body / h.esize;
        const size_t elems = ((c1 + 1) * (size_t)h.chunk < m ? (c1 + 1) * (size_t)h.chunk : m) - c0 * (size_t)h.chunk;
        HostCtx *cp = nullptr;
        std::unique_lock<std::mutex> lk;
        if (planes_ctx(cp, lk)) return 0;
        if (!planes_host_decode(*cp, pred_from(pred, c0 * (size_t)h.chunk * h.esize), b, h, false, c0, c1 - c0 + 1, elems, nullptr)) return 0;
        hipStream_t s = cp->s_k[0];
        PCHK(hipMemcpyAsync(out, cp->d_in + (offset - c0 * (size_t)h.chunk * h.esize), lb, hipMemcpyDeviceToHost, s));
        PCHK(hipStreamSynchronize(s));
    }
    if (lb < len) memcpy((uint8_t *)out + lb, b + h.size - h.tail + (offset + lb - body), len - lb);
    return len;
}
extern "C" size_t trc_decode_planes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out)
{
    if (!in || !out) { fail(TRC_E_ARG, "decode_planes_range_host: bad arguments"); return 0; }
    return planes_host_decode_bytes(pred_none(), in, inlen, offset, len, out);
}
#undef PCHK

// ---- the TRCF container: trc_fplanes_hdr (16 B) | the TRCP container of the filtered data ------------------------------------------
extern "C" size_t trc_fplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum)
{
    const size_t b = trc_planes_bound(n, esize, chunk, cdfnum);
    return b ? b + sizeof(trc_fplanes_hdr) : 0;
}

// What the prefixes of the TRCF, TRCS and TRCD containers have in common -- magic, filter, version and size lie alike in all three
// headers -- in the order they are looked at; `own` is the container's check of its 16-bit field, between the filter and the size.
// 0 and the header, or TRC_E_ARG with the reason set.
template <class Hdr, class Own> static int planes_prefix(const char *noun, uint32_t magic, const void *buf, size_t buflen, Hdr &h, Own own)
{
    if (!buf || buflen < sizeof h) return fail(TRC_E_ARG, "%s: %zu bytes is shorter than the header", noun, buflen);
    memcpy(&h, buf, sizeof h);
    if (h.magic != magic || h.version != 1) return fail(TRC_E_ARG, "%s: bad magic/version", noun);
    if (h.filter != TRC_FILTER_ZDELTA && h.filter != TRC_FILTER_XOR) return fail(TRC_E_ARG, "%s: filter %u (1 zigzag delta, 2 xor)", noun, h.filter);
    const int rc = own(h);
    if (rc) return rc;
    if (h.size > buflen) return fail(TRC_E_ARG, "%s: states %llu bytes, the buffer holds %zu", noun, (unsigned long long)h.size, buflen);
    if (h.size <= sizeof h) return fail(TRC_E_ARG, "%s: size %llu leaves no room behind the header", noun, (unsigned long long)h.size);
    return TRC_OK;
}
static int fplanes_prefix(const void *buf, size_t buflen, trc_fplanes_hdr &h)
{
    return planes_prefix("filtered planes container", TRC_FPLANES_MAGIC, buf, buflen, h, [](const trc_fplanes_hdr &f) {
        return f.zero ? fail(TRC_E_ARG, "filtered planes container: reserved field is 0x%x, must be 0", f.zero) : (int)TRC_OK; });
}
extern "C" int trc_fplanes_check(const void *buf, size_t buflen, size_t outlen)
{
    trc_fplanes_hdr h;
    const int rc = fplanes_prefix(buf, buflen, h);
    return rc ? rc : trc_planes_check((const uint8_t *)buf + sizeof h, (size_t)h.size - sizeof h, outlen);
}

extern "C" size_t trc_encode_fplanes_host(int codec, int filter, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                          void *out, size_t outcap, unsigned cdfnum)
{
    if (filter != TRC_FILTER_ZDELTA && filter != TRC_FILTER_XOR) {
        fail(TRC_E_ARG, "encode_fplanes_host: filter %d (1 zigzag delta, 2 xor; unfiltered data goes through trc_encode_planes_host)", filter);
        return 0;
    }
    if (!out || outcap <= sizeof(trc_fplanes_hdr)) { fail(TRC_E_ARG, "encode_fplanes_host: out holds %zu bytes (trc_fplanes_bound)", outcap); return 0; }
    const size_t inner = planes_host_encode(codec, pred_stride(filter, 1), false, in, n, esize, chunk, (uint8_t *)out + sizeof(trc_fplanes_hdr), outcap - sizeof(trc_fplanes_hdr), cdfnum,
                                            nullptr, nullptr);
    if (!inner) return 0;
    trc_fplanes_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_FPLANES_MAGIC; h.filter = (uint8_t)filter; h.version = 1; h.size = sizeof h + inner;
    memcpy(out, &h, sizeof h);
    return (size_t)h.size;
}

// (the prefix is checked here, the inner container by the planes decoders: together trc_fplanes_check, ahead of anything else)
extern "C" size_t trc_decode_fplanes_host(const void *in, size_t inlen, void *out, size_t outlen)
{
    trc_fplanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_fplanes_host: bad arguments"); return 0; }
    if (fplanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_all(pred_stride(h.filter, 1), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, out, outlen, nullptr);
}

extern "C" size_t trc_decode_fplanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out)
{
    trc_fplanes_hdr h;
    if (!in || !out) { fail(TRC_E_ARG, "decode_fplanes_range_host: bad arguments"); return 0; }
    if (fplanes_prefix(in, inlen, h)) return 0;
    return planes_host_decode_bytes(pred_stride(h.filter, 1), (const uint8_t *)in + sizeof h, (size_t)h.size - sizeof h, offset, len, out);
}

// ---- either container, and the encoder that chooses between them ------------------------------------------------------------------
extern "C" size_t trc_encode_aplanes_host(int codec, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                          void *out, size_t outcap, unsigned cdfnum, trc_planes_advice *advice)
{
    return planes_host_encode(codec, pred_none(), true, in, n, esize, chunk, out, outcap, cdfnum, advice, nullptr);
}

extern "C" size_t trc_decode_xplanes_host(const void *in, size_t inlen, void *out, size_t outlen)
{
    uint32_t magic = 0;
    if (!in || !out) { fail(TRC_E_ARG, "decode_xplanes_host: bad arguments"); return 0; }
    if (inlen >= sizeof magic) memcpy(&magic, in, sizeof magic);
    if (magic == TRC_PLANES_MAGIC) return trc_decode_planes_host(in, inlen, out, outlen);
    if (magic == TRC_FPLANES_MAGIC) return trc_decode_fplanes_host(in, inlen, out, outlen);
    if (magic == TRC_SPLANES_MAGIC) return trc_decode_splanes_host(in, inlen, out, outlen);
    if (magic == TRC_OPLANES_MAGIC) return trc_decode_oplanes_host(in, inlen, out, outlen);
    if (magic == TRC_BPLANES_MAGIC) {
        fail(TRC_E_ARG, "decode_xplanes_host: a planes container against a base (TRCD): trc_decode_bplanes_host decodes it, given the base");
        return 0;
    }
    fail(TRC_E_ARG, "decode_xplanes_host: neither a planes (TRCP) nor a filtered planes (TRCF, TRCS) container");
    return 0;
}
