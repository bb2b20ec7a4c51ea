// trc_bplanes.hip -- the byte-plane split and join of trc_planes.hip behind a zigzag-delta (TRC_FILTER_ZDELTA) or xor (TRC_FILTER_XOR)
// filter whose predictor is not inside the buffer but in a BASE buffer of the same shape, resident on the device: the previous
// checkpoint, the base model of a fine-tune, a page before its update.  Also here: the advisor's histograms under these filters
// and the fingerprint by which a container names its base.
//
// Definition (include/trc_hip.h): x[i], b[i] = the m little-endian elements of w = 8 * esize bits of `in` and of `base`;
// y[i] = zigzag(x[i] - b[i] mod 2^w)  or  x[i] ^ b[i];  plane k = byte k of every y[i].  The tail bytes are not filtered, and of the
// base only bytes [0, m * esize) are read: it needs no slack behind it and no tail.
//
// Element i depends on element i of the base alone, so there is no restart, no reach backwards and, in the join, no scan: both
// kernels are the unfiltered ones of trc_planes.hip with a second load stream, the base's 16-byte words next to the input's (split)
// or next to the planes' 8-byte words (join), all issued before the first use.  The join may write where it reads the base
// (out == base applies a delta to a resident base in place): a thread has its base vector in registers before it stores to those
// addresses and no other thread touches them, which is why `base` and `out` carry no __restrict__ there.
#include "trc_planes_count.h"

// in, base: 16-byte aligned; m * ESIZE + t bytes of in and m * ESIZE bytes of base are read.  planes: 256-byte aligned, pitch a
// multiple of 256.  Writes [0, m) of every plane and [0, t) of tail, nothing else.
template <int ESIZE, int FILTER> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_bplanes_split_kernel(const uint8_t *__restrict__ in, const uint8_t *__restrict__ base, size_t m, u32 t,
                              uint8_t *__restrict__ planes, size_t pitch, uint8_t *__restrict__ tail)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE)), *bsrc = (const uint4 *)(base + v * (TRC_PLANES_VEC * ESIZE));
        uint4 xq[NQ], bq[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) { xq[q] = src[q]; bq[q] = bsrc[q]; }
        u32 w[NW], bw[NW];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            w[4 * q] = xq[q].x; w[4 * q + 1] = xq[q].y; w[4 * q + 2] = xq[q].z; w[4 * q + 3] = xq[q].w;
            bw[4 * q] = bq[q].x; bw[4 * q + 1] = bq[q].y; bw[4 * q + 2] = bq[q].z; bw[4 * q + 3] = bq[q].w;
        }
        T e[TRC_PLANES_VEC], b[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
        unpack<ESIZE>(bw, b);
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) e[j] = fwd<ESIZE, FILTER>(e[j], b[j]);
        pack<ESIZE>(e, w);
        uint2 p[ESIZE];
        vec_split<ESIZE>(w, p);
#pragma unroll
        for (int k = 0; k < ESIZE; k++) *(uint2 *)(planes + k * pitch + v * TRC_PLANES_VEC) = p[k];
    }
    // the elements behind the last whole vector (at most 7), one per lane, and the tail bytes (at most ESIZE - 1)
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC), g = threadIdx.x;
        if (g < rest) {
            const size_t i = nv * TRC_PLANES_VEC + g;
            const T y = fwd<ESIZE, FILTER>((T)((const M *)in)[i], (T)((const M *)base)[i]);
#pragma unroll
            for (int k = 0; k < ESIZE; k++) planes[k * pitch + i] = (uint8_t)(y >> (8 * k));
        } else if (g < rest + t) tail[g - rest] = in[m * ESIZE + (g - rest)];
    }
}

// the mirror image: writes [0, m * ESIZE + t) of out, nothing else; reads [0, m * ESIZE) of base.  out == base is allowed (see above).
template <int ESIZE, int FILTER> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_bplanes_join_kernel(const uint8_t *__restrict__ planes, size_t pitch, const uint8_t *__restrict__ tail, const uint8_t *base,
                             size_t m, u32 t, uint8_t *out)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const uint4 *bsrc = (const uint4 *)(base + v * (TRC_PLANES_VEC * ESIZE));
        uint2 p[ESIZE];
        uint4 bq[NQ];
#pragma unroll
        for (int k = 0; k < ESIZE; k++) p[k] = *(const uint2 *)(planes + k * pitch + v * TRC_PLANES_VEC);
#pragma unroll
        for (int q = 0; q < NQ; q++) bq[q] = bsrc[q];
        u32 w[NW], bw[NW];
        vec_join<ESIZE>(p, w);
#pragma unroll
        for (int q = 0; q < NQ; q++) { bw[4 * q] = bq[q].x; bw[4 * q + 1] = bq[q].y; bw[4 * q + 2] = bq[q].z; bw[4 * q + 3] = bq[q].w; }
        T e[TRC_PLANES_VEC], b[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
        unpack<ESIZE>(bw, b);
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) e[j] = inv<ESIZE, FILTER>(e[j], b[j]);
        pack<ESIZE>(e, w);
        uint4 *dst = (uint4 *)(out + v * (TRC_PLANES_VEC * ESIZE));
#pragma unroll
        for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC), g = threadIdx.x;
        if (g < rest) {
            const size_t i = nv * TRC_PLANES_VEC + g;
            T y = 0;
#pragma unroll
            for (int k = 0; k < ESIZE; k++) y |= (T)planes[k * pitch + i] << (8 * k);
            ((M *)out)[i] = (M)inv<ESIZE, FILTER>(y, (T)((const M *)base)[i]);
        } else if (g < rest + t) out[m * ESIZE + (g - rest)] = tail[g - rest];
    }
}

// ---- the advisor's histograms against a base: trc_planes_hist_kernel (trc_planes_hist.hip) with the base as predictor ------------
// in, base: 16-byte aligned, m * ESIZE bytes of each are read.  filters: bit f = count filter f, 1 .. 7 with bit 1 or 2 set.
// hist[(f * ESIZE + k) * 256 + b] += the elements whose byte k under filter f is b.  Dynamic LDS and round_vecs as there.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_bplanes_hist_kernel(const uint8_t *__restrict__ in, const uint8_t *__restrict__ base, size_t m, u32 filters, u32 cshift, u32 round_vecs,
                             u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const HistRows R = hist_rows<ESIZE>(sm, filters, cshift);

    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK, b0 = (size_t)blockIdx.x * TRC_PLANES_BLOCK;
    const size_t turns = b0 < nv ? (nv - b0 + step - 1) / step : 0;      // of the whole workgroup: the flush holds barriers
    u32 since = 0;
    size_t v = b0 + tid;
    for (size_t it = 0; it < turns; it++, v += step) {
        if (v < nv) {
            const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE)), *bsrc = (const uint4 *)(base + v * (TRC_PLANES_VEC * ESIZE));
            uint4 xq[NQ], bq[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) { xq[q] = src[q]; bq[q] = bsrc[q]; }
            u32 w[NW], bw[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                w[4 * q] = xq[q].x; w[4 * q + 1] = xq[q].y; w[4 * q + 2] = xq[q].z; w[4 * q + 3] = xq[q].w;
                bw[4 * q] = bq[q].x; bw[4 * q + 1] = bq[q].y; bw[4 * q + 2] = bq[q].z; bw[4 * q + 3] = bq[q].w;
            }
            T b[TRC_PLANES_VEC];
            unpack<ESIZE>(bw, b);
            count_predicted<ESIZE>(sm, R, cshift, w, b);
        }
        if (++since == round_vecs && it + 1 < turns) { hist_flush<ESIZE>(sm, R, cshift, hist, false); since = 0; }
    }
    // the elements behind the last whole vector (at most 7), one per lane
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC);
        if (tid < rest) {
            const size_t i = nv * TRC_PLANES_VEC + tid;
            count_filtered_elem<ESIZE>(sm, R, cshift, (T)((const M *)in)[i], (T)((const M *)base)[i]);
        }
    }
    hist_flush<ESIZE>(sm, R, cshift, hist, false);
}

// ---- the fingerprint of a base: fp = sum_j (2j + 1) * w_j + nbytes * TRC_FP_LEN_MUL mod 2^64 over the little-endian u64 words w_j
// of the nbytes bytes, zero-padded to 8.  A sum, so its terms are added in any order: a partial sum per thread over the whole
// 16-byte pairs of words, the bytes behind them (at most 15, read one by one: nothing at or behind p + nbytes is touched) and the
// length term by one lane, a reduction across the wave and the workgroup, one 64-bit atomicAdd per workgroup into *fp, which the
// call has zeroed on the stream.  (A base per item of a batch, from one launch: trc_fp_batch.inc.)
#include "trc_fp.h"                               // TRC_FP_LEN_MUL, fp_pair
__global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_base_fingerprint_kernel(const uint8_t *__restrict__ p, size_t nbytes, u64a *__restrict__ fp)
{
    __shared__ uint64_t wave_sum[TRC_PLANES_BLOCK / 64];
    const size_t np = nbytes / 16, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    const uint4 *src = (const uint4 *)p;
    uint64_t sum = 0;
    size_t i = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x;
    for (; i + 3 * step < np; i += 4 * step) {                             // four loads in flight per thread
        uint4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = src[i + u * step];
#pragma unroll
        for (int u = 0; u < 4; u++) sum += fp_pair(i + u * step, x[u]);
    }
    for (; i < np; i += step) sum += fp_pair(i, src[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (size_t j = 2 * np; j * 8 < nbytes; j++) {
            uint64_t w = 0;
            for (u32 b = 0; b < 8 && j * 8 + b < nbytes; b++) w |= (uint64_t)p[j * 8 + b] << (8 * b);
            sum += (2 * (uint64_t)j + 1) * w;
        }
        sum += (uint64_t)nbytes * TRC_FP_LEN_MUL;
    }
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
#pragma unroll
        for (int i = 0; i < TRC_PLANES_BLOCK / 64; i++) s += wave_sum[i];
        atomicAdd(fp, (u64a)s);
    }
}

extern "C" uint64_t trc_base_fingerprint_host(const void *base, size_t nbytes)
{
    const uint8_t *p = (const uint8_t *)base;
    uint64_t sum = (uint64_t)nbytes * TRC_FP_LEN_MUL;
    for (size_t j = 0; j * 8 < nbytes; j++) {
        uint64_t w = 0;
        for (unsigned b = 0; b < 8 && j * 8 + b < nbytes; b++) w |= (uint64_t)p[j * 8 + b] << (8 * b);
        sum += (2 * (uint64_t)j + 1) * w;
    }
    return sum;
}

extern "C" int trc_base_fingerprint_dev(const void *d_base, size_t nbytes, uint64_t *d_fp, void *stream)
{
    if (!d_fp || ((uintptr_t)d_fp & 7)) return trc_fail(TRC_E_ARG, "base_fingerprint: d_fp must be 8-byte aligned");
    if (nbytes && (!d_base || ((uintptr_t)d_base & 15))) return trc_fail(TRC_E_ARG, "base_fingerprint: the base must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_fp, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return trc_fail(TRC_E_HIP, "base_fingerprint: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(trc_base_fingerprint_kernel, dim3(planes_grid(nbytes / 16 * TRC_PLANES_VEC)), dim3(TRC_PLANES_BLOCK), 0, s,
                       (const uint8_t *)d_base, nbytes, (u64a *)d_fp);
    e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "base_fingerprint: %s", hipGetErrorString(e));
}

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
int trc_planes_filter_arg(const char *who, int filter);                // trc_fplanes.hip

// the base of a call with filter 1 or 2 (also for the coded calls of trc_planes.inc, which look at it before they enqueue anything)
int trc_bplanes_base_arg(const char *who, const void *d_base)
{
    if (!d_base || ((uintptr_t)d_base & 15)) return trc_fail(TRC_E_ARG, "%s: a filter against a base needs the base, 16-byte aligned", who);
    return TRC_OK;
}
// where a join writes: on top of the base exactly (in place) or clear of the bytes it reads of it
int trc_bplanes_overlap_arg(const char *who, const void *d_base, size_t base_bytes, const void *d_out, size_t n)
{
    const uintptr_t b = (uintptr_t)d_base, o = (uintptr_t)d_out;
    if (o != b && o < b + base_bytes && b < o + n)
        return trc_fail(TRC_E_ARG, "%s: the output overlaps the base without starting where it starts (in place means d_out == the base)", who);
    return TRC_OK;
}

typedef void (*bsplit_fn)(const uint8_t *, const uint8_t *, size_t, u32, uint8_t *, size_t, uint8_t *);
typedef void (*bjoin_fn)(const uint8_t *, size_t, const uint8_t *, const uint8_t *, size_t, u32, uint8_t *);
#define BPLANES_TABLE(K) { { K<2, TRC_FILTER_ZDELTA>, K<2, TRC_FILTER_XOR> }, { K<4, TRC_FILTER_ZDELTA>, K<4, TRC_FILTER_XOR> }, \
                           { K<8, TRC_FILTER_ZDELTA>, K<8, TRC_FILTER_XOR> } }
// [esize_row][filter - 1]
static const bsplit_fn bsplit_kernels[3][2] = BPLANES_TABLE(trc_bplanes_split_kernel);
static const bjoin_fn bjoin_kernels[3][2] = BPLANES_TABLE(trc_bplanes_join_kernel);

extern "C" int trc_planes_split_base_dev(int filter, const void *d_in, const void *d_base, size_t n, unsigned esize,
                                         void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    int rc = trc_planes_filter_arg("planes_split_base", filter);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_split_dev(d_in, n, esize, d_planes, pitch, d_tail, stream);
    if ((rc = planes_args("planes_split_base", d_in, n, esize, d_planes, pitch, d_tail))) return rc;
    if ((rc = trc_bplanes_base_arg("planes_split_base", d_base))) return rc;
    const size_t m = n / esize;
    hipLaunchKernelGGL(bsplit_kernels[esize_row(esize)][filter - 1], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_in, (const uint8_t *)d_base, m, (u32)(n % esize), (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_split_base: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_join_base_dev(int filter, const void *d_planes, size_t pitch, const void *d_tail, const void *d_base,
                                        size_t n, unsigned esize, void *d_out, void *stream)
{
    int rc = trc_planes_filter_arg("planes_join_base", filter);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_join_dev(d_planes, pitch, d_tail, n, esize, d_out, stream);
    if ((rc = planes_args("planes_join_base", d_out, n, esize, d_planes, pitch, d_tail))) return rc;
    if ((rc = trc_bplanes_base_arg("planes_join_base", d_base))) return rc;
    const size_t m = n / esize;
    if ((rc = trc_bplanes_overlap_arg("planes_join_base", d_base, m * esize, d_out, n))) return rc;
    hipLaunchKernelGGL(bjoin_kernels[esize_row(esize)][filter - 1], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, (const uint8_t *)d_base, m, (u32)(n % esize), (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_join_base: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_hist_base_dev(unsigned filters, const void *d_in, const void *d_base, size_t n, unsigned esize,
                                        uint64_t *d_hist, void *stream)
{
    if (filters < 1 || filters > 7 || !(filters & 6u))                  // nothing to predict (or nothing sound): the unfiltered row, or its refusal
        return trc_planes_hist_dev(filters, d_in, n, esize, TRC_CHUNK_MIN, d_hist, stream);
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "planes_hist_base: esize %u (2, 4 or 8)", esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "planes_hist_base: %zu bytes hold no element of %u bytes", n, esize);
    if (!d_in || !d_hist || ((uintptr_t)d_in & 15) || ((uintptr_t)d_hist & 7))
        return trc_fail(TRC_E_ARG, "planes_hist_base: the element buffer must be 16-byte, the histogram 8-byte aligned");
    const int rc = trc_bplanes_base_arg("planes_hist_base", d_base);
    if (rc) return rc;
    const size_t m = n / esize;
    const HistShape h = hist_shape(filters, esize);
    unsigned grid = planes_grid(m);
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_bytes(esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "planes_hist_base: %s", hipGetErrorString(he));
    static void (*const kernels[3])(const uint8_t *, const uint8_t *, size_t, u32, u32, u32, u64a *) = TRC_BY_ESIZE(trc_bplanes_hist_kernel);
    hipLaunchKernelGGL(kernels[esize_row(esize)], dim3(grid), dim3(TRC_PLANES_BLOCK), h.lds, s,
                       (const uint8_t *)d_in, (const uint8_t *)d_base, m, filters, h.cshift, h.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_hist_base: %s", hipGetErrorString(he));
}
