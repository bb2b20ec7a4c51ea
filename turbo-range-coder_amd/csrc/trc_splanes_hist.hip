// trc_splanes_hist.hip -- the planes advisor's histograms under a STRIDED predictor: trc_planes_hist_kernel's counting (the LDS
// rows, the adds and the flush of trc_planes_hist.hip / trc_planes_count.h, explained there) with the rows of the zigzag-delta
// and xor filters counted under F_S, S = 2 .. 8: an element's predecessor is the element S back in its restart segment.  As in the
// strided split (trc_splanes.hip) a thread that does not open a segment loads the 16-byte words of the vector in front of its own
// that hold that vector's last S elements.  The row of TRC_FILTER_NONE does not depend on the stride.  What it writes is
// 3 * esize * 256 counters, so that trc_planes_advise serves on its output as it stands.
#include "trc_planes_count.h"

// in: 16-byte aligned, m * ESIZE bytes are read, nothing in front of them.  seg: a multiple of 64.  r0 = (m / 8 * 8) % seg.  filters:
// bit f = count filter f, 1 .. 7, with bit 1 or 2 set.  hist[(f * ESIZE + k) * 256 + b] += the elements whose byte k under filter f
// is b.  Dynamic LDS: (requested filters * ESIZE * 256 * 4) << cshift bytes.  round_vecs >= 1.
template <int ESIZE, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_splanes_hist_kernel(const uint8_t *__restrict__ in, size_t m, u32 seg, u32 r0, u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4, Q0 = NQ - (S * ESIZE + 15) / 16;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x, copy = tid & ((1u << cshift) - 1u);
    const u32 nf = __builtin_popcount(filters), words = (nf * ESIZE * 256u) << cshift, fwords = (ESIZE * 256u) << cshift;
    // where the rows of filter f start (the requested filters lie packed, in the order of their ids)
    const u32 row_n = copy, row_z = row_n + (filters & 1u ? fwords : 0u), row_x = row_z + (filters & 2u ? fwords : 0u);
    const bool with_n = filters & 1u, with_z = filters & 2u, with_x = filters & 4u;
    for (u32 i = tid; i < words; i += TRC_PLANES_BLOCK) sm[i] = 0;
    __syncthreads();

    // the workgroup's counters to the global histogram, and zero again; the whole workgroup calls it
    auto flush = [&]() __attribute__((always_inline)) {
        __syncthreads();
        for (u32 i = tid; i < nf * ESIZE * 256u; i += TRC_PLANES_BLOCK) {
            const u32 row = i >> 8, bin = ((i & 255u) + 37u * blockIdx.x) & 255u;
            u32 *c = sm + ((row * 256u + bin) << cshift);
            u32 sum = 0;
            for (u32 q = 0; q < (1u << cshift); q++) { sum += c[q]; c[q] = 0; }
            u32 f = row / ESIZE;                                         // the row's filter id: the f-th requested one
            f = f == 0 ? (with_n ? 0u : with_z ? 1u : 2u) : f == 1 ? (with_n && with_z ? 1u : 2u) : 2u;
            if (sum) atomicAdd(&hist[((size_t)f * ESIZE + row % ESIZE) * 256u + bin], (u64a)sum);
        }
        __syncthreads();
    };

    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK, b0 = (size_t)blockIdx.x * TRC_PLANES_BLOCK;
    const size_t turns = b0 < nv ? (nv - b0 + step - 1) / step : 0;      // of the whole workgroup: flush() holds barriers
    const M *el = (const M *)in;
    const u32 vseg = seg / TRC_PLANES_VEC, rstep = (u32)(step % vseg);
    u32 r = (u32)((b0 + tid) % vseg), since = 0;                         // the vector's place in its segment: 0 opens one
    size_t v = b0 + tid;
    for (size_t it = 0; it < turns; it++, v += step) {
        if (v < nv) {
            const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
            u32 w[NW], pw[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
#pragma unroll
            for (int q = 0; q < NQ; q++) {                               // the words that hold the last S elements of the vector in front
                uint4 x = make_uint4(0u, 0u, 0u, 0u);
                if (q >= Q0 && r) x = (src - NQ)[q];
                pw[4 * q] = x.x; pw[4 * q + 1] = x.y; pw[4 * q + 2] = x.z; pw[4 * q + 3] = x.w;
            }
            if (with_n) count_vec<ESIZE>(sm, row_n, cshift, w);
            T e[TRC_PLANES_VEC], pe[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
            unpack<ESIZE>(w, e);
            unpack<ESIZE>(pw, pe);
            if (with_z) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_ZDELTA>(e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
                pack<ESIZE>(y, w);
                count_vec<ESIZE>(sm, row_z, cshift, w);
            }
            if (with_x) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_XOR>(e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
                pack<ESIZE>(y, w);
                count_vec<ESIZE>(sm, row_x, cshift, w);
            }
        }
        r += rstep;
        if (r >= vseg) r -= vseg;
        if (++since == round_vecs && it + 1 < turns) { flush(); since = 0; }
    }
    // the elements behind the last whole vector (at most 7), one per lane
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC);
        if (tid < rest) {
            const size_t i = nv * TRC_PLANES_VEC + tid;
            const T x = (T)el[i], p = r0 + tid >= (u32)S ? (T)el[i - S] : (T)0;      // (r0 + tid >= S: i >= S)
            if (with_n) count_elem<ESIZE>(sm, row_n, cshift, x);
            if (with_z) count_elem<ESIZE>(sm, row_z, cshift, fwd<ESIZE, TRC_FILTER_ZDELTA>(x, p));
            if (with_x) count_elem<ESIZE>(sm, row_x, cshift, fwd<ESIZE, TRC_FILTER_XOR>(x, p));
        }
    }
    flush();
}

typedef void (*hist_fn)(const uint8_t *, size_t, u32, u32, u32, u32, u32, u64a *);
#define SHIST_STRIDES(E) { trc_splanes_hist_kernel<E, 2>, trc_splanes_hist_kernel<E, 3>, trc_splanes_hist_kernel<E, 4>, trc_splanes_hist_kernel<E, 5>, \
                           trc_splanes_hist_kernel<E, 6>, trc_splanes_hist_kernel<E, 7>, trc_splanes_hist_kernel<E, 8> }
static const hist_fn hist_kernels[3][TRC_STRIDE_MAX - 1] = { SHIST_STRIDES(2), SHIST_STRIDES(4), SHIST_STRIDES(8) };       // [esize 2 / 4 / 8][stride - 2]

extern "C" int trc_planes_hist_stride_dev(unsigned filters, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    if (stride < 1 || stride > TRC_STRIDE_MAX) return trc_fail(TRC_E_ARG, "planes_hist_stride: stride %d (1 .. %d)", stride, TRC_STRIDE_MAX);
    if (stride == 1 || !(filters & 6u) || filters > 7) return trc_planes_hist_dev(filters, d_in, n, esize, seg, d_hist, stream);
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "planes_hist_stride: restart length %u: must be a multiple of 64 in [%u,%u]", seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "planes_hist_stride: esize %u (2, 4 or 8)", esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "planes_hist_stride: %zu bytes hold no element of %u bytes", n, esize);
    if (!d_in || !d_hist || ((uintptr_t)d_in & 15) || ((uintptr_t)d_hist & 7))
        return trc_fail(TRC_E_ARG, "planes_hist_stride: the element buffer must be 16-byte, the histogram 8-byte aligned");
    const size_t m = n / esize;
    const uint32_t r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    const unsigned nf = (unsigned)__builtin_popcount(filters), rows = nf * esize;
    uint32_t cshift = 0;
    while ((2u << cshift) <= TRC_PHIST_COPIES_MAX && ((size_t)rows * 1024u << (cshift + 1)) <= TRC_PHIST_LDS) cshift++;
    const size_t lds = (size_t)rows * 1024u << cshift;
    uint32_t rv = TRC_PHIST_ROUND_VECS;                                  // TRC_PLANES_HIST_ROUND_VECS: as in trc_planes_hist_dev
    const char *e = getenv("TRC_PLANES_HIST_ROUND_VECS");
    if (e) { const long x = strtol(e, 0, 10); if (x >= 1 && x < (long)TRC_PHIST_ROUND_VECS) rv = (uint32_t)x; }
    unsigned grid = planes_grid(m);
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_bytes(esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "planes_hist_stride: %s", hipGetErrorString(he));
    hipLaunchKernelGGL(hist_kernels[esize == 2 ? 0 : esize == 4 ? 1 : 2][stride - 2], dim3(grid), dim3(TRC_PLANES_BLOCK), lds, s,
                       (const uint8_t *)d_in, m, seg, r0, filters, cshift, rv, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_hist_stride: %s", hipGetErrorString(he));
}
