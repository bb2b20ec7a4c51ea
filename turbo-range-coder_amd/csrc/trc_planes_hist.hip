// trc_planes_hist.hip -- the planes advisor's kernel: the order-0 byte histogram of every byte plane under every requested filter
// (none, zigzag delta, xor: include/trc_hip.h), from ONE read of the input.  It is the split kernel of trc_fplanes.hip with the
// plane stores replaced by counting: the same vector of 8 elements per thread, the same reach backwards for the S elements in front
// of it (S = the stride, 1 .. 8; the row of TRC_FILTER_NONE does not depend on it), the same grid-stride loop.  What it writes is
// 3 * esize * 256 counters, so that trc_planes_advise serves on its output as it stands.  The LDS counters, their layout and their
// flush are trc_planes_count.h's and are explained there.
#include "trc_planes_count.h"

// in: 16-byte aligned, m * ESIZE bytes are read, nothing in front of them.  seg: a multiple of 64.  r0 = (m / 8 * 8) % seg.  filters:
// bit f = count filter f, 1 .. 7 (S > 1: with bit 1 or 2 set).  hist[(f * ESIZE + k) * 256 + b] += the elements whose byte k under
// filter f is b; the rows of other filters are not touched.  Dynamic LDS: (requested filters * ESIZE * 256 * 4) << cshift bytes.
// round_vecs >= 1.
template <int ESIZE, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_kernel(const uint8_t *__restrict__ in, size_t m, u32 seg, u32 r0, u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const HistRows R = hist_rows<ESIZE>(sm, filters, cshift);

    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK, b0 = (size_t)blockIdx.x * TRC_PLANES_BLOCK;
    const size_t turns = b0 < nv ? (nv - b0 + step - 1) / step : 0;      // of the whole workgroup: the flush holds barriers
    const M *el = (const M *)in;
    const u32 vseg = seg / TRC_PLANES_VEC, rstep = (u32)(step % vseg);
    u32 r = (u32)((b0 + tid) % vseg), since = 0;                         // the vector's place in its segment: 0 opens one
    size_t v = b0 + tid;
    for (size_t it = 0; it < turns; it++, v += step) {
        if (v < nv) {
            const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            T pe[TRC_PLANES_VEC];
#pragma unroll
            for (int j = 0; j < TRC_PLANES_VEC; j++) pe[j] = 0;
            if (r && (filters & 6u)) {
                if constexpr (S == 1) pe[TRC_PLANES_VEC - 1] = el[v * TRC_PLANES_VEC - 1];
                else load_front<ESIZE, S>(in, v, pe);
            }
            count_filtered<ESIZE, S>(sm, R, cshift, w, pe);
        }
        r += rstep;
        if (r >= vseg) r -= vseg;
        if (++since == round_vecs && it + 1 < turns) { hist_flush<ESIZE>(sm, R, cshift, hist, false); since = 0; }
    }
    // the elements behind the last whole vector (at most 7), one per lane
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC);
        if (tid < rest) {
            const size_t i = nv * TRC_PLANES_VEC + tid;
            count_filtered_elem<ESIZE>(sm, R, cshift, (T)el[i], r0 + tid >= (u32)S ? (T)el[i - S] : (T)0);      // (r0 + tid >= S: i >= S)
        }
    }
    hist_flush<ESIZE>(sm, R, cshift, hist, false);
}

extern "C" size_t trc_planes_hist_bytes(unsigned esize)
{
    return esize_ok(esize) ? (size_t)TRC_PHIST_FILTERS * esize * 256 * sizeof(uint64_t) : 0;
}

typedef void (*hist_fn)(const uint8_t *, size_t, u32, u32, u32, u32, u32, u64a *);
#define HIST_STRIDES(E) { trc_planes_hist_kernel<E, 1>, trc_planes_hist_kernel<E, 2>, trc_planes_hist_kernel<E, 3>, trc_planes_hist_kernel<E, 4>, \
                          trc_planes_hist_kernel<E, 5>, trc_planes_hist_kernel<E, 6>, trc_planes_hist_kernel<E, 7>, trc_planes_hist_kernel<E, 8> }
static const hist_fn hist_kernels[3][TRC_STRIDE_MAX] = { HIST_STRIDES(2), HIST_STRIDES(4), HIST_STRIDES(8) };       // [esize_row][stride - 1]

// stride 1 .. TRC_STRIDE_MAX, vetted by the caller; `who` names the call in every message
static int hist_run(const char *who, unsigned filters, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    if (filters < 1 || filters > 7) return trc_fail(TRC_E_ARG, "%s: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", who, filters);
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "%s: restart length %u: must be a multiple of 64 in [%u,%u]", who, seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "%s: esize %u (2, 4 or 8)", who, esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "%s: %zu bytes hold no element of %u bytes", who, n, esize);
    if (!d_in || !d_hist || ((uintptr_t)d_in & 15) || ((uintptr_t)d_hist & 7))
        return trc_fail(TRC_E_ARG, "%s: the element buffer must be 16-byte, the histogram 8-byte aligned", who);
    const size_t m = n / esize;
    const uint32_t r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    const HistShape h = hist_shape(filters, esize);
    unsigned grid = planes_grid(m);
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_bytes(esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
    hipLaunchKernelGGL(hist_kernels[esize_row(esize)][stride - 1], dim3(grid), dim3(TRC_PLANES_BLOCK), h.lds, s,
                       (const uint8_t *)d_in, m, seg, r0, filters, h.cshift, h.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
}

extern "C" int trc_planes_hist_dev(unsigned filters, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    return hist_run("planes_hist", filters, 1, d_in, n, esize, seg, d_hist, stream);
}

// (a call that counts no predicted row, or whose filters are out of range, is the stride-1 call and says so in its messages)
extern "C" int trc_planes_hist_stride_dev(unsigned filters, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    if (stride < 1 || stride > TRC_STRIDE_MAX) return trc_fail(TRC_E_ARG, "planes_hist_stride: stride %d (1 .. %d)", stride, TRC_STRIDE_MAX);
    if (stride == 1 || !(filters & 6u) || filters > 7) return hist_run("planes_hist", filters, 1, d_in, n, esize, seg, d_hist, stream);
    return hist_run("planes_hist_stride", filters, stride, d_in, n, esize, seg, d_hist, stream);
}
