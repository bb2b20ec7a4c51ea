// trc_planes_hist.hip -- the planes advisor's kernel: the order-0 byte histogram of every byte plane under every requested filter
// (none, zigzag delta, xor: include/trc_hip.h), from ONE read of the input.  It is the split kernel of trc_fplanes.hip with the
// plane stores replaced by counting: the same vector of 8 elements per thread, the same predecessor load, the same grid-stride loop.
// What it writes is 3 * esize * 256 counters.
//
// LDS layout and why.  A workgroup counts into [row][bin][copy] of u32, row = (requested filter, plane), with R copies of every bin
// side by side and lane l adding to copy l & (R - 1).  R is the largest power of two that keeps the rows within 48 KiB, at most 16
// (3 filters: 8 / 4 / 2 copies for esize 2 / 4 / 8; one filter: 16 / 8 / 4), so three workgroups (12 waves) share a CU's 160 KiB.
//   - The planes that matter for the decision are the skewed ones: the sign / exponent byte of weights, the high planes of a
//     filtered series.  There most lanes of a wave meet on one bin, and a ds_add_u32 serialises on lanes that share an ADDRESS (the
//     project's first histogram, shared copies, serialised on text's most frequent symbol: trc_dir.hip).  Copies next to each other
//     put the lanes of one bin on R different banks: the worst case is 32 / R lanes per address within an LDS lane group.
//   - trc_hist2_kernel's per-wave copies with packed 16-bit counters need 8 KiB per row and wave; 24 rows do not fit.  Copies are
//     shared by the workgroup's four waves instead (LDS atomics are atomic across waves; only lanes of ONE instruction collide).
//   - Aggregating equal bytes across the wave ahead of the add needs a match-any, which gfx950 has only as a loop of
//     readfirstlane / ballot steps: up to 64 turns on the uniform planes, which are half of all planes.  What is cheap is the
//     aggregation within the THREAD: where the 8 bytes a thread holds of a plane are equal (two compares), it adds 8 once.  That is
//     the common case exactly where contention is worst (constant and near-constant planes), and it cuts those adds eightfold.
// Counters are 32-bit; a workgroup adds 2048 per turn of its loop to a row, so it flushes to the 64-bit global histogram every
// TRC_PHIST_ROUND_VECS turns (2^20: a counter stays below 2^31) and once at the end, one 64-bit atomicAdd per non-zero bin, the
// bins rotated by the workgroup's number as in trc_hist2_kernel so that the workgroups do not walk the global rows in step.
// The grid is capped at what is resident (3 workgroups on each of 256 CUs) on top of the TRC_PLANES_GRID cap: every workgroup ends
// with up to rows * 256 global atomics, so more workgroups than that only add flushes.
#include "trc_planes_count.h"                     // the LDS counters' shape and the adds into them, shared with the batched kernel

// in: 16-byte aligned, m * ESIZE bytes are read.  seg: a multiple of 64.  r0 = (m / 8 * 8) % seg.  filters: bit f = count filter f,
// 1 .. 7.  hist[(f * ESIZE + k) * 256 + b] += the elements whose byte k under filter f is b; the rows of other filters are not
// touched.  Dynamic LDS: (requested filters * ESIZE * 256 * 4) << cshift bytes.  round_vecs >= 1.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_kernel(const uint8_t *__restrict__ in, size_t m, u32 seg, u32 r0, u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
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
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            T prev = 0;
            if (r && (filters & 6u)) prev = el[v * TRC_PLANES_VEC - 1];
            if (with_n) count_vec<ESIZE>(sm, row_n, cshift, w);
            if (filters & 6u) {
                T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
                unpack<ESIZE>(w, e);
                if (with_z) {
#pragma unroll
                    for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_ZDELTA>(e[j], j ? e[j - 1] : prev);
                    pack<ESIZE>(y, w);
                    count_vec<ESIZE>(sm, row_z, cshift, w);
                }
                if (with_x) {
#pragma unroll
                    for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_XOR>(e[j], j ? e[j - 1] : prev);
                    pack<ESIZE>(y, w);
                    count_vec<ESIZE>(sm, row_x, cshift, w);
                }
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
            const T x = (T)el[i], p = r0 + tid ? (T)el[i - 1] : (T)0;
            if (with_n) count_elem<ESIZE>(sm, row_n, cshift, x);
            if (with_z) count_elem<ESIZE>(sm, row_z, cshift, fwd<ESIZE, TRC_FILTER_ZDELTA>(x, p));
            if (with_x) count_elem<ESIZE>(sm, row_x, cshift, fwd<ESIZE, TRC_FILTER_XOR>(x, p));
        }
    }
    flush();
}

extern "C" size_t trc_planes_hist_bytes(unsigned esize)
{
    return esize_ok(esize) ? (size_t)TRC_PHIST_FILTERS * esize * 256 * sizeof(uint64_t) : 0;
}

extern "C" int trc_planes_hist_dev(unsigned filters, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    if (filters < 1 || filters > 7) return trc_fail(TRC_E_ARG, "planes_hist: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", filters);
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "planes_hist: restart length %u: must be a multiple of 64 in [%u,%u]", seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "planes_hist: esize %u (2, 4 or 8)", esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "planes_hist: %zu bytes hold no element of %u bytes", n, esize);
    if (!d_in || !d_hist || ((uintptr_t)d_in & 15) || ((uintptr_t)d_hist & 7))
        return trc_fail(TRC_E_ARG, "planes_hist: the element buffer must be 16-byte, the histogram 8-byte aligned");
    const size_t m = n / esize;
    const uint32_t r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    const unsigned nf = (unsigned)__builtin_popcount(filters), rows = nf * esize;
    uint32_t cshift = 0;
    while ((2u << cshift) <= TRC_PHIST_COPIES_MAX && ((size_t)rows * 1024u << (cshift + 1)) <= TRC_PHIST_LDS) cshift++;
    const size_t lds = (size_t)rows * 1024u << cshift;
    // TRC_PLANES_HIST_ROUND_VECS (test aid): vectors per thread between two flushes, so that a few hundred KB flush more than once
    uint32_t rv = TRC_PHIST_ROUND_VECS;
    const char *e = getenv("TRC_PLANES_HIST_ROUND_VECS");
    if (e) { const long x = strtol(e, 0, 10); if (x >= 1 && x < (long)TRC_PHIST_ROUND_VECS) rv = (uint32_t)x; }
    unsigned grid = planes_grid(m);
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_bytes(esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "planes_hist: %s", hipGetErrorString(he));
    const dim3 g(grid), b(TRC_PLANES_BLOCK);
    if (esize == 2) hipLaunchKernelGGL((trc_planes_hist_kernel<2>), g, b, lds, s, (const uint8_t *)d_in, m, seg, r0, filters, cshift, rv, (u64a *)d_hist);
    else if (esize == 4) hipLaunchKernelGGL((trc_planes_hist_kernel<4>), g, b, lds, s, (const uint8_t *)d_in, m, seg, r0, filters, cshift, rv, (u64a *)d_hist);
    else hipLaunchKernelGGL((trc_planes_hist_kernel<8>), g, b, lds, s, (const uint8_t *)d_in, m, seg, r0, filters, cshift, rv, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_hist: %s", hipGetErrorString(he));
}
