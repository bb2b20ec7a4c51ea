// trc_planes_count.h -- what the histogram kernels of the planes advisor share (trc_planes_hist.hip: one buffer, every stride;
// trc_planes_hist_batch.inc: the items of a batch): the shape of a workgroup's LDS counters, the adds into them, their flush to the
// global histogram, and the host's choice of that shape.
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
#ifndef TRC_PLANES_COUNT_H
#define TRC_PLANES_COUNT_H
#include "trc_planes_vec.h"

#define TRC_PHIST_LDS (48u * 1024u)
#define TRC_PHIST_COPIES_MAX 16u
#define TRC_PHIST_GRID_MAX 768u
#define TRC_PHIST_ROUND_VECS (1u << 20)             // vectors per thread between two flushes: 2^20 * 256 * 8 = 2^31 per row
#define TRC_PHIST_FILTERS 3u

typedef unsigned long long u64a;

__device__ __forceinline__ void lds_add(u32 *p, u32 v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the 8 bytes a thread holds of one plane into the row that starts at word `row` (the lane's copy included)
__device__ __forceinline__ void count_plane(u32 *sm, u32 row, u32 cshift, uint2 p)
{
    const u32 b0 = p.x & 0xffu;
    if (p.x == p.y && p.x == b0 * 0x01010101u) { lds_add(sm + row + (b0 << cshift), TRC_PLANES_VEC); return; }
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++)
        lds_add(sm + row + (__builtin_amdgcn_ubfe(j < 4 ? p.x : p.y, 8 * (j & 3), 8) << cshift), 1u);
}
template <int ESIZE> __device__ __forceinline__ void count_vec(u32 *sm, u32 row, u32 cshift, const u32 *w)
{
    uint2 p[ESIZE];
    vec_split<ESIZE>(w, p);
#pragma unroll
    for (int k = 0; k < ESIZE; k++) count_plane(sm, row + ((u32)k << (8 + cshift)), cshift, p[k]);
}
template <int ESIZE> __device__ __forceinline__ void count_elem(u32 *sm, u32 row, u32 cshift, typename Elem<ESIZE>::T y)
{
#pragma unroll
    for (int k = 0; k < ESIZE; k++) lds_add(sm + row + ((u32)k << (8 + cshift)) + (((u32)(y >> (8 * k)) & 0xffu) << cshift), 1u);
}


// a workgroup's counters as one lane sees them: where the rows of filter f start, the lane's copy included (the requested filters
// lie packed, in the order of their ids)
struct HistRows {
    u32 nf, row_n, row_z, row_x;
    bool with_n, with_z, with_x;
};

// sm: (requested filters * ESIZE * 256 * 4) << cshift bytes of dynamic LDS, zeroed here; the whole workgroup calls it
template <int ESIZE> __device__ __forceinline__ HistRows hist_rows(u32 *sm, u32 filters, u32 cshift)
{
    const u32 tid = threadIdx.x, copy = tid & ((1u << cshift) - 1u);
    const u32 nf = __builtin_popcount(filters), words = (nf * ESIZE * 256u) << cshift, fwords = (ESIZE * 256u) << cshift;
    HistRows R;
    R.nf = nf;
    R.row_n = copy; R.row_z = R.row_n + (filters & 1u ? fwords : 0u); R.row_x = R.row_z + (filters & 2u ? fwords : 0u);
    R.with_n = filters & 1u; R.with_z = filters & 2u; R.with_x = filters & 4u;
    for (u32 i = tid; i < words; i += TRC_PLANES_BLOCK) sm[i] = 0;
    __syncthreads();
    return R;
}

// the workgroup's counters to the global rows h of one buffer or item, and zero again; the whole workgroup calls it.  store: nobody
// else adds to these rows and nothing has been added to them yet, so the sums are stored, zeros included
template <int ESIZE> __device__ __forceinline__ void hist_flush(u32 *sm, const HistRows &R, u32 cshift, u64a *h, bool store)
{
    __syncthreads();
    for (u32 i = threadIdx.x; i < R.nf * ESIZE * 256u; i += TRC_PLANES_BLOCK) {
        const u32 row = i >> 8, bin = ((i & 255u) + 37u * blockIdx.x) & 255u;
        u32 *c = sm + ((row * 256u + bin) << cshift);
        u32 sum = 0;
        for (u32 q = 0; q < (1u << cshift); q++) { sum += c[q]; c[q] = 0; }
        u32 f = row / ESIZE;                                             // the row's filter id: the f-th requested one
        f = f == 0 ? (R.with_n ? 0u : R.with_z ? 1u : 2u) : f == 1 ? (R.with_n && R.with_z ? 1u : 2u) : 2u;
        u64a *dst = &h[((size_t)f * ESIZE + row % ESIZE) * 256u + bin];
        if (store) *dst = (u64a)sum;
        else if (sum) atomicAdd(dst, (u64a)sum);
    }
    __syncthreads();
}

// a whole vector (its words w, which are used up) under every requested filter at stride S; pe[8 - S .. 7] = the last S elements of
// the vector in front of it, zeros where the vector opens a segment
template <int ESIZE, int S> __device__ __forceinline__ void count_filtered(u32 *sm, const HistRows &R, u32 cshift, u32 *w, const typename Elem<ESIZE>::T *pe)
{
    typedef typename Elem<ESIZE>::T T;
    if (R.with_n) count_vec<ESIZE>(sm, R.row_n, cshift, w);
    T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    unpack<ESIZE>(w, e);
    if (R.with_z) {
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_ZDELTA>(e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
        pack<ESIZE>(y, w);
        count_vec<ESIZE>(sm, R.row_z, cshift, w);
    }
    if (R.with_x) {
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_XOR>(e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
        pack<ESIZE>(y, w);
        count_vec<ESIZE>(sm, R.row_x, cshift, w);
    }
}
// the same with the predictor of every element given, not derived from the vector: p[j] predicts element j (trc_bplanes.hip)
template <int ESIZE> __device__ __forceinline__ void count_predicted(u32 *sm, const HistRows &R, u32 cshift, u32 *w, const typename Elem<ESIZE>::T *p)
{
    typedef typename Elem<ESIZE>::T T;
    if (R.with_n) count_vec<ESIZE>(sm, R.row_n, cshift, w);
    T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    unpack<ESIZE>(w, e);
    if (R.with_z) {
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_ZDELTA>(e[j], p[j]);
        pack<ESIZE>(y, w);
        count_vec<ESIZE>(sm, R.row_z, cshift, w);
    }
    if (R.with_x) {
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, TRC_FILTER_XOR>(e[j], p[j]);
        pack<ESIZE>(y, w);
        count_vec<ESIZE>(sm, R.row_x, cshift, w);
    }
}
// one element x with its predecessor p (0 where it has none)
template <int ESIZE> __device__ __forceinline__ void count_filtered_elem(u32 *sm, const HistRows &R, u32 cshift, typename Elem<ESIZE>::T x, typename Elem<ESIZE>::T p)
{
    if (R.with_n) count_elem<ESIZE>(sm, R.row_n, cshift, x);
    if (R.with_z) count_elem<ESIZE>(sm, R.row_z, cshift, fwd<ESIZE, TRC_FILTER_ZDELTA>(x, p));
    if (R.with_x) count_elem<ESIZE>(sm, R.row_x, cshift, fwd<ESIZE, TRC_FILTER_XOR>(x, p));
}

// ---- host: the shape of a launch that counts `filters` (a bit set) of `esize`-byte elements
struct HistShape {
    u32 cshift, round_vecs;                        // copies per bin = 1 << cshift; vectors per thread between two flushes
    size_t lds;
};
static HistShape hist_shape(unsigned filters, unsigned esize)
{
    const unsigned rows = (unsigned)__builtin_popcount(filters) * esize;
    HistShape h = { 0, TRC_PHIST_ROUND_VECS, 0 };
    while ((2u << h.cshift) <= TRC_PHIST_COPIES_MAX && ((size_t)rows * 1024u << (h.cshift + 1)) <= TRC_PHIST_LDS) h.cshift++;
    h.lds = (size_t)rows * 1024u << h.cshift;
    // TRC_PLANES_HIST_ROUND_VECS (test aid): a lower round_vecs, so that a few hundred KB flush more than once
    const char *e = getenv("TRC_PLANES_HIST_ROUND_VECS");
    if (e) { const long x = strtol(e, 0, 10); if (x >= 1 && x < (long)TRC_PHIST_ROUND_VECS) h.round_vecs = (u32)x; }
    return h;
}

#endif
