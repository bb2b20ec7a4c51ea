// trc_planes_order.h -- what the kernels behind a fixed polynomial predictor of ORDER 2 or 3 share (trc_oplanes.hip: one buffer;
// trc_oplanes_batch.inc: the items of a batch, an order per item): the reach of a vector's difference into the vectors in front of it
// and its loads, the difference itself in registers and from memory, and the LDS rows of the histograms of orders 0 .. 3 with their
// flushes.  The definition is in trc_oplanes.hip and include/trc_hip.h.
#ifndef TRC_PLANES_ORDER_H
#define TRC_PLANES_ORDER_H
#include "trc_planes_scan.h"
#include "trc_planes_count.h"

// the 8 elements of vector v at a[0 .. 7]; only the 16-byte words that hold element FROM and those behind it are loaded
template <int ESIZE, int FROM> __device__ __forceinline__ void load_vec_from(const uint8_t *__restrict__ in, size_t v, typename Elem<ESIZE>::T *a)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4, Q0 = FROM * ESIZE / 16;
    const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
    u32 w[NW];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (q >= Q0) x = src[q];
        w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
    }
    unpack<ESIZE>(w, a);
}

// what a vector's ORDER-th difference needs in front of it: NF whole vectors, the farthest from its element FROM on; a[B + j] is
// the vector's own element j
template <int ORDER, int S> struct Reach {
    static constexpr int R = ORDER * S, NF = (R + TRC_PLANES_VEC - 1) / TRC_PLANES_VEC, B = NF * TRC_PLANES_VEC, FROM = B - R;
};

// the vectors in front of vector v into a[0 .. B): vector f in front where f <= r (r = the vector's place in its segment) and
// f <= need, zeros elsewhere
template <int ESIZE, int ORDER, int S> __device__ __forceinline__ void load_reach(const uint8_t *__restrict__ in, size_t v, u32 r, u32 need, typename Elem<ESIZE>::T *a)
{
    typedef Reach<ORDER, S> Q;
#pragma unroll
    for (int j = 0; j < Q::B; j++) a[j] = 0;
    if (r >= 1u && need >= 1u) load_vec_from<ESIZE, Q::NF == 1 ? Q::FROM : 0>(in, v - 1, a + Q::B - TRC_PLANES_VEC);
    if constexpr (Q::NF >= 2) { if (r >= 2u && need >= 2u) load_vec_from<ESIZE, Q::NF == 2 ? Q::FROM : 0>(in, v - 2, a + Q::B - 2 * TRC_PLANES_VEC); }
    if constexpr (Q::NF >= 3) { if (r >= 3u && need >= 3u) load_vec_from<ESIZE, Q::FROM>(in, v - 3, a + Q::B - 3 * TRC_PLANES_VEC); }
}

// the ORDER-th difference at a[0] of a series whose element S * j back is a[-S * j]: mod 2^64 or 2^32, the caller drops what lies
// above the element's width
template <int ORDER, int S, typename T> __device__ __forceinline__ T diff(const T *a)
{
    if constexpr (ORDER == 0) return a[0];
    else if constexpr (ORDER == 1) return a[0] - a[-S];
    else if constexpr (ORDER == 2) return a[0] - 2 * a[-S] + a[-2 * S];
    else return a[0] - 3 * a[-S] + 3 * a[-2 * S] - a[-3 * S];
}
// the same for one element i at place `at` of its segment, from memory: the terms that reach in front of the segment are zero
// (at >= j * S: i >= j * S)
template <int ORDER, typename T, typename M> __device__ __forceinline__ T diff_elem(const M *el, size_t i, u32 at, u32 s)
{
    constexpr int C[4][4] = { { 1, 0, 0, 0 }, { 1, 1, 0, 0 }, { 1, 2, 1, 0 }, { 1, 3, 3, 1 } };
    T d = (T)el[i];
#pragma unroll
    for (int j = 1; j <= ORDER; j++) {
        const T x = at >= (u32)j * s ? (T)el[i - (size_t)j * s] : (T)0;
        d = j & 1 ? d - (T)C[ORDER][j] * x : d + (T)C[ORDER][j] * x;
    }
    return d;
}
template <int ESIZE> __device__ __forceinline__ typename Elem<ESIZE>::T zigzag(typename Elem<ESIZE>::T d)
{
    return fwd<ESIZE, TRC_FILTER_ZDELTA>(d, (typename Elem<ESIZE>::T)0);
}

// ---- the histograms of orders 0 .. 3 --------------------------------------------------------------------------------------------
// A workgroup's counters are trc_planes_count.h's [row][bin][copy] with the requested orders packed in the order of their ids:
// 4 orders of esize 2 / 4 / 8 take 4 / 2 / 1 copies (hist_shape), 32 KiB each way, inside the 48 KiB that header budgets, so
// three workgroups still share a CU.
#define TRC_OHIST_ORDERS 4u
struct OrderRows { u32 nf, row[TRC_OHIST_ORDERS]; };                     // where the rows of order k start, the lane's copy included

template <int ESIZE> __device__ __forceinline__ OrderRows order_rows(u32 *sm, u32 orders, u32 cshift)
{
    const u32 tid = threadIdx.x, copy = tid & ((1u << cshift) - 1u), fwords = (ESIZE * 256u) << cshift;
    OrderRows R;
    R.nf = __builtin_popcount(orders);
#pragma unroll
    for (u32 k = 0; k < TRC_OHIST_ORDERS; k++) R.row[k] = copy + fwords * (u32)__builtin_popcount(orders & ((1u << k) - 1u));
    for (u32 i = tid; i < R.nf * fwords; i += TRC_PLANES_BLOCK) sm[i] = 0;
    __syncthreads();
    return R;
}
// the workgroup's counters to the global rows and zero again (hist_flush of trc_planes_count.h, with the row's order looked up in
// the bit set); the whole workgroup calls it
template <int ESIZE> __device__ __forceinline__ void order_flush(u32 *sm, u32 nf, u32 orders, u32 cshift, u64a *h)
{
    __syncthreads();
    for (u32 i = threadIdx.x; i < nf * ESIZE * 256u; i += TRC_PLANES_BLOCK) {
        const u32 row = i >> 8, bin = ((i & 255u) + 37u * blockIdx.x) & 255u;
        u32 *c = sm + ((row * 256u + bin) << cshift);
        u32 sum = 0;
        for (u32 q = 0; q < (1u << cshift); q++) { sum += c[q]; c[q] = 0; }
        u32 left = row / ESIZE, k = 0;                                   // the row's order: the left-th requested one
        for (u32 b = orders; !(b & 1u) || left; b >>= 1, k++) if (b & 1u) left--;
        if (sum) atomicAdd(&h[((size_t)k * ESIZE + row % ESIZE) * 256u + bin], (u64a)sum);
    }
    __syncthreads();
}
// the same into the rows of one item of a batch; store: nobody else adds to these rows and nothing has been added to them yet, so
// the sums are stored, zeros included (hist_flush's rule, trc_planes_count.h)
template <int ESIZE> __device__ __forceinline__ void order_flush_item(u32 *sm, u32 nf, u32 orders, u32 cshift, u64a *h, bool store)
{
    __syncthreads();
    for (u32 i = threadIdx.x; i < nf * ESIZE * 256u; i += TRC_PLANES_BLOCK) {
        const u32 row = i >> 8, bin = ((i & 255u) + 37u * blockIdx.x) & 255u;
        u32 *c = sm + ((row * 256u + bin) << cshift);
        u32 sum = 0;
        for (u32 q = 0; q < (1u << cshift); q++) { sum += c[q]; c[q] = 0; }
        u32 left = row / ESIZE, k = 0;
        for (u32 b = orders; !(b & 1u) || left; b >>= 1, k++) if (b & 1u) left--;
        u64a *dst = &h[((size_t)k * ESIZE + row % ESIZE) * 256u + bin];
        if (store) *dst = (u64a)sum;
        else if (sum) atomicAdd(dst, (u64a)sum);
    }
    __syncthreads();
}

#endif
