// trc_planes_vec.h -- what the plane kernels share: the byte separation of one thread's vector of 8 elements in registers, the
// filters' forward step over a vector, the launch shape, the kernel tables' row and the argument rules.
//   trc_planes.hip              split / join
//   trc_fplanes.hip             the same behind a zigzag-delta or xor filter, of every stride (join: trc_planes_scan.h)
//   trc_bplanes.hip             the same behind a zigzag-delta or xor filter against a BASE buffer (elementwise both ways), the
//                               advisor's histograms against a base, the base's fingerprint
//   trc_planes_hist.hip         the advisor's histograms of the filtered planes, of every stride (trc_planes_count.h)
//   trc_oplanes.hip             split / join behind a predictor of order 2 or 3, of every stride (join: trc_planes_scan.h), and the
//                               advisor's histograms of orders 0 .. 3
//   trc_planes_batch.hip        split / join over a table of separate allocations; includes
//     trc_fplanes_batch.inc       the same with a filter per item (join: trc_planes_scan.h)
//     trc_bplanes_batch.inc       the same with a filter against a base per item (join: elementwise)
//     trc_splanes_batch.inc       the same with a filter and a stride per item: split, join, histograms
//     trc_planes_hist_batch.inc   the advisor's histograms per item (trc_planes_count.h)
//   trc_planes_pack.hip         the batch container's packing (trc_planes_pack.h)
#ifndef TRC_PLANES_VEC_H
#define TRC_PLANES_VEC_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/trc_hip.h"

int trc_fail(int code, const char *fmt, ...);      // trc_api.hip: sets trc_last_error(), prints, returns code

#define TRC_PLANES_BLOCK 256
#define TRC_PLANES_GRID_MAX 2048u
#define TRC_PLANES_VEC 8                            // elements per thread and step

typedef uint32_t u32;

// v_perm_b32: byte j of the result is byte sel[j] of the 8 bytes { hi : lo } (0..3 = lo, 4..7 = hi)
__device__ __forceinline__ u32 perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// 4 x 4 byte transpose: out[k] byte j = w[j] byte k.  Its own inverse.
__device__ __forceinline__ void tr4(u32 w0, u32 w1, u32 w2, u32 w3, u32 &o0, u32 &o1, u32 &o2, u32 &o3)
{
    const u32 p_lo = perm(w1, w0, 0x05010400u), p_hi = perm(w1, w0, 0x07030602u);   // (w0.b0 w1.b0 w0.b1 w1.b1), (w0.b2 w1.b2 w0.b3 w1.b3)
    const u32 q_lo = perm(w3, w2, 0x05010400u), q_hi = perm(w3, w2, 0x07030602u);
    o0 = perm(q_lo, p_lo, 0x05040100u); o1 = perm(q_lo, p_lo, 0x07060302u);
    o2 = perm(q_hi, p_hi, 0x05040100u); o3 = perm(q_hi, p_hi, 0x07060302u);
}

// one vector: W = the 2 * ESIZE input words of 8 elements, P[k] = the 8 bytes of plane k
template <int ESIZE> __device__ __forceinline__ void vec_split(const u32 *w, uint2 *p)
{
    if constexpr (ESIZE == 2) {                    // a word = two elements (lo0 hi0 lo1 hi1)
        p[0].x = perm(w[1], w[0], 0x06040200u); p[1].x = perm(w[1], w[0], 0x07050301u);
        p[0].y = perm(w[3], w[2], 0x06040200u); p[1].y = perm(w[3], w[2], 0x07050301u);
    } else if constexpr (ESIZE == 4) {             // a word = one element
        tr4(w[0], w[1], w[2], w[3], p[0].x, p[1].x, p[2].x, p[3].x);
        tr4(w[4], w[5], w[6], w[7], p[0].y, p[1].y, p[2].y, p[3].y);
    } else {                                       // element i = words 2i (planes 0..3) and 2i + 1 (planes 4..7)
        tr4(w[0], w[2], w[4], w[6], p[0].x, p[1].x, p[2].x, p[3].x);
        tr4(w[1], w[3], w[5], w[7], p[4].x, p[5].x, p[6].x, p[7].x);
        tr4(w[8], w[10], w[12], w[14], p[0].y, p[1].y, p[2].y, p[3].y);
        tr4(w[9], w[11], w[13], w[15], p[4].y, p[5].y, p[6].y, p[7].y);
    }
}
template <int ESIZE> __device__ __forceinline__ void vec_join(const uint2 *p, u32 *w)
{
    if constexpr (ESIZE == 2) {
        w[0] = perm(p[1].x, p[0].x, 0x05010400u); w[1] = perm(p[1].x, p[0].x, 0x07030602u);
        w[2] = perm(p[1].y, p[0].y, 0x05010400u); w[3] = perm(p[1].y, p[0].y, 0x07030602u);
    } else if constexpr (ESIZE == 4) {
        tr4(p[0].x, p[1].x, p[2].x, p[3].x, w[0], w[1], w[2], w[3]);
        tr4(p[0].y, p[1].y, p[2].y, p[3].y, w[4], w[5], w[6], w[7]);
    } else {
        tr4(p[0].x, p[1].x, p[2].x, p[3].x, w[0], w[2], w[4], w[6]);
        tr4(p[4].x, p[5].x, p[6].x, p[7].x, w[1], w[3], w[5], w[7]);
        tr4(p[0].y, p[1].y, p[2].y, p[3].y, w[8], w[10], w[12], w[14]);
        tr4(p[4].y, p[5].y, p[6].y, p[7].y, w[9], w[11], w[13], w[15]);
    }
}

// ---- what the filter kernels share (split / join, the advisor's histograms)
template <int ESIZE> struct Elem { typedef u32 T; typedef u32 M; };          // T: the register type of an element, M: its type in memory
template <> struct Elem<2> { typedef u32 T; typedef uint16_t M; };           // (16-bit elements are computed in 32 bits and truncated when packed)
template <> struct Elem<8> { typedef uint64_t T; typedef uint64_t M; };

// the 8 elements of a vector from / to its 2 * ESIZE words
template <int ESIZE> __device__ __forceinline__ void unpack(const u32 *w, typename Elem<ESIZE>::T *e)
{
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) {
        if constexpr (ESIZE == 2) e[j] = j & 1 ? w[j / 2] >> 16 : w[j / 2] & 0xffffu;
        else if constexpr (ESIZE == 4) e[j] = w[j];
        else e[j] = (uint64_t)w[2 * j] | (uint64_t)w[2 * j + 1] << 32;
    }
}
template <int ESIZE> __device__ __forceinline__ void pack(const typename Elem<ESIZE>::T *e, u32 *w)
{
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) {
        if constexpr (ESIZE == 2) { if (j & 1) w[j / 2] = (e[j - 1] & 0xffffu) | e[j] << 16; }
        else if constexpr (ESIZE == 4) w[j] = e[j];
        else { w[2 * j] = (u32)e[j]; w[2 * j + 1] = (u32)(e[j] >> 32); }
    }
}

// y of x and its predecessor: clean in the element's width
template <int ESIZE, int FILTER> __device__ __forceinline__ typename Elem<ESIZE>::T fwd(typename Elem<ESIZE>::T x, typename Elem<ESIZE>::T p)
{
    typedef typename Elem<ESIZE>::T T;
    constexpr int W = 8 * ESIZE;
    constexpr T MASK = (T)~(T)0 >> (8 * sizeof(T) - W);
    if constexpr (FILTER == TRC_FILTER_XOR) return x ^ p;
    const T d = (x - p) & MASK;
    return ((d << 1) ^ ((T)0 - (d >> (W - 1)))) & MASK;
}

// x of y and the predictor, where the predictor is at hand and no scan is needed (trc_bplanes.hip): clean in the element's width
template <int ESIZE, int FILTER> __device__ __forceinline__ typename Elem<ESIZE>::T inv(typename Elem<ESIZE>::T y, typename Elem<ESIZE>::T p)
{
    typedef typename Elem<ESIZE>::T T;
    constexpr int W = 8 * ESIZE;
    constexpr T MASK = (T)~(T)0 >> (8 * sizeof(T) - W);
    if constexpr (FILTER == TRC_FILTER_XOR) return y ^ p;
    return (p + ((y >> 1) ^ ((T)0 - (y & 1)))) & MASK;
}

// the last S elements of the vector in front of vector v, at pe[8 - S .. 7]; only the 16-byte words that hold them are loaded
template <int ESIZE, int S> __device__ __forceinline__ void load_front(const uint8_t *__restrict__ in, size_t v, typename Elem<ESIZE>::T *pe)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4, Q0 = NQ - (S * ESIZE + 15) / 16;
    const uint4 *src = (const uint4 *)(in + (v - 1) * (TRC_PLANES_VEC * ESIZE));
    u32 w[NW];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (q >= Q0) x = src[q];
        w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
    }
    unpack<ESIZE>(w, pe);
}

// workgroups of a launch over m elements; TRC_PLANES_GRID in the environment lowers the cap (tuning aid, and how the tests make
// a small input take the grid-stride loop more than once)
static unsigned planes_grid_cap()
{
    unsigned cap = TRC_PLANES_GRID_MAX;
    const char *e = getenv("TRC_PLANES_GRID");
    if (e) { const long v = strtol(e, 0, 10); if (v >= 1 && v < (long)TRC_PLANES_GRID_MAX) cap = (unsigned)v; }
    return cap;
}
static unsigned planes_grid(size_t m)
{
    const size_t nv = m / TRC_PLANES_VEC, want = (nv + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK;
    const unsigned cap = planes_grid_cap();
    return want < 1 ? 1u : want > cap ? cap : (unsigned)want;
}

static bool esize_ok(unsigned esize) { return esize == 2 || esize == 4 || esize == 8; }

// kernels are picked from tables: [esize_row(esize)], then [filter - 1] and [stride - 1] where a kernel has them
static int esize_row(unsigned esize) { return esize == 2 ? 0 : esize == 4 ? 1 : 2; }
#define TRC_BY_ESIZE(K) { K<2>, K<4>, K<8> }

static int planes_args(const char *who, const void *d_flat, size_t n, unsigned esize, const void *d_planes, size_t pitch, const void *d_tail)
{
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "%s: esize %u (2, 4 or 8)", who, esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "%s: %zu bytes hold no element of %u bytes", who, n, esize);
    if (!d_flat || !d_planes || ((uintptr_t)d_flat & 15) || ((uintptr_t)d_planes & 255))
        return trc_fail(TRC_E_ARG, "%s: the element buffer must be 16-byte, the planes 256-byte aligned", who);
    if ((pitch & 255) || pitch < n / esize) return trc_fail(TRC_E_ARG, "%s: pitch %zu must be a multiple of 256 and at least %zu", who, pitch, n / esize);
    if (n % esize && !d_tail) return trc_fail(TRC_E_ARG, "%s: %zu tail bytes and no tail buffer", who, n % esize);
    return TRC_OK;
}

#endif
