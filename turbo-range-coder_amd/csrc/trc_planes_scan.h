// trc_planes_scan.h -- the scanning join of the filtered byte planes: what it is, and the pieces that trc_fplanes_join_kernel
// (trc_fplanes.hip: one buffer, every stride), trc_fplanes_join_batch_kernel (trc_fplanes_batch.inc: the items of a batch, a filter
// per item) and trc_splanes_join_batch_kernel (trc_splanes_batch.inc: a filter and a stride per item) share.
//
// A join with a predictor filter undoes a prefix sum (or prefix xor) that restarts every seg elements.  One WAVE walks one segment in
// tiles of 512 elements, 8 per lane: join the planes' bytes to elements, undo the zigzag, scan the lane's 8 serially, scan the 64
// lane totals across the wave (six __shfl_up steps), add the value carried out of the previous tile and store 16-byte words.  A
// tile's loads do not depend on the carry, so the loads of the wave's NEXT tile -- of the same segment or of the wave's next segment
// -- are issued before the current tile is scanned: two tiles in flight per wave.  Segments shorter than a tile (256 .. 448 elements)
// would leave lanes idle, so there a wave walks 8 consecutive segments as one SPAN (a multiple of the tile, so every lane of every
// tile has work) and the wave scan is segmented: a lane knows how many lanes of its segment lie in front of it and adds no further
// back, and only the lanes whose segment began in an earlier tile take the carry.  nspan = ceil(m / span); wave w of the grid takes
// the spans w, w + waves, ...  The last vector of the input may hold fewer than 8 elements; that one lane moves its elements singly.
// No LDS beyond what the shuffles use, no workspace, no dependency between workgroups.
//
// Here: the tile, the launch shape, a tile's loads, the segment arithmetic, the scan's operand and operation, and what the strided
// scans are made of (the class rotate, the packed 16-bit operation, the S-class wave scan: trc_fplanes_join_kernel and
// trc_splanes_join_batch_kernel of trc_splanes_batch.inc, where the stride is the item's).  The walk itself -- the
// span / tile advance, the prefetch, the whole / partial vector store -- is written out in both kernels: as one __forceinline__
// function taking the kernels' parts as functors it compiled to slower code (5 - 18 % on the 32- and 64-bit joins, measured:
// profiles/planes/refactor_notes.md), so a change to it is made in both places.
#ifndef TRC_PLANES_SCAN_H
#define TRC_PLANES_SCAN_H
#include "trc_planes_vec.h"

#define TRC_FPLANES_TILE (64 * TRC_PLANES_VEC)      // elements a wave handles per step of the join

// span and grid of a scanning join over m elements: a wave per span, TRC_PLANES_GRID as for the other plane kernels
static unsigned join_grid(size_t m, u32 seg, u32 &span, size_t &nspan)
{
    span = seg < TRC_FPLANES_TILE ? 8 * seg : seg;
    nspan = (m + span - 1) / span;
    const size_t want = (nspan + TRC_PLANES_BLOCK / 64 - 1) / (TRC_PLANES_BLOCK / 64);
    const unsigned cap = planes_grid_cap();
    return want > cap ? cap : (unsigned)want;
}

// the scan's operand of y (bits above a 16-bit element's width are junk from here on; pack drops them) and the scan's operation
template <int ESIZE, int FILTER> __device__ __forceinline__ typename Elem<ESIZE>::T operand(typename Elem<ESIZE>::T y)
{
    typedef typename Elem<ESIZE>::T T;
    if constexpr (FILTER == TRC_FILTER_XOR) return y;
    return (y >> 1) ^ ((T)0 - (y & 1));
}
template <int FILTER, typename T> __device__ __forceinline__ T op(T a, T b) { return FILTER == TRC_FILTER_XOR ? a ^ b : a + b; }

// the bytes of `cnt` elements from `base` on, of every plane: 8 = a whole vector, 0 = none (zeros: the scan's identity)
template <int ESIZE> __device__ __forceinline__ void tile_load(const uint8_t *__restrict__ planes, size_t pitch, size_t base, u32 cnt, uint2 *p)
{
#pragma unroll
    for (int k = 0; k < ESIZE; k++) p[k] = make_uint2(0u, 0u);
    if (cnt == TRC_PLANES_VEC) {
#pragma unroll
        for (int k = 0; k < ESIZE; k++) p[k] = *(const uint2 *)(planes + k * pitch + base);
    } else if (cnt) {                              // the input's last vector
#pragma unroll
        for (int k = 0; k < ESIZE; k++) {
            uint64_t a = 0;
#pragma unroll
            for (int j = 0; j < TRC_PLANES_VEC - 1; j++) if ((u32)j < cnt) a |= (uint64_t)planes[k * pitch + base + j] << (8 * j);
            p[k] = make_uint2((u32)a, (u32)(a >> 32));
        }
    }
}

// x < 3 * seg -> x % seg
__device__ __forceinline__ u32 wrap_seg(u32 x, u32 seg)
{
    if (x >= seg) x -= seg;
    if (x >= seg) x -= seg;
    return x;
}

// out[i] = a[(i + r) % S], r in [0, S): a rotate by 1, by 2 and by 4, each taken where r has that bit -- selects over static
// indices, three per value
template <int S, typename T> __device__ __forceinline__ void rotate(const T *a, u32 r, T *out)
{
    T x[S];
#pragma unroll
    for (int i = 0; i < S; i++) x[i] = a[i];
#pragma unroll
    for (int b = 1; b < S; b <<= 1) {
        const bool take = r & (u32)b;
        T y[S];
#pragma unroll
        for (int i = 0; i < S; i++) y[i] = take ? x[(i + b) % S] : x[i];
#pragma unroll
        for (int i = 0; i < S; i++) x[i] = y[i];
    }
#pragma unroll
    for (int i = 0; i < S; i++) out[i] = x[i];
}

// 16-bit sums two to a word (v_pk_add_u16), so that a wave scan of 16-bit elements moves two classes per shuffle
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
template <int FILTER> __device__ __forceinline__ u32 pkop(u32 a, u32 b)
{
    if constexpr (FILTER == TRC_FILTER_XOR) return a ^ b;
    return __builtin_bit_cast(u32, (us2)(__builtin_bit_cast(us2, a) + __builtin_bit_cast(us2, b)));
}

// N segmented inclusive wave scans (six __shfl_up steps each): inc[c] = the lane's total of value c on entry.  A lane adds what lies
// at most `reach` lanes in front of it.  before[c] = the sum of the lanes in front of this one in its segment, those of earlier
// tiles included where take_carry says the segment began there; carry[c] = the running value where this tile ends.
template <int FILTER, int N, typename V, bool PK> __device__ __forceinline__ void wave_scan(V *inc, V *carry, V *before, u32 reach, bool take_carry)
{
    auto f = [](V a, V b) __attribute__((always_inline)) { if constexpr (PK) return (V)pkop<FILTER>((u32)a, (u32)b); else return op<FILTER>(a, b); };
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int c = 0; c < N; c++) {
            const V o = __shfl_up(inc[c], d);
            if (reach >= d) inc[c] = f(inc[c], o);
        }
    }
#pragma unroll
    for (int c = 0; c < N; c++) {
        const V in_carry = take_carry ? carry[c] : (V)0, b = __shfl_up(inc[c], 1u);
        before[c] = f(in_carry, reach ? b : (V)0);
        carry[c] = __shfl(f(inc[c], in_carry), 63);
    }
}

#endif
