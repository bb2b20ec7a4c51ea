// trc_planes_scan.h -- the scanning join of the filtered byte planes: what it is, and the pieces that trc_fplanes_join_kernel
// (trc_fplanes.hip: one buffer, every stride) and trc_fplanes_join_batch_kernel (trc_fplanes_batch.inc: the items of a batch, a filter
// per item) share.
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
// Here: the tile, the launch shape, a tile's loads, the segment arithmetic, the scan's operand and operation.  The walk itself -- the
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

#endif
