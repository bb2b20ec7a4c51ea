// trc_planes_count.h -- what the two histogram kernels of the planes advisor share (trc_planes_hist.hip: one buffer;
// trc_planes_hist_batch.inc: the items of a batch): the shape of a workgroup's LDS counters and the adds into them.  The layout
// [row][bin][copy] and why it is what it is: trc_planes_hist.hip.
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

#endif
