// trc_tree.h -- the mb8enc tree nodes in the TRC_RCC1 block layout, shared by the bitwise coders that keep trees in the
// workspace (trc_rc_o1bit.hip, trc_rc_word.hip): a block is 16 u16 (32 B) read as eight packed dwords, slot j = node j.
#pragma once
#include "trc_dev.h"

// u16 slot j (0..15) of eight packed dwords
__device__ __forceinline__ u32 o1b_pick(const u32 (&q)[8], u32 j)
{
    u32 r = q[0];
#pragma unroll
    for (u32 i = 1; i < 8; i++) r = (j >> 1) == i ? q[i] : r;
    return (j & 1u) ? r >> 16 : r & 0xffffu;
}
