// trc_fp.h -- the terms of a base's fingerprint, for the two files that sum them: trc_bplanes.hip (one buffer) and trc_fp_batch.inc
// (a base per item of a batch).  fp = sum_j (2j + 1) * w_j + nbytes * TRC_FP_LEN_MUL mod 2^64 over the little-endian u64 words w_j
// of the nbytes bytes, zero-padded to 8: a wrapping sum, so every order of addition gives the same value.
#pragma once

#define TRC_FP_LEN_MUL 0x9E3779B97F4A7C15ull
// the terms of words 2i and 2i + 1, the 16-byte pair x
__device__ __forceinline__ uint64_t fp_pair(size_t i, uint4 x)
{
    return (4 * (uint64_t)i + 1) * ((uint64_t)x.x | (uint64_t)x.y << 32) + (4 * (uint64_t)i + 3) * ((uint64_t)x.z | (uint64_t)x.w << 32);
}
// the terms one lane adds: the bytes behind the last whole pair (at most 15, read one by one: nothing at or behind p + nbytes is
// touched) and the length term
__device__ inline uint64_t fp_rest(const uint8_t *p, size_t nbytes)
{
    uint64_t sum = (uint64_t)nbytes * TRC_FP_LEN_MUL;
    for (size_t j = nbytes / 16 * 2; j * 8 < nbytes; j++) {
        uint64_t w = 0;
        for (uint32_t b = 0; b < 8 && j * 8 + b < nbytes; b++) w |= (uint64_t)p[j * 8 + b] << (8 * b);
        sum += (2 * (uint64_t)j + 1) * w;
    }
    return sum;
}
