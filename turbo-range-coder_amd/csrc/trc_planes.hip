// trc_planes.hip -- byte planes of 16 / 32 / 64-bit elements: split (element order -> plane k = byte k of every element) and join.
//
// Layout (include/trc_hip.h): n bytes = m elements of `esize` bytes + t tail bytes; plane k is the m bytes in[i * esize + k], planes
// lie `pitch` bytes apart, the tail bytes go to a buffer of their own.  This is the plain definition, the scalar loop of the
// reference's tpenc (transpose_.c:115-121); DESIGN.md says why its SIMD layouts are not reproduced.
//
// Both kernels move n bytes in and n bytes out and nothing else: no LDS, the bytes change places in registers.  A thread owns a
// VECTOR of 8 consecutive elements: it loads them as esize / 2 aligned 16-byte words (1, 2 or 4 loads, all issued before the first
// use), separates the bytes with v_perm_b32 and stores 8 contiguous bytes to each plane, so one store instruction of a wave
// covers 512 contiguous bytes of a plane (two whole 256-byte runs) and one load instruction 1 KiB of the input.  Join is the mirror
// image: esize 8-byte loads, esize / 2 16-byte stores.  Eight elements per thread for every size keeps every plane access at
// 8 bytes and the three sizes on one code path.  The m % 8 elements behind the last whole vector and the t tail bytes are moved
// one byte per lane by the first lanes of workgroup 0.
//
// Launch: 256 threads, a grid-stride loop over the vectors, at most TRC_PLANES_GRID_MAX workgroups = 8 per CU on 256 CUs
// (32 waves per CU when the input is large enough; the kernels use no LDS and few registers, so they all fit).
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

// in: 16-byte aligned, m * ESIZE + t bytes.  planes: 256-byte aligned, pitch a multiple of 256.  Writes [0, m) of every plane and
// [0, t) of tail, nothing else.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_split_kernel(const uint8_t *__restrict__ in, size_t m, u32 t, uint8_t *__restrict__ planes, size_t pitch, uint8_t *__restrict__ tail)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;     // words and 16-byte words of a vector
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
        u32 w[NW];
#pragma unroll
        for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
        uint2 p[ESIZE];
        vec_split<ESIZE>(w, p);
#pragma unroll
        for (int k = 0; k < ESIZE; k++) *(uint2 *)(planes + k * pitch + v * TRC_PLANES_VEC) = p[k];
    }
    // the elements behind the last whole vector (at most 7) and the tail bytes (at most ESIZE - 1): a byte per lane
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC) * ESIZE, g = threadIdx.x;
        const size_t b0 = nv * (TRC_PLANES_VEC * ESIZE);
        if (g < rest) planes[(g % ESIZE) * pitch + nv * TRC_PLANES_VEC + g / ESIZE] = in[b0 + g];
        else if (g < rest + t) tail[g - rest] = in[b0 + g];
    }
}

// the mirror image: writes [0, m * ESIZE + t) of out, nothing else
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_join_kernel(const uint8_t *__restrict__ planes, size_t pitch, const uint8_t *__restrict__ tail, size_t m, u32 t, uint8_t *__restrict__ out)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        uint2 p[ESIZE];
#pragma unroll
        for (int k = 0; k < ESIZE; k++) p[k] = *(const uint2 *)(planes + k * pitch + v * TRC_PLANES_VEC);
        u32 w[NW];
        vec_join<ESIZE>(p, w);
        uint4 *dst = (uint4 *)(out + v * (TRC_PLANES_VEC * ESIZE));
#pragma unroll
        for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC) * ESIZE, g = threadIdx.x;
        const size_t b0 = nv * (TRC_PLANES_VEC * ESIZE);
        if (g < rest) out[b0 + g] = planes[(g % ESIZE) * pitch + nv * TRC_PLANES_VEC + g / ESIZE];
        else if (g < rest + t) out[b0 + g] = tail[g - rest];
    }
}

// workgroups of a launch over m elements; TRC_PLANES_GRID in the environment lowers the cap (tuning aid, and how the tests make
// a small input take the grid-stride loop more than once)
static unsigned planes_grid(size_t m)
{
    const size_t nv = m / TRC_PLANES_VEC, want = (nv + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK;
    unsigned cap = TRC_PLANES_GRID_MAX;
    const char *e = getenv("TRC_PLANES_GRID");
    if (e) { const long v = strtol(e, 0, 10); if (v >= 1 && v < (long)TRC_PLANES_GRID_MAX) cap = (unsigned)v; }
    return want < 1 ? 1u : want > cap ? cap : (unsigned)want;
}

static bool esize_ok(unsigned esize) { return esize == 2 || esize == 4 || esize == 8; }

extern "C" size_t trc_planes_pitch(size_t n, unsigned esize)
{
    if (!esize_ok(esize) || n < esize) return 0;
    return (n / esize + TRC_PAD + 255) & ~(size_t)255;
}

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

extern "C" int trc_planes_split_dev(const void *d_in, size_t n, unsigned esize, void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    const int rc = planes_args("planes_split", d_in, n, esize, d_planes, pitch, d_tail);
    if (rc) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize);
    const dim3 grid(planes_grid(m)), block(TRC_PLANES_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    if (esize == 2) hipLaunchKernelGGL(trc_planes_split_kernel<2>, grid, block, 0, s, (const uint8_t *)d_in, m, t, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    else if (esize == 4) hipLaunchKernelGGL(trc_planes_split_kernel<4>, grid, block, 0, s, (const uint8_t *)d_in, m, t, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    else hipLaunchKernelGGL(trc_planes_split_kernel<8>, grid, block, 0, s, (const uint8_t *)d_in, m, t, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_split: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_join_dev(const void *d_planes, size_t pitch, const void *d_tail, size_t n, unsigned esize, void *d_out, void *stream)
{
    const int rc = planes_args("planes_join", d_out, n, esize, d_planes, pitch, d_tail);
    if (rc) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize);
    const dim3 grid(planes_grid(m)), block(TRC_PLANES_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    if (esize == 2) hipLaunchKernelGGL(trc_planes_join_kernel<2>, grid, block, 0, s, (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, t, (uint8_t *)d_out);
    else if (esize == 4) hipLaunchKernelGGL(trc_planes_join_kernel<4>, grid, block, 0, s, (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, t, (uint8_t *)d_out);
    else hipLaunchKernelGGL(trc_planes_join_kernel<8>, grid, block, 0, s, (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, t, (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_join: %s", hipGetErrorString(e));
}
