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
#include "trc_planes_vec.h"

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

extern "C" size_t trc_planes_pitch(size_t n, unsigned esize)
{
    if (!esize_ok(esize) || n < esize) return 0;
    return (n / esize + TRC_PAD + 255) & ~(size_t)255;
}

extern "C" int trc_planes_split_dev(const void *d_in, size_t n, unsigned esize, void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    const int rc = planes_args("planes_split", d_in, n, esize, d_planes, pitch, d_tail);
    if (rc) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize);
    static void (*const kernels[3])(const uint8_t *, size_t, u32, uint8_t *, size_t, uint8_t *) = TRC_BY_ESIZE(trc_planes_split_kernel);
    hipLaunchKernelGGL(kernels[esize_row(esize)], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_in, m, t, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_split: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_join_dev(const void *d_planes, size_t pitch, const void *d_tail, size_t n, unsigned esize, void *d_out, void *stream)
{
    const int rc = planes_args("planes_join", d_out, n, esize, d_planes, pitch, d_tail);
    if (rc) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize);
    static void (*const kernels[3])(const uint8_t *, size_t, const uint8_t *, size_t, u32, uint8_t *) = TRC_BY_ESIZE(trc_planes_join_kernel);
    hipLaunchKernelGGL(kernels[esize_row(esize)], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, t, (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_join: %s", hipGetErrorString(e));
}
