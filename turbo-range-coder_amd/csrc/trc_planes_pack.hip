// trc_planes_pack.hip -- the coded buffers of a batch (trc_encode_(f)planes_batch_dev: directories NC entries apart, payload planes
// `pitch` apart with total[k] bytes at each one's start, CDFs at TRC_PLANES_CDF_STRIDE) packed into the inner TRCP container of a
// TRCB container (include/trc_hip.h), compactly, in device memory, with no host round trip.
//
// Where a section starts depends on d_total, which lives on the device.  EVERY workgroup re-derives the esize <= 8 section offsets
// from it: eight loads and a serial sum, cheaper than any dependency between workgroups -- no atomics, no second launch.  The work
// is then 2 * esize REGIONS (plane k's directory, plane k's payload), each cut into tiles of PACK_TILE 16-byte vectors; a workgroup
// takes tiles in a grid-stride loop and finds a tile's region by a search that is uniform across the workgroup.
//
// Alignment.  d_out is 16-byte aligned and sections start on multiples of 8, so a directory's destination is 8-byte aligned and a
// payload's (section + CDF + 32 + 4 * NC) only 4-byte aligned where NC is odd; a directory's source is 4-byte, a payload's 256-byte
// aligned.  A region is copied as a HEAD of up to 12 bytes that brings the destination to a multiple of 16, a BODY of 16-byte
// stores whose loads are 16 bytes at a 4-byte aligned address (both ends of every region are 4-byte aligned, so head and body keep
// the source on a multiple of 4; where the two agree modulo 16 the same instruction is an aligned load), and a TAIL of up to 15
// bytes.  Heads, tails, CDFs, headers and the zero bytes up to every multiple of 8 are workgroup 0's, byte by byte.
// Loads stay inside [src, src + len) of their region and stores inside [dst, dst + len): nothing is read behind d_clen's
// esize * NC entries or a plane's total[k] bytes, nothing is written at or behind d_out + size.
#include "trc_planes_vec.h"
#include "trc_planes_pack.h"

#define PACK_BLOCK 256
#define PACK_UNROLL 4                               // vectors a thread has in flight
#define PACK_TILE (PACK_BLOCK * PACK_UNROLL)        // 16-byte vectors per tile: 16 KiB
#define PACK_NREG 16                                // directory and payload of up to 8 planes

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4))); // 16 bytes at a 4-byte aligned address

struct PackRegion { uint64_t dst, src, len; u32 head, tile0; };      // offsets of the region's first byte from d_out and from d_clen (directories) or
                                                                     // d_payload (payloads): kernel arguments, so that the accesses are global ones; head bytes; its first tile

__device__ __forceinline__ uint64_t pack_up8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }

__global__ __launch_bounds__(PACK_BLOCK)
void trc_planes_pack_kernel(const PackArgs a)
{
    __shared__ PackRegion reg[PACK_NREG];
    __shared__ uint64_t sec[9];                    // section k's offset in the inner container; sec[esize] = the inner container's size
    const u32 tid = threadIdx.x, nreg = 2 * a.esize;

    // the layout, uniform across the workgroup (and the same in every workgroup): planes_host_encode's rules
    uint64_t pos = 32 + 8 * (uint64_t)a.esize;
    u32 tiles = 0;
    bool bad = false;
#pragma unroll
    for (u32 k = 0; k < 8; k++) {
        if (k >= a.esize) continue;
        const uint64_t tot = a.total[k];
        bad |= tot > a.M;
        if (a.status) bad |= a.status[k] < 0;
        const uint64_t dird = a.inner + pos + a.cdfb + 32, dlen = 4 * a.NC;
#pragma unroll
        for (u32 j = 0; j < 2; j++) {
            const uint64_t d = j ? dird + dlen : dird, len = j ? tot : dlen;
            uint64_t head = (0 - d) & 15;          // (a.out is a multiple of 16)
            if (head > len) head = len;
            const uint64_t nvec = (len - head) >> 4;
            if (tid == 0) {
                PackRegion R;
                R.dst = d;
                R.src = j ? k * a.pitch : 4 * k * a.NC;
                R.len = len; R.head = (u32)head; R.tile0 = tiles;
                reg[2 * k + j] = R;
            }
            tiles += (u32)((nvec + PACK_TILE - 1) / PACK_TILE);
        }
        if (tid == 0) sec[k] = pos;
        pos = pack_up8(pos + a.cdfb + 32 + dlen + tot);
    }
    if (bad) {                                     // a CDF that could not be built, or a total no encoder writes: no container
        if (blockIdx.x == 0 && tid == 0) *a.d_size = 0;
        return;
    }
    if (tid == 0) sec[a.esize] = pos;
    __syncthreads();

    // the bodies
    for (u32 t = blockIdx.x; t < tiles; t += gridDim.x) {
        u32 r = 0;
#pragma unroll
        for (u32 j = 1; j < PACK_NREG; j++) if (j < nreg && t >= reg[j].tile0) r = j;
        const PackRegion R = reg[r];
        const uint64_t nvec = (R.len - R.head) >> 4;
        const uint8_t *src = (r & 1 ? a.payload : (const uint8_t *)a.clen) + R.src + R.head;
        uint8_t *dst = a.out + R.dst + R.head;
        const uint64_t v0 = (uint64_t)(t - R.tile0) * PACK_TILE + tid;
        u32x4 x[PACK_UNROLL];
#pragma unroll
        for (u32 u = 0; u < PACK_UNROLL; u++) {
            const uint64_t i = v0 + u * PACK_BLOCK;
            if (i < nvec) x[u] = *(const u32x4_a4 *)(src + 16 * i);
        }
#pragma unroll
        for (u32 u = 0; u < PACK_UNROLL; u++) {
            const uint64_t i = v0 + u * PACK_BLOCK;
            if (i < nvec) *(u32x4 *)(dst + 16 * i) = x[u];
        }
    }
    if (blockIdx.x) return;

    // everything small: headers, the offset table, sizes, heads and tails, CDFs, the zero bytes up to a multiple of 8
    uint8_t *in = a.out + a.inner;
    if (tid < a.esize) {
        uint64_t *h = (uint64_t *)(in + sec[tid] + a.cdfb);
        h[0] = a.sh[0]; h[1] = a.sh[1]; h[2] = a.sh[2]; h[3] = a.total[tid];
        ((uint64_t *)(in + 32))[tid] = sec[tid];
    }
    if (tid == 64) {
        const uint64_t isz = sec[a.esize];
        uint64_t *h = (uint64_t *)in;
        h[0] = a.ph[0]; h[1] = a.ph[1]; h[2] = a.ph[2]; h[3] = isz;
        ((uint64_t *)a.out)[4] = a.inner + isz;    // trc_planes_batch_hdr.size
        *a.d_size = a.inner + isz;
    }
    for (u32 r = 0; r < nreg; r++) {
        const PackRegion R = reg[r];
        const uint64_t body = ((R.len - R.head) >> 4) << 4;
        const u32 tail = (u32)(R.len - R.head - body);
        const uint8_t *src = (r & 1 ? a.payload : (const uint8_t *)a.clen) + R.src;
        uint8_t *dst = a.out + R.dst;
        if (tid < R.head) dst[tid] = src[tid];
        else if (tid - R.head < tail) { const uint64_t i = R.head + body + (tid - R.head); dst[i] = src[i]; }
    }
    for (u32 k = 0; k < a.esize; k++) {
        uint8_t *s = in + sec[k];
        const uint8_t *cdf = (const uint8_t *)(a.cdf + k * TRC_PLANES_CDF_STRIDE);
        for (u32 i = tid; i < a.cdfb; i += PACK_BLOCK) s[i] = i < a.cdf_used ? cdf[i] : (uint8_t)0;
        const uint64_t end = sec[k] + a.cdfb + 32 + 4 * a.NC + a.total[k];
        if (tid < sec[k + 1] - end) in[end + tid] = 0;
    }
}

int trc_planes_pack_launch(const PackArgs &a, hipStream_t s)
{
    // the tiles the regions have at most: the grid cannot wait for d_total
    const size_t dir = (a.NC / 4 + PACK_TILE - 1) / PACK_TILE, pay = (a.M / 16 + PACK_TILE - 1) / PACK_TILE;
    const size_t want = a.esize * (dir + pay);
    const unsigned cap = planes_grid_cap();
    const dim3 grid(want < 1 ? 1u : want > cap ? cap : (unsigned)want), block(PACK_BLOCK);
    hipLaunchKernelGGL(trc_planes_pack_kernel, grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_batch_pack: %s", hipGetErrorString(e));
}
