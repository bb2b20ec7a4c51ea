// trc_fplanes.hip -- the byte-plane split and join of trc_planes.hip with a predictor filter in front of the planes: zigzag delta
// (TRC_FILTER_ZDELTA) or xor (TRC_FILTER_XOR) against the previous element, restarted every `seg` elements.
//
// Definition (include/trc_hip.h): x[i] = the m little-endian elements of w = 8 * esize bits, p[i] = 0 where i % seg == 0, else
// x[i - 1];  y[i] = zigzag(x[i] - p[i] mod 2^w)  or  x[i] ^ p[i];  plane k = byte k of every y[i].  The tail bytes are not filtered.
//
// Split is the unfiltered kernel plus one element load: a thread owns a vector of 8 elements, seg is a multiple of 64, so a vector
// never straddles a restart and the only element a thread lacks is the one in front of its vector (a line its neighbour loads
// anyway).  Whether a vector opens a segment is kept as v % (seg / 8) in 32 bits and stepped with the grid-stride loop.
//
// Join undoes a prefix sum (or prefix xor) that restarts every seg elements.  One WAVE walks one segment in tiles of 512 elements,
// 8 per lane: join the planes' bytes to elements, undo the zigzag, scan the lane's 8 serially, scan the 64 lane totals across the
// wave (six __shfl_up steps), add the value carried out of the previous tile and store 16-byte words.  A tile's loads do not depend
// on the carry, so the loads of the wave's NEXT tile -- of the same segment or of the wave's next segment -- are issued before the
// current tile is scanned: two tiles in flight per wave.  Segments shorter than a tile (256 .. 448 elements) would leave lanes idle,
// so there a wave walks 8 consecutive segments as one span and the wave scan is segmented: a lane knows how many lanes of its
// segment lie in front of it and adds no further back.  The last vector of the input may hold fewer than 8 elements; that one
// lane moves its elements singly.  No LDS beyond what the shuffles use, no workspace.
#include "trc_planes_vec.h"

#define TRC_FPLANES_TILE (64 * TRC_PLANES_VEC)      // elements a wave handles per step of the join

// the scan's operand of y (bits above a 16-bit element's width are junk from here on; pack drops them) and the scan's operation
template <int ESIZE, int FILTER> __device__ __forceinline__ typename Elem<ESIZE>::T operand(typename Elem<ESIZE>::T y)
{
    typedef typename Elem<ESIZE>::T T;
    if constexpr (FILTER == TRC_FILTER_XOR) return y;
    return (y >> 1) ^ ((T)0 - (y & 1));
}
template <int FILTER, typename T> __device__ __forceinline__ T op(T a, T b) { return FILTER == TRC_FILTER_XOR ? a ^ b : a + b; }

// in: 16-byte aligned, m * ESIZE + t bytes.  planes: 256-byte aligned, pitch a multiple of 256.  seg: a multiple of 64.  r0 =
// (m / 8 * 8) % seg, where the elements behind the last whole vector lie in their segment.  Writes [0, m) of every plane and
// [0, t) of tail, nothing else.
template <int ESIZE, int FILTER> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_split_kernel(const uint8_t *__restrict__ in, size_t m, u32 t, u32 seg, u32 r0, uint8_t *__restrict__ planes, size_t pitch, uint8_t *__restrict__ tail)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    const M *el = (const M *)in;
    const u32 vseg = seg / TRC_PLANES_VEC, v0 = blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x, rstep = (u32)step % vseg;
    u32 r = v0 % vseg;                             // the vector's place in its segment: 0 opens one
    for (size_t v = v0; v < nv; v += step) {
        const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
        u32 w[NW];
#pragma unroll
        for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
        T prev = 0;
        if (r) prev = el[v * TRC_PLANES_VEC - 1];
        T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, FILTER>(e[j], j ? e[j - 1] : prev);
        pack<ESIZE>(y, w);
        uint2 p[ESIZE];
        vec_split<ESIZE>(w, p);
#pragma unroll
        for (int k = 0; k < ESIZE; k++) *(uint2 *)(planes + k * pitch + v * TRC_PLANES_VEC) = p[k];
        r += rstep;
        if (r >= vseg) r -= vseg;
    }
    // the elements behind the last whole vector (at most 7), one per lane, and the tail bytes (at most ESIZE - 1)
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC), g = threadIdx.x;
        if (g < rest) {
            const size_t i = nv * TRC_PLANES_VEC + g;
            const T y = fwd<ESIZE, FILTER>((T)el[i], r0 + g ? (T)el[i - 1] : (T)0);
#pragma unroll
            for (int k = 0; k < ESIZE; k++) planes[k * pitch + i] = (uint8_t)(y >> (8 * k));
        } else if (g < rest + t) tail[g - rest] = in[m * ESIZE + (g - rest)];
    }
}

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

// the mirror image: writes [0, m * ESIZE + t) of out, nothing else.  A SPAN is what a wave walks in one go: a segment, or, where
// segments are shorter than a tile, 8 of them (a multiple of the tile, so every lane of every tile has work); nspan = ceil(m / span),
// wave w of the grid takes the spans w, w + waves, ...  The wave scan is segmented: a lane adds what lies at most `lanes in front of
// it within its segment` away, and only the lanes whose segment began in an earlier tile take the carry.
template <int ESIZE, int FILTER> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_join_kernel(const uint8_t *__restrict__ planes, size_t pitch, const uint8_t *__restrict__ tail, size_t m, u32 t, u32 seg, u32 span,
                             size_t nspan, uint8_t *__restrict__ out)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const u32 lane = threadIdx.x & 63u;
    const size_t waves = (size_t)gridDim.x * (TRC_PLANES_BLOCK / 64);
    size_t s = (size_t)blockIdx.x * (TRC_PLANES_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // the span, the tile in it,
    u32 tile = 0;                                                                                                   // the span's length: one per wave
    if (s < nspan) {
        u32 len = (u32)(m - s * span < span ? m - s * span : span);
        u32 at = lane * TRC_PLANES_VEC;                                  // the lane's first element in the span ...
        u32 nin = wrap_seg(at, seg);                                     // ... and in its segment (span <= 8 * seg, a tile < 3 * seg)
        u32 ncnt = at < len ? (len - at < TRC_PLANES_VEC ? len - at : TRC_PLANES_VEC) : 0;
        size_t nbase = s * span + at;
        uint2 pn[ESIZE];
        tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
        T carry = 0;
        for (;;) {
            uint2 p[ESIZE];
#pragma unroll
            for (int k = 0; k < ESIZE; k++) p[k] = pn[k];
            const size_t base = nbase;
            const u32 cnt = ncnt, ahead = nin / TRC_PLANES_VEC;          // lanes' worth of elements in front of this one in its segment
            // the wave's next tile: its loads are under way while this one is scanned
            tile++;
            bool more = true;
            if (tile * TRC_FPLANES_TILE >= len) {
                s += waves; tile = 0;
                more = s < nspan;
                if (more) len = (u32)(m - s * span < span ? m - s * span : span);
                nin = wrap_seg(lane * TRC_PLANES_VEC, seg);
            } else nin = wrap_seg(nin + TRC_FPLANES_TILE, seg);
            if (more) {
                at = tile * TRC_FPLANES_TILE + lane * TRC_PLANES_VEC;
                ncnt = at < len ? (len - at < TRC_PLANES_VEC ? len - at : TRC_PLANES_VEC) : 0;
                nbase = s * span + at;
                tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
            }
            u32 w[NW];
            vec_join<ESIZE>(p, w);
            T e[TRC_PLANES_VEC];
            unpack<ESIZE>(w, e);
            e[0] = operand<ESIZE, FILTER>(e[0]);
#pragma unroll
            for (int j = 1; j < TRC_PLANES_VEC; j++) e[j] = op<FILTER>(e[j - 1], operand<ESIZE, FILTER>(e[j]));
            const u32 reach = ahead < lane ? ahead : lane;               // ... of them in this tile
            T inc = e[TRC_PLANES_VEC - 1];                               // the lane's total -> the totals of its segment's lanes up to it
#pragma unroll
            for (u32 d = 1; d < 64; d <<= 1) {
                const T o = __shfl_up(inc, d);
                if (reach >= d) inc = op<FILTER>(inc, o);
            }
            T before = __shfl_up(inc, 1u);                               // ... of the lanes in front of it, and of the earlier tiles
            before = op<FILTER>(ahead > lane ? carry : (T)0, reach ? before : (T)0);
#pragma unroll
            for (int j = 0; j < TRC_PLANES_VEC; j++) e[j] = op<FILTER>(e[j], before);
            carry = __shfl(e[TRC_PLANES_VEC - 1], 63);                   // the tile's last element: the predecessor the next tile starts from
            if (cnt == TRC_PLANES_VEC) {
                pack<ESIZE>(e, w);
                uint4 *dst = (uint4 *)(out + base * ESIZE);
#pragma unroll
                for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
            } else if (cnt) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC - 1; j++) if ((u32)j < cnt) ((M *)out)[base + j] = (M)e[j];
            }
            if (!more) break;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < t) out[m * ESIZE + threadIdx.x] = tail[threadIdx.x];
}

static int filter_args(const char *who, int filter, uint32_t seg)
{
    if (filter != TRC_FILTER_NONE && filter != TRC_FILTER_ZDELTA && filter != TRC_FILTER_XOR)
        return trc_fail(TRC_E_ARG, "%s: filter %d (0 none, 1 zigzag delta, 2 xor)", who, filter);
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "%s: restart length %u: must be a multiple of 64 in [%u,%u]", who, seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    return TRC_OK;
}

#define FPLANES_LAUNCH(kernel, grid, ...) do { \
        const dim3 g_(grid), b_(TRC_PLANES_BLOCK); \
        if (filter == TRC_FILTER_ZDELTA) { \
            if (esize == 2) hipLaunchKernelGGL((kernel<2, TRC_FILTER_ZDELTA>), g_, b_, 0, s, __VA_ARGS__); \
            else if (esize == 4) hipLaunchKernelGGL((kernel<4, TRC_FILTER_ZDELTA>), g_, b_, 0, s, __VA_ARGS__); \
            else hipLaunchKernelGGL((kernel<8, TRC_FILTER_ZDELTA>), g_, b_, 0, s, __VA_ARGS__); \
        } else { \
            if (esize == 2) hipLaunchKernelGGL((kernel<2, TRC_FILTER_XOR>), g_, b_, 0, s, __VA_ARGS__); \
            else if (esize == 4) hipLaunchKernelGGL((kernel<4, TRC_FILTER_XOR>), g_, b_, 0, s, __VA_ARGS__); \
            else hipLaunchKernelGGL((kernel<8, TRC_FILTER_XOR>), g_, b_, 0, s, __VA_ARGS__); \
        } } while (0)

extern "C" int trc_planes_split_filter_dev(int filter, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                           void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    int rc = filter_args("planes_split_filter", filter, seg);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_split_dev(d_in, n, esize, d_planes, pitch, d_tail, stream);
    if ((rc = planes_args("planes_split_filter", d_in, n, esize, d_planes, pitch, d_tail))) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize), r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    hipStream_t s = (hipStream_t)stream;
    FPLANES_LAUNCH(trc_fplanes_split_kernel, planes_grid(m), (const uint8_t *)d_in, m, t, seg, r0, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_split_filter: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_join_filter_dev(int filter, const void *d_planes, size_t pitch, const void *d_tail,
                                          size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream)
{
    int rc = filter_args("planes_join_filter", filter, seg);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_join_dev(d_planes, pitch, d_tail, n, esize, d_out, stream);
    if ((rc = planes_args("planes_join_filter", d_out, n, esize, d_planes, pitch, d_tail))) return rc;
    const uint32_t t = (uint32_t)(n % esize), span = seg < TRC_FPLANES_TILE ? 8 * seg : seg;
    const size_t m = n / esize, nspan = (m + span - 1) / span;
    // a wave per span, TRC_PLANES_GRID as for the other plane kernels
    const size_t want = (nspan + TRC_PLANES_BLOCK / 64 - 1) / (TRC_PLANES_BLOCK / 64);
    const unsigned cap = planes_grid_cap(), grid = want > cap ? cap : (unsigned)want;
    hipStream_t s = (hipStream_t)stream;
    FPLANES_LAUNCH(trc_fplanes_join_kernel, grid, (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, t, seg, span, nspan, (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_join_filter: %s", hipGetErrorString(e));
}
