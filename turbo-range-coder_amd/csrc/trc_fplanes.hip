// trc_fplanes.hip -- the byte-plane split and join of trc_planes.hip with a predictor filter in front of the planes: zigzag delta
// (TRC_FILTER_ZDELTA) or xor (TRC_FILTER_XOR) against the element S back, restarted every `seg` elements.  S = 1 is the plain
// predecessor; S = 2 .. 8 (TRC_STRIDE_MAX) is for data that interleaves S series of one element width (rows of S fields, stereo /
// 5.1 / 7.1 PCM, xyz(w) points, complex pairs, RGB(A)16).  One kernel per (esize, filter, stride) and direction.
//
// Definition (include/trc_hip.h): x[i] = the m little-endian elements of w = 8 * esize bits, p[i] = 0 where i % seg < S, else
// x[i - S];  y[i] = zigzag(x[i] - p[i] mod 2^w)  or  x[i] ^ p[i];  plane k = byte k of every y[i].  The tail bytes are not filtered.
//
// Split is the unfiltered kernel with a reach backwards: a thread owns a vector of 8 elements, seg is a multiple of 64, so a vector
// never straddles a restart, and with S <= 8 the only elements it lacks are the last S of the vector in front of it (a line its
// neighbour loads anyway).  At S = 1 it loads that one element, else the 16-byte words that hold them; a vector that opens a segment
// loads nothing and predicts zero for its first S elements.  Whether a vector opens a segment is kept as v % (seg / 8) in 32 bits
// and stepped with the grid-stride loop.  S is a template argument, so every index is static.
//
// Join undoes S interleaved prefix sums (or prefix xors) that restart every seg elements.  The walk -- a wave per span, tiles of 512
// elements, the next tile's loads in flight -- is explained in trc_planes_scan.h, which has its pieces; what changes with S is the scan.
// An element's CLASS is its position in the segment mod S; the S classes are S independent scans.  At S = 1 that is: scan the lane's
// 8 serially, scan the 64 lane totals across the wave, add the carry of lane 63 out of the previous tile.  At S > 1:
//   - in the lane: e[j] = op(e[j], e[j - S]) for j >= S, so the lane's last S elements are its per-class totals;
//   - which class the lane's element j has depends on where the lane stands in its segment: (nin + j) % S.  The totals are brought
//     into class order by a rotate -- none where S divides 8 (nin is a multiple of 8), a chain of selects on nin % S otherwise; no
//     register array is indexed dynamically;
//   - S segmented wave scans (six __shfl_up steps each), plus the carry of S values out of the previous tile for the lanes whose
//     segment began in an earlier tile; the carry is kept in class order, so it needs no rotate.  16-bit elements go two classes
//     to a word through the scans (v_pk_add_u16 / xor): the shuffles are what the scan costs, and this halves them;
//   - the sums of the lanes in front are rotated back to the lane's element order and added per element.
#include "trc_planes_scan.h"

// in: 16-byte aligned, m * ESIZE + t bytes.  planes: 256-byte aligned, pitch a multiple of 256.  seg: a multiple of 64.  r0 =
// (m / 8 * 8) % seg, where the elements behind the last whole vector lie in their segment.  Writes [0, m) of every plane and
// [0, t) of tail, nothing else; reads nothing in front of `in`.
template <int ESIZE, int FILTER, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_split_kernel(const uint8_t *__restrict__ in, size_t m, u32 t, u32 seg, u32 r0, uint8_t *__restrict__ planes, size_t pitch, uint8_t *__restrict__ tail)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE;
    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    const M *el = (const M *)in;
    const u32 vseg = seg / TRC_PLANES_VEC, v0 = blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x, rstep = (u32)step % vseg;
    u32 r = v0 % vseg;                             // the vector's place in its segment: 0 opens one
    for (size_t v = v0; v < nv; v += step) {
        const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
        u32 w[NW];
#pragma unroll
        for (int q = 0; q < NW / 4; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
        T pe[TRC_PLANES_VEC];
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) pe[j] = 0;
        if (r) {
            if constexpr (S == 1) pe[TRC_PLANES_VEC - 1] = el[v * TRC_PLANES_VEC - 1];
            else load_front<ESIZE, S>(in, v, pe);
        }
        T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, FILTER>(e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
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
            const T y = fwd<ESIZE, FILTER>((T)el[i], r0 + g >= (u32)S ? (T)el[i - S] : (T)0);      // (r0 + g >= S: i >= S)
#pragma unroll
            for (int k = 0; k < ESIZE; k++) planes[k * pitch + i] = (uint8_t)(y >> (8 * k));
        } else if (g < rest + t) tail[g - rest] = in[m * ESIZE + (g - rest)];
    }
}

// the mirror image of the split: writes [0, m * ESIZE + t) of out, nothing else.  span, nspan: join_grid (trc_planes_scan.h, which
// also says how the walk goes and why).  carry[c] = the running value of class c at the end of the previous tile.  The walk is the
// one trc_fplanes_join_batch_kernel has; it stands in both kernels as text, not as a shared function: profiles/planes/refactor_notes.md.
template <int ESIZE, int FILTER, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_join_kernel(const uint8_t *__restrict__ planes, size_t pitch, const uint8_t *__restrict__ tail, size_t m, u32 t, u32 seg, u32 span,
                             size_t nspan, uint8_t *__restrict__ out)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4, V = TRC_PLANES_VEC;
    constexpr bool ROT = (V % S) != 0;                                   // S divides 8: a lane's element j has class j % S
    constexpr int NP = ESIZE == 2 ? (S + 1) / 2 : S;                     // values the wave scans (16-bit elements: two classes to a word, T is u32)
    const u32 lane = threadIdx.x & 63u;
    const size_t waves = (size_t)gridDim.x * (TRC_PLANES_BLOCK / 64);
    size_t s = (size_t)blockIdx.x * (TRC_PLANES_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // the span, the tile in it,
    u32 tile = 0;                                                                                                   // the span's length: one per wave
    if (s < nspan) {
        u32 len = (u32)(m - s * span < span ? m - s * span : span);
        u32 at = lane * V;                                               // the lane's first element in the span ...
        u32 nin = wrap_seg(at, seg);                                     // ... and in its segment (span <= 8 * seg, a tile < 3 * seg)
        u32 ncnt = at < len ? (len - at < V ? len - at : V) : 0;
        size_t nbase = s * span + at;
        uint2 pn[ESIZE];
        tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
        T carry[NP];
        if constexpr (S == 1) carry[0] = 0;                              // (not the loop: even one turn of it in front of the walk reorders
        else {                                                           // the walk's entries for the compiler; 16- and 32-bit stride-1 joins
                                                                         // then come out 22 instructions longer and 6 - 9 % slower at seg 65536)
#pragma unroll
            for (int c = 0; c < NP; c++) carry[c] = 0;
        }
        for (;;) {
            uint2 p[ESIZE];
#pragma unroll
            for (int k = 0; k < ESIZE; k++) p[k] = pn[k];
            const size_t base = nbase;
            const u32 cnt = ncnt, ahead = nin / V;                       // lanes' worth of elements in front of this one in its segment
            const u32 r8 = ROT ? nin % (u32)S : 0u;                      // the class of the lane's first element
            // the wave's next tile: its loads are under way while this one is scanned
            tile++;
            bool more = true;
            if (tile * TRC_FPLANES_TILE >= len) {
                s += waves; tile = 0;
                more = s < nspan;
                if (more) len = (u32)(m - s * span < span ? m - s * span : span);
                nin = wrap_seg(lane * V, seg);
            } else nin = wrap_seg(nin + TRC_FPLANES_TILE, seg);
            if (more) {
                at = tile * TRC_FPLANES_TILE + lane * V;
                ncnt = at < len ? (len - at < V ? len - at : V) : 0;
                nbase = s * span + at;
                tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
            }
            u32 w[NW];
            vec_join<ESIZE>(p, w);
            T e[V];
            unpack<ESIZE>(w, e);
            if constexpr (S == 1) {                                      // one class: the lane's 8 serially, one wave scan, the carry of lane 63
                e[0] = operand<ESIZE, FILTER>(e[0]);
#pragma unroll
                for (int j = 1; j < V; j++) e[j] = op<FILTER>(e[j - 1], operand<ESIZE, FILTER>(e[j]));
                const u32 reach = ahead < lane ? ahead : lane;           // lanes in front of this one in its segment and in this tile
                T inc = e[V - 1];                                        // the lane's total -> the totals of its segment's lanes up to it
#pragma unroll
                for (u32 d = 1; d < 64; d <<= 1) {
                    const T o = __shfl_up(inc, d);
                    if (reach >= d) inc = op<FILTER>(inc, o);
                }
                T before = __shfl_up(inc, 1u);                           // ... of the lanes in front of it, and of the earlier tiles
                before = op<FILTER>(ahead > lane ? carry[0] : (T)0, reach ? before : (T)0);
#pragma unroll
                for (int j = 0; j < V; j++) e[j] = op<FILTER>(e[j], before);
                carry[0] = __shfl(e[V - 1], 63);                         // the tile's last element: the predecessor the next tile starts from
            } else {
#pragma unroll
                for (int j = 0; j < V; j++) e[j] = operand<ESIZE, FILTER>(e[j]);
#pragma unroll
                for (int j = S; j < V; j++) e[j] = op<FILTER>(e[j], e[j - S]);
                // the lane's totals by class: element 8 - S + i has class (r8 + 8 + i) % S
                T inc[S];
                if constexpr (ROT) {
                    const u32 rot = (r8 + V) % (u32)S;
                    rotate<S>(e + V - S, rot ? (u32)S - rot : 0u, inc);
                } else {
#pragma unroll
                    for (int c = 0; c < S; c++) inc[c] = e[V - S + c];
                }
                const u32 reach = ahead < lane ? ahead : lane;           // lanes in front of this one in its segment and in this tile
                T before[S];                                             // per class: the lanes in front of it, and the earlier tiles
                if constexpr (ESIZE == 2) {                              // two classes to a word: half the shuffles
                    u32 pk[NP], pb[NP];
#pragma unroll
                    for (int i = 0; i < NP; i++) {
                        constexpr int LAST = S - 1;
                        const int hi = 2 * i + 1 < S ? 2 * i + 1 : LAST; // (an odd S: the last word holds one class)
                        pk[i] = (inc[2 * i] & 0xffffu) | (2 * i + 1 < S ? inc[hi] << 16 : 0u);
                    }
                    wave_scan<FILTER, NP, u32, true>(pk, carry, pb, reach, ahead > lane);
#pragma unroll
                    for (int c = 0; c < S; c++) before[c] = c & 1 ? pb[c / 2] >> 16 : pb[c / 2];       // (junk above bit 15, as everywhere)
                } else wave_scan<FILTER, S, T, false>(inc, carry, before, reach, ahead > lane);
                if constexpr (ROT) {
                    T loc[S];
                    rotate<S>(before, r8, loc);                          // loc[i] = before[(r8 + i) % S]: element j takes loc[j % S]
#pragma unroll
                    for (int j = 0; j < V; j++) e[j] = op<FILTER>(e[j], loc[j % S]);
                } else {
#pragma unroll
                    for (int j = 0; j < V; j++) e[j] = op<FILTER>(e[j], before[j % S]);
                }
            }
            if (cnt == V) {
                pack<ESIZE>(e, w);
                uint4 *dst = (uint4 *)(out + base * ESIZE);
#pragma unroll
                for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
            } else if (cnt) {
#pragma unroll
                for (int j = 0; j < V - 1; j++) if ((u32)j < cnt) ((M *)out)[base + j] = (M)e[j];
            }
            if (!more) break;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < t) out[m * ESIZE + threadIdx.x] = tail[threadIdx.x];
}

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
// the filter id alone (also for the coded calls of trc_planes.inc, which vet the restart length with the chunk)
int trc_planes_filter_arg(const char *who, int filter)
{
    if (filter != TRC_FILTER_NONE && filter != TRC_FILTER_ZDELTA && filter != TRC_FILTER_XOR)
        return trc_fail(TRC_E_ARG, "%s: filter %d (0 none, 1 zigzag delta, 2 xor)", who, filter);
    return TRC_OK;
}
// what the filter calls check ahead of everything else, pointers included: the stride, then filter and restart length
static int filter_args(const char *who, int filter, int stride, uint32_t seg)
{
    if (stride < 1 || stride > TRC_STRIDE_MAX) return trc_fail(TRC_E_ARG, "%s: stride %d (1 .. %d)", who, stride, TRC_STRIDE_MAX);
    const int rc = trc_planes_filter_arg(who, filter);
    if (rc) return rc;
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "%s: restart length %u: must be a multiple of 64 in [%u,%u]", who, seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    return TRC_OK;
}

typedef void (*split_fn)(const uint8_t *, size_t, u32, u32, u32, uint8_t *, size_t, uint8_t *);
typedef void (*join_fn)(const uint8_t *, size_t, const uint8_t *, size_t, u32, u32, u32, size_t, uint8_t *);
#define FPLANES_STRIDES(K, E, F) { K<E, F, 1>, K<E, F, 2>, K<E, F, 3>, K<E, F, 4>, K<E, F, 5>, K<E, F, 6>, K<E, F, 7>, K<E, F, 8> }
#define FPLANES_TABLE(K) { { FPLANES_STRIDES(K, 2, TRC_FILTER_ZDELTA), FPLANES_STRIDES(K, 2, TRC_FILTER_XOR) }, \
                           { FPLANES_STRIDES(K, 4, TRC_FILTER_ZDELTA), FPLANES_STRIDES(K, 4, TRC_FILTER_XOR) }, \
                           { FPLANES_STRIDES(K, 8, TRC_FILTER_ZDELTA), FPLANES_STRIDES(K, 8, TRC_FILTER_XOR) } }
// [esize_row][filter - 1][stride - 1]
static const split_fn split_kernels[3][2][TRC_STRIDE_MAX] = FPLANES_TABLE(trc_fplanes_split_kernel);
static const join_fn join_kernels[3][2][TRC_STRIDE_MAX] = FPLANES_TABLE(trc_fplanes_join_kernel);

// `who` names the call in every message: the sfilter calls at stride 1 are the filter calls, and say so
extern "C" int trc_planes_split_sfilter_dev(int filter, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                            void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    int rc = filter_args("planes_split_sfilter", filter, stride, seg);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_split_dev(d_in, n, esize, d_planes, pitch, d_tail, stream);
    const char *who = stride == 1 ? "planes_split_filter" : "planes_split_sfilter";
    if ((rc = planes_args(who, d_in, n, esize, d_planes, pitch, d_tail))) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize), r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    hipLaunchKernelGGL(split_kernels[esize_row(esize)][filter - 1][stride - 1], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_in, m, t, seg, r0, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int trc_planes_join_sfilter_dev(int filter, int stride, const void *d_planes, size_t pitch, const void *d_tail,
                                           size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream)
{
    int rc = filter_args("planes_join_sfilter", filter, stride, seg);
    if (rc) return rc;
    if (filter == TRC_FILTER_NONE) return trc_planes_join_dev(d_planes, pitch, d_tail, n, esize, d_out, stream);
    const char *who = stride == 1 ? "planes_join_filter" : "planes_join_sfilter";
    if ((rc = planes_args(who, d_out, n, esize, d_planes, pitch, d_tail))) return rc;
    const size_t m = n / esize;
    u32 span;
    size_t nspan;
    const unsigned grid = join_grid(m, seg, span, nspan);
    hipLaunchKernelGGL(join_kernels[esize_row(esize)][filter - 1][stride - 1], dim3(grid), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, (u32)(n % esize), seg, span, nspan, (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int trc_planes_split_filter_dev(int filter, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                           void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    const int rc = filter_args("planes_split_filter", filter, 1, seg);
    return rc ? rc : trc_planes_split_sfilter_dev(filter, 1, d_in, n, esize, seg, d_planes, pitch, d_tail, stream);
}

extern "C" int trc_planes_join_filter_dev(int filter, const void *d_planes, size_t pitch, const void *d_tail,
                                          size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream)
{
    const int rc = filter_args("planes_join_filter", filter, 1, seg);
    return rc ? rc : trc_planes_join_sfilter_dev(filter, 1, d_planes, pitch, d_tail, n, esize, seg, d_out, stream);
}
