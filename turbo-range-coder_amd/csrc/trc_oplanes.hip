// trc_oplanes.hip -- the byte-plane split, join and histograms behind a fixed polynomial predictor of ORDER 2 or 3 (the "fixed"
// predictors of the lossless audio coders) at stride S = 1 .. 8: for sampled signals, PCM and sensor series, whose first difference
// is itself smooth.  A translation unit of its own, so that the code objects of trc_fplanes.hip and trc_planes_hist.hip stay what
// they were.  One kernel per (esize, order, stride) and direction; orders 0 and 1 are the kernels of trc_planes.hip / trc_fplanes.hip.
//
// Definition (include/trc_hip.h): x[i] = the m little-endian elements of w = 8 * esize bits, D_S(a)[i] = a[i] where i % seg < S, else
// a[i] - a[i - S] mod 2^w;  y[i] = zigzag(D_S applied ORDER times to x, at i);  plane k = byte k of every y[i].  With x taken as zero
// in front of its segment that is the closed form  D^K[i] = sum_j (-1)^j C(K, j) x[i - j S], which is what the split computes.
//
// Split is the strided split of trc_fplanes.hip with a longer reach: a thread owns a vector of 8 elements and lacks the ORDER * S
// elements in front of it, up to 24, so 1 .. 3 whole vectors -- lines its neighbours load anyway.  seg is a multiple of 64, a vector
// never straddles a restart, and the vector f in front lies in the same segment where v % (seg / 8) >= f; the others count as zero.
//
// Join runs the scan of trc_fplanes_join_kernel ORDER times on the registers of one tile (the walk: trc_planes_scan.h): a level's
// output is the next level's input, complete with its carry before the next level starts, and every level keeps S running values of
// its own.  No LDS beyond the shuffles, no workspace, no dependency between workgroups.
//
// The histograms are those of trc_planes_hist.hip for orders 0 .. 3 under one stride, from one read of the input (trc_planes_count.h
// has the counters): four rows of planes where that kernel has three.
#include "trc_planes_order.h"                     // the reach, the difference, the histogram rows: shared with the batched kernels

// in: 16-byte aligned, m * ESIZE + t bytes.  planes: 256-byte aligned, pitch a multiple of 256.  seg: a multiple of 64.  r0 =
// (m / 8 * 8) % seg, where the elements behind the last whole vector lie in their segment.  Writes [0, m) of every plane and
// [0, t) of tail, nothing else; reads nothing in front of `in`.
template <int ESIZE, int ORDER, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_oplanes_split_kernel(const uint8_t *__restrict__ in, size_t m, u32 t, u32 seg, u32 r0, uint8_t *__restrict__ planes, size_t pitch, uint8_t *__restrict__ tail)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    typedef Reach<ORDER, S> Q;
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
        T a[Q::B + TRC_PLANES_VEC], y[TRC_PLANES_VEC];
        load_reach<ESIZE, ORDER, S>(in, v, r, (u32)Q::NF, a);
        unpack<ESIZE>(w, a + Q::B);
#pragma unroll
        for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = zigzag<ESIZE>(diff<ORDER, S, T>(a + Q::B + j));
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
            const T y = zigzag<ESIZE>(diff_elem<ORDER, T, M>(el, i, r0 + g, (u32)S));
#pragma unroll
            for (int k = 0; k < ESIZE; k++) planes[k * pitch + i] = (uint8_t)(y >> (8 * k));
        } else if (g < rest + t) tail[g - rest] = in[m * ESIZE + (g - rest)];
    }
}

// the mirror image of the split: writes [0, m * ESIZE + t) of out, nothing else.  span, nspan: join_grid (trc_planes_scan.h, which
// also says how the walk goes and why it is written out here).  carry[l][c] = the running value of class c at level l where the
// previous tile ended; level l undoes one D_S, so its output is level l + 1's input and the last level's is x.
template <int ESIZE, int ORDER, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_oplanes_join_kernel(const uint8_t *__restrict__ planes, size_t pitch, const uint8_t *__restrict__ tail, size_t m, u32 t, u32 seg, u32 span,
                             size_t nspan, uint8_t *__restrict__ out)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int F = TRC_FILTER_ZDELTA;
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
        T carry[ORDER][NP];
#pragma unroll
        for (int l = 0; l < ORDER; l++) {
#pragma unroll
            for (int c = 0; c < NP; c++) carry[l][c] = 0;
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
#pragma unroll
            for (int j = 0; j < V; j++) e[j] = operand<ESIZE, F>(e[j]);
            const u32 reach = ahead < lane ? ahead : lane;               // lanes in front of this one in its segment and in this tile
            const bool take = ahead > lane;                              // the lane's segment began in an earlier tile
#pragma unroll
            for (int l = 0; l < ORDER; l++) {
#pragma unroll
                for (int j = S; j < V; j++) e[j] = e[j] + e[j - S];
                // the lane's totals by class: element 8 - S + i has class (r8 + 8 + i) % S
                T inc[S];
                if constexpr (ROT) {
                    const u32 rot = (r8 + V) % (u32)S;
                    rotate<S>(e + V - S, rot ? (u32)S - rot : 0u, inc);
                } else {
#pragma unroll
                    for (int c = 0; c < S; c++) inc[c] = e[V - S + c];
                }
                T before[S];                                             // per class: the lanes in front of it, and the earlier tiles
                if constexpr (ESIZE == 2) {                              // two classes to a word: half the shuffles
                    u32 pk[NP], pb[NP];
#pragma unroll
                    for (int i = 0; i < NP; i++) {
                        constexpr int LAST = S - 1;
                        const int hi = 2 * i + 1 < S ? 2 * i + 1 : LAST; // (an odd S: the last word holds one class)
                        pk[i] = (inc[2 * i] & 0xffffu) | (2 * i + 1 < S ? inc[hi] << 16 : 0u);
                    }
                    wave_scan<F, NP, u32, true>(pk, carry[l], pb, reach, take);
#pragma unroll
                    for (int c = 0; c < S; c++) before[c] = c & 1 ? pb[c / 2] >> 16 : pb[c / 2];       // (junk above bit 15, as everywhere)
                } else wave_scan<F, S, T, false>(inc, carry[l], before, reach, take);
                if constexpr (ROT) {
                    T loc[S];
                    rotate<S>(before, r8, loc);                          // loc[i] = before[(r8 + i) % S]: element j takes loc[j % S]
#pragma unroll
                    for (int j = 0; j < V; j++) e[j] = e[j] + loc[j % S];
                } else {
#pragma unroll
                    for (int j = 0; j < V; j++) e[j] = e[j] + before[j % S];
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

// ---- the histograms of orders 0 .. 3 (rows and flushes: trc_planes_order.h) -------------------------------------------------------

// in: 16-byte aligned, m * ESIZE bytes are read, nothing in front of them.  seg: a multiple of 64.  r0 = (m / 8 * 8) % seg.  orders:
// bit k = count order k, 1 .. 15.  hist[(k * ESIZE + p) * 256 + b] += the elements whose byte p under order k is b; the rows of
// other orders are not touched.  Dynamic LDS: (requested orders * ESIZE * 256 * 4) << cshift bytes.  round_vecs >= 1.
template <int ESIZE, int S> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_oplanes_hist_kernel(const uint8_t *__restrict__ in, size_t m, u32 seg, u32 r0, u32 orders, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    typedef Reach<3, S> Q;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const OrderRows R = order_rows<ESIZE>(sm, orders, cshift);
    const u32 top = orders & 8u ? 3u : orders & 4u ? 2u : orders & 2u ? 1u : 0u;         // the highest order counted ...
    const u32 need = (top * (u32)S + TRC_PLANES_VEC - 1) / TRC_PLANES_VEC;               // ... reaches into this many vectors in front

    const size_t nv = m / TRC_PLANES_VEC, step = (size_t)gridDim.x * TRC_PLANES_BLOCK, b0 = (size_t)blockIdx.x * TRC_PLANES_BLOCK;
    const size_t turns = b0 < nv ? (nv - b0 + step - 1) / step : 0;      // of the whole workgroup: the flush holds barriers
    const M *el = (const M *)in;
    const u32 vseg = seg / TRC_PLANES_VEC, rstep = (u32)(step % vseg);
    u32 r = (u32)((b0 + tid) % vseg), since = 0;                         // the vector's place in its segment: 0 opens one
    size_t v = b0 + tid;
    for (size_t it = 0; it < turns; it++, v += step) {
        if (v < nv) {
            const uint4 *src = (const uint4 *)(in + v * (TRC_PLANES_VEC * ESIZE));
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            T a[Q::B + TRC_PLANES_VEC], y[TRC_PLANES_VEC];
            load_reach<ESIZE, 3, S>(in, v, r, need, a);
            unpack<ESIZE>(w, a + Q::B);
            if (orders & 1u) count_vec<ESIZE>(sm, R.row[0], cshift, w);
            if (orders & 2u) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = zigzag<ESIZE>(diff<1, S, T>(a + Q::B + j));
                pack<ESIZE>(y, w);
                count_vec<ESIZE>(sm, R.row[1], cshift, w);
            }
            if (orders & 4u) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = zigzag<ESIZE>(diff<2, S, T>(a + Q::B + j));
                pack<ESIZE>(y, w);
                count_vec<ESIZE>(sm, R.row[2], cshift, w);
            }
            if (orders & 8u) {
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = zigzag<ESIZE>(diff<3, S, T>(a + Q::B + j));
                pack<ESIZE>(y, w);
                count_vec<ESIZE>(sm, R.row[3], cshift, w);
            }
        }
        r += rstep;
        if (r >= vseg) r -= vseg;
        if (++since == round_vecs && it + 1 < turns) { order_flush<ESIZE>(sm, R.nf, orders, cshift, hist); since = 0; }
    }
    // the elements behind the last whole vector (at most 7), one per lane
    if (blockIdx.x == 0) {
        const u32 rest = (u32)(m - nv * TRC_PLANES_VEC);
        if (tid < rest) {
            const size_t i = nv * TRC_PLANES_VEC + tid;
            if (orders & 1u) count_elem<ESIZE>(sm, R.row[0], cshift, (T)el[i]);
            if (orders & 2u) count_elem<ESIZE>(sm, R.row[1], cshift, zigzag<ESIZE>(diff_elem<1, T, M>(el, i, r0 + tid, (u32)S)));
            if (orders & 4u) count_elem<ESIZE>(sm, R.row[2], cshift, zigzag<ESIZE>(diff_elem<2, T, M>(el, i, r0 + tid, (u32)S)));
            if (orders & 8u) count_elem<ESIZE>(sm, R.row[3], cshift, zigzag<ESIZE>(diff_elem<3, T, M>(el, i, r0 + tid, (u32)S)));
        }
    }
    order_flush<ESIZE>(sm, R.nf, orders, cshift, hist);
}

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
// what the order calls check ahead of everything else, pointers included: the order, then the stride
int trc_planes_order_arg(const char *who, int order, int stride)
{
    if (order < 0 || order > TRC_ORDER_MAX) return trc_fail(TRC_E_ARG, "%s: order %d (0 .. %d)", who, order, TRC_ORDER_MAX);
    if (stride < 1 || stride > TRC_STRIDE_MAX) return trc_fail(TRC_E_ARG, "%s: stride %d (1 .. %d)", who, stride, TRC_STRIDE_MAX);
    return TRC_OK;
}
static int seg_arg(const char *who, uint32_t seg)
{
    if (seg < TRC_CHUNK_MIN || seg > TRC_CHUNK_MAX || seg % 64u)
        return trc_fail(TRC_E_ARG, "%s: restart length %u: must be a multiple of 64 in [%u,%u]", who, seg, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    return TRC_OK;
}

typedef void (*split_fn)(const uint8_t *, size_t, u32, u32, u32, uint8_t *, size_t, uint8_t *);
typedef void (*join_fn)(const uint8_t *, size_t, const uint8_t *, size_t, u32, u32, u32, size_t, uint8_t *);
#define OPLANES_STRIDES(K, E, O) { K<E, O, 1>, K<E, O, 2>, K<E, O, 3>, K<E, O, 4>, K<E, O, 5>, K<E, O, 6>, K<E, O, 7>, K<E, O, 8> }
#define OPLANES_TABLE(K) { { OPLANES_STRIDES(K, 2, 2), OPLANES_STRIDES(K, 2, 3) }, { OPLANES_STRIDES(K, 4, 2), OPLANES_STRIDES(K, 4, 3) }, \
                           { OPLANES_STRIDES(K, 8, 2), OPLANES_STRIDES(K, 8, 3) } }
// [esize_row][order - 2][stride - 1]
static const split_fn split_kernels[3][2][TRC_STRIDE_MAX] = OPLANES_TABLE(trc_oplanes_split_kernel);
static const join_fn join_kernels[3][2][TRC_STRIDE_MAX] = OPLANES_TABLE(trc_oplanes_join_kernel);

// (order 0 is the unfiltered call, order 1 the strided zigzag delta: those calls run, and name themselves in their messages)
extern "C" int trc_planes_split_ofilter_dev(int order, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                            void *d_planes, size_t pitch, void *d_tail, void *stream)
{
    int rc = trc_planes_order_arg("planes_split_ofilter", order, stride);
    if (rc) return rc;
    if (order < 2) return trc_planes_split_sfilter_dev(order ? TRC_FILTER_ZDELTA : TRC_FILTER_NONE, stride, d_in, n, esize, seg, d_planes, pitch, d_tail, stream);
    if ((rc = seg_arg("planes_split_ofilter", seg)) || (rc = planes_args("planes_split_ofilter", d_in, n, esize, d_planes, pitch, d_tail))) return rc;
    const size_t m = n / esize;
    const uint32_t t = (uint32_t)(n % esize), r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    hipLaunchKernelGGL(split_kernels[esize_row(esize)][order - 2][stride - 1], dim3(planes_grid(m)), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_in, m, t, seg, r0, (uint8_t *)d_planes, pitch, (uint8_t *)d_tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_split_ofilter: %s", hipGetErrorString(e));
}

extern "C" int trc_planes_join_ofilter_dev(int order, int stride, const void *d_planes, size_t pitch, const void *d_tail,
                                           size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream)
{
    int rc = trc_planes_order_arg("planes_join_ofilter", order, stride);
    if (rc) return rc;
    if (order < 2) return trc_planes_join_sfilter_dev(order ? TRC_FILTER_ZDELTA : TRC_FILTER_NONE, stride, d_planes, pitch, d_tail, n, esize, seg, d_out, stream);
    if ((rc = seg_arg("planes_join_ofilter", seg)) || (rc = planes_args("planes_join_ofilter", d_out, n, esize, d_planes, pitch, d_tail))) return rc;
    const size_t m = n / esize;
    u32 span;
    size_t nspan;
    const unsigned grid = join_grid(m, seg, span, nspan);
    hipLaunchKernelGGL(join_kernels[esize_row(esize)][order - 2][stride - 1], dim3(grid), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)d_planes, pitch, (const uint8_t *)d_tail, m, (u32)(n % esize), seg, span, nspan, (uint8_t *)d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_join_ofilter: %s", hipGetErrorString(e));
}

extern "C" size_t trc_planes_hist_order_bytes(unsigned esize)
{
    return esize_ok(esize) ? (size_t)TRC_OHIST_ORDERS * esize * 256 * sizeof(uint64_t) : 0;
}

typedef void (*hist_fn)(const uint8_t *, size_t, u32, u32, u32, u32, u32, u64a *);
#define OHIST_STRIDES(E) { trc_oplanes_hist_kernel<E, 1>, trc_oplanes_hist_kernel<E, 2>, trc_oplanes_hist_kernel<E, 3>, trc_oplanes_hist_kernel<E, 4>, \
                           trc_oplanes_hist_kernel<E, 5>, trc_oplanes_hist_kernel<E, 6>, trc_oplanes_hist_kernel<E, 7>, trc_oplanes_hist_kernel<E, 8> }
static const hist_fn hist_kernels[3][TRC_STRIDE_MAX] = { OHIST_STRIDES(2), OHIST_STRIDES(4), OHIST_STRIDES(8) };       // [esize_row][stride - 1]

extern "C" int trc_planes_hist_order_dev(unsigned orders, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg, uint64_t *d_hist, void *stream)
{
    const char *who = "planes_hist_order";
    if (orders < 1 || orders > 15) return trc_fail(TRC_E_ARG, "%s: orders 0x%x (a bit set: bit k = order k, 1 .. 15)", who, orders);
    if (stride < 1 || stride > TRC_STRIDE_MAX) return trc_fail(TRC_E_ARG, "%s: stride %d (1 .. %d)", who, stride, TRC_STRIDE_MAX);
    int rc = seg_arg(who, seg);
    if (rc) return rc;
    if (!esize_ok(esize)) return trc_fail(TRC_E_ARG, "%s: esize %u (2, 4 or 8)", who, esize);
    if (n < esize) return trc_fail(TRC_E_ARG, "%s: %zu bytes hold no element of %u bytes", who, n, esize);
    if (!d_in || !d_hist || ((uintptr_t)d_in & 15) || ((uintptr_t)d_hist & 7))
        return trc_fail(TRC_E_ARG, "%s: the element buffer must be 16-byte, the histogram 8-byte aligned", who);
    const size_t m = n / esize;
    const uint32_t r0 = (uint32_t)((m / TRC_PLANES_VEC * TRC_PLANES_VEC) % seg);
    const HistShape h = hist_shape(orders, esize);
    unsigned grid = planes_grid(m);
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_order_bytes(esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
    hipLaunchKernelGGL(hist_kernels[esize_row(esize)][stride - 1], dim3(grid), dim3(TRC_PLANES_BLOCK), h.lds, s,
                       (const uint8_t *)d_in, m, seg, r0, orders, h.cshift, h.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
}
