// trc_oplanes_batch.inc -- the batched split, join and histograms of trc_planes_batch.hip (which includes this file behind
// trc_splanes_batch.inc) with a filter, a stride AND A PREDICTOR ORDER per item: the fixed polynomial predictors of trc_oplanes.hip,
// restarted at every chunk, where order and stride are run-time properties of the item.
//
// Definition (include/trc_hip.h): GO(i) = item i where filters[i] == TRC_FILTER_NONE, F_{strides[i]}(TRC_FILTER_XOR, seg = chunk,
// esize, item i) where it is TRC_FILTER_XOR, O(orders[i], strides[i], seg = chunk, esize, item i) where it is TRC_FILTER_ZDELTA;
// VO = V([GO(0) .. GO(count - 1)]).  Plan, pad, restart and read rules are those of the strided batch.  A batch in which no ZDELTA
// item has an order above 1 never comes here: it launches the kernels of trc_splanes_batch.inc or those in front of them.
//
// The order travels in the item's record next to filter and stride: order - 1 in bits 59 .. 60 of v0, so a record of order 1 is the
// strided batch's record bit for bit.  The host stores 1 for an item whose filter is not ZDELTA.
//
// Everything that depends on order or stride is a body that is static in both (trc_planes_order.h, trc_planes_scan.h), entered by
// a branch; a reach indexed at run time would put the register arrays into scratch:
//   split      per thread, as trc_splanes_split_batch_kernel: a vector never straddles a chunk, so it has one item and one (filter,
//              order, stride).  Order 1 and xor take that kernel's svec_fwd; orders 2 and 3 load the 1 .. 3 whole vectors in front of
//              the thread's own (load_reach: those that lie in the vector's chunk, so in its item; the others count as zero).
//   histogram  per workgroup: the item is workgroup-uniform there.
//   join       per WAVE, as trc_splanes_join_batch_kernel: a pass per distinct (filter, order, stride) among the tile's storing
//              lanes, all lanes active, a lane keeping the result only where the triple is its own.  A pass of order K runs the static
//              scan K times on the registers of the tile, level after level, as trc_oplanes_join_kernel does.
//              The carry is kept per LEVEL and class across tiles: 3 levels x 8 classes (4 packed pairs for 16-bit elements), and
//              as many again for next[], because a tile's passes all read the previous tile's carry whichever of them leaves the next
//              one.  A carry is the value of lane 63 and so the same in all lanes: it is taken through v_readfirstlane_b32 when it is
//              committed, which lets the compiler keep carry[] and next[] in scalar registers (profiles/planes/obatch_notes.md has
//              the resource report of both forms).

#define OBATCH_SHIFT 59
#define OBATCH_ORDER(r) ((((u32)((r).v0 >> OBATCH_SHIFT)) & 3u) + 1u)
#define OBATCH_EACH_HIGH(X) X(2, 1) X(2, 2) X(2, 3) X(2, 4) X(2, 5) X(2, 6) X(2, 7) X(2, 8) X(3, 1) X(3, 2) X(3, 3) X(3, 4) X(3, 5) X(3, 6) X(3, 7) X(3, 8)

// a whole vector's words behind the predictor of ORDER (2 or 3) at stride S; in = the item, lv = the vector's number in it,
// rv = the vector's place in its chunk, in vectors: the vectors in front of it are loaded where they lie in the chunk
template <int ESIZE, int ORDER, int S> __device__ __forceinline__ void ovec_fwd(u32 *w, const uint8_t *__restrict__ in, size_t lv, u32 rv)
{
    typedef typename Elem<ESIZE>::T T;
    typedef Reach<ORDER, S> Q;
    T a[Q::B + TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    load_reach<ESIZE, ORDER, S>(in, lv, rv, (u32)Q::NF, a);
    unpack<ESIZE>(w, a + Q::B);
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = zigzag<ESIZE>(diff<ORDER, S, T>(a + Q::B + j));
    pack<ESIZE>(y, w);
}

// arguments, reads and writes: as trc_splanes_split_batch_kernel, whose walk this is (keep the two alike).  The vectors in front of
// a whole vector that lie in its chunk are whole vectors of the item; the item's last, partial vector is read element by element,
// each with the elements j * S in front of it where its place in the chunk is at least j * S (diff_elem's rule).
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_oplanes_split_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp,
                                    size_t nv, size_t M, uint8_t *__restrict__ planes, size_t pitch)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const u32 c = vec_chunk(v, vpc, rcp);
        const BatchRec r = rec[chunk_item[c]];
        const u32 f = FBATCH_FILTER(r), st = SBATCH_STRIDE(r), ord = OBATCH_ORDER(r);
        const size_t lv = v - SBATCH_V0(r), e = lv * TRC_PLANES_VEC, vb = v * TRC_PLANES_VEC;
        const u32 rv = (u32)(v - (size_t)c * vpc), place = rv * TRC_PLANES_VEC;      // the vector's place in its chunk: 0 opens one
        const uint8_t *in = (const uint8_t *)r.ptr;
        const EM *el = (const EM *)in;
        uint8_t *dst = planes + vb;
        if (e + TRC_PLANES_VEC <= r.m) {
            const uint4 *src = (const uint4 *)(in + e * ESIZE);
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            if (f != TRC_FILTER_NONE) {
                switch (ord * 8u + st) {
#define OB_CASE1(S) case 8 + S: svec_fwd<ESIZE, S>(w, f, in, lv, place != 0); break;
#define OB_CASE(K, S) case K * 8 + S: ovec_fwd<ESIZE, K, S>(w, in, lv, rv); break;
                SBATCH_EACH_STRIDE(OB_CASE1)
                OBATCH_EACH_HIGH(OB_CASE)
#undef OB_CASE
#undef OB_CASE1
                }
            }
            uint2 p[ESIZE];
            vec_split<ESIZE>(w, p);
#pragma unroll
            for (int k = 0; k < ESIZE; k++) *(uint2 *)(dst + k * pitch) = p[k];
        } else if (e < r.m) {                      // the item's last vector: rest of its elements, then zeros as split_rest
            const u32 rest = (u32)(r.m - e), lim = vb + TRC_PLANES_VEC <= M ? TRC_PLANES_VEC : rest;
#pragma unroll 1
            for (u32 j = 0; j < lim; j++) {
                T y = 0;
                if (j < rest) {
                    const T x = el[e + j];
                    y = x;
                    if (ord == 2u) y = zigzag<ESIZE>(diff_elem<2, T, EM>(el, e + j, place + j, st));
                    else if (ord == 3u) y = zigzag<ESIZE>(diff_elem<3, T, EM>(el, e + j, place + j, st));
                    else if (f != TRC_FILTER_NONE) y = fwd_of<ESIZE>(f, x, place + j >= st ? (T)el[e + j - st] : (T)0);
                }
#pragma unroll
                for (int k = 0; k < ESIZE; k++) dst[k * pitch + j] = (uint8_t)(y >> (8 * k));
            }
        } else {
#pragma unroll
            for (int k = 0; k < ESIZE; k++) *(uint2 *)(dst + k * pitch) = make_uint2(0u, 0u);
        }
    }
}

// ---- join ----------------------------------------------------------------------------------------------------------------------
// a value that is the same in all lanes, through the scalar unit
__device__ __forceinline__ u32 obatch_uni(u32 x) { return (u32)__builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t obatch_uni(uint64_t x)      // (the builtin gives an int: each half is made unsigned before it is widened)
{
    const u32 hi = (u32)__builtin_amdgcn_readfirstlane((u32)(x >> 32)), lo = (u32)__builtin_amdgcn_readfirstlane((u32)x);
    return ((uint64_t)hi << 32) | lo;
}

// one pass of a tile under the predictor of ORDER (2 or 3) at stride S, both static: the levels of trc_oplanes_join_kernel<ESIZE,
// ORDER, S> as they stand there.  e[], mine, commit, lane, ahead, nin: as sbatch_scan.  carry[l * NC + c]: class c of the running
// value of level l where the previous tile ended (16-bit elements: two classes to a word, at every stride); where `commit`,
// next[] <- the same where this tile ends.  Every lane of the wave calls this (shuffles).
template <int ESIZE, int ORDER, int S, int NC> __device__ __forceinline__ void obatch_scan(typename Elem<ESIZE>::T *e, bool mine, bool commit, u32 lane, u32 ahead, u32 nin,
                                                                                           const typename Elem<ESIZE>::T *carry, typename Elem<ESIZE>::T *next)
{
    typedef typename Elem<ESIZE>::T T;
    constexpr int F = TRC_FILTER_ZDELTA, V = TRC_PLANES_VEC;
    constexpr bool ROT = (V % S) != 0;                                   // S divides 8: a lane's element j has class j % S
    constexpr int NP = ESIZE == 2 ? (S + 1) / 2 : S;
    const u32 reach = ahead < lane ? ahead : lane;                       // lanes in front of this one in its chunk and in this tile
    const bool take = ahead > lane;                                      // the lane's chunk began in an earlier tile
    const u32 r8 = ROT ? nin % (u32)S : 0u;                              // the class of the lane's first element
    T x[V];
#pragma unroll
    for (int j = 0; j < V; j++) x[j] = operand<ESIZE, F>(e[j]);
#pragma unroll
    for (int l = 0; l < ORDER; l++) {
#pragma unroll
        for (int j = S; j < V; j++) x[j] = x[j] + x[j - S];
        T inc[S];                                                        // the lane's totals by class
        if constexpr (ROT) {
            const u32 rot = (r8 + V) % (u32)S;
            rotate<S>(x + V - S, rot ? (u32)S - rot : 0u, inc);
        } else {
#pragma unroll
            for (int c = 0; c < S; c++) inc[c] = x[V - S + c];
        }
        T before[S], run[NP];                                            // run: wave_scan reads and renews one carry array
#pragma unroll
        for (int c = 0; c < NP; c++) run[c] = carry[l * NC + c];
        if constexpr (ESIZE == 2) {                                      // two classes to a word: half the shuffles
            u32 pk[NP], pb[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) {
                constexpr int LAST = S - 1;
                const int hi = 2 * i + 1 < S ? 2 * i + 1 : LAST;         // (an odd S: the last word holds one class)
                pk[i] = (inc[2 * i] & 0xffffu) | (2 * i + 1 < S ? inc[hi] << 16 : 0u);
            }
            wave_scan<F, NP, u32, true>(pk, run, pb, reach, take);
#pragma unroll
            for (int c = 0; c < S; c++) before[c] = c & 1 ? pb[c / 2] >> 16 : pb[c / 2];
        } else wave_scan<F, S, T, false>(inc, run, before, reach, take);
        if (commit) {
#pragma unroll
            for (int c = 0; c < NP; c++) next[l * NC + c] = obatch_uni(run[c]);
        }
        if constexpr (ROT) {
            T loc[S];
            rotate<S>(before, r8, loc);                                  // loc[i] = before[(r8 + i) % S]: element j takes loc[j % S]
#pragma unroll
            for (int j = 0; j < V; j++) x[j] = x[j] + loc[j % S];
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) x[j] = x[j] + before[j % S];
        }
    }
#pragma unroll
    for (int j = 0; j < V; j++) if (mine) e[j] = x[j];
}

// a pass of order 1 or xor: sbatch_scan on level 0 of the carry, its carry out taken through the scalar unit as well
template <int ESIZE, int FILTER, int S, int NC> __device__ __forceinline__ void obatch_scan1(typename Elem<ESIZE>::T *e, bool mine, bool commit, u32 lane, u32 ahead, u32 nin,
                                                                                             const typename Elem<ESIZE>::T *carry, typename Elem<ESIZE>::T *next)
{
    typedef typename Elem<ESIZE>::T T;
    T out[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) out[c] = 0;
    sbatch_scan<ESIZE, FILTER, S>(e, mine, commit, lane, ahead, nin, carry, out);
    if (commit) {
#pragma unroll
        for (int c = 0; c < NC; c++) next[c] = obatch_uni(out[c]);       // (the classes the pass does not use: never read by its successor)
    }
}

// arguments, reads and writes: as trc_splanes_join_batch_kernel, whose walk this is (keep the two alike)
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_oplanes_join_batch_kernel(const uint8_t *__restrict__ planes, size_t pitch, const BatchRec *__restrict__ rec,
                                   const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp, size_t elems, u32 chunk, u32 span, size_t nspan)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    constexpr int NC = ESIZE == 2 ? TRC_STRIDE_MAX / 2 : TRC_STRIDE_MAX, NCARRY = TRC_ORDER_MAX * NC;
    const u32 lane = threadIdx.x & 63u;
    const size_t waves = (size_t)gridDim.x * (TRC_PLANES_BLOCK / 64);
    size_t s = (size_t)blockIdx.x * (TRC_PLANES_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u32 tile = 0;
    if (s >= nspan) return;
    u32 len = (u32)(elems - s * span < span ? elems - s * span : span);
    u32 at = lane * TRC_PLANES_VEC;
    u32 nin = wrap_seg(at, chunk);
    u32 ncnt = at < len ? (len - at < TRC_PLANES_VEC ? len - at : TRC_PLANES_VEC) : 0;
    size_t nbase = s * span + at;
    uint2 pn[ESIZE];
    BatchRec rn = { 0, 0, 0, 0 };                  // (m = 0: a lane behind the range stores nothing)
    tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
    if (ncnt) rn = rec[chunk_item[vec_chunk(nbase / TRC_PLANES_VEC, vpc, rcp)]];
    T carry[NCARRY];
#pragma unroll
    for (int c = 0; c < NCARRY; c++) carry[c] = 0;
    for (;;) {
        uint2 p[ESIZE];
#pragma unroll
        for (int k = 0; k < ESIZE; k++) p[k] = pn[k];
        const BatchRec r = rn;
        const size_t base = nbase;
        const u32 in_chunk = nin, ahead = nin / TRC_PLANES_VEC;
        // the wave's next tile: its plane loads and its map and record loads are under way while this one is scanned
        tile++;
        bool more = true;
        if (tile * TRC_FPLANES_TILE >= len) {
            s += waves; tile = 0;
            more = s < nspan;
            if (more) len = (u32)(elems - s * span < span ? elems - s * span : span);
            nin = wrap_seg(lane * TRC_PLANES_VEC, chunk);
        } else nin = wrap_seg(nin + TRC_FPLANES_TILE, chunk);
        if (more) {
            at = tile * TRC_FPLANES_TILE + lane * TRC_PLANES_VEC;
            ncnt = at < len ? (len - at < TRC_PLANES_VEC ? len - at : TRC_PLANES_VEC) : 0;
            nbase = s * span + at;
            tile_load<ESIZE>(planes, pitch, nbase, ncnt, pn);
            rn.m = 0;
            if (ncnt) rn = rec[chunk_item[vec_chunk(nbase / TRC_PLANES_VEC, vpc, rcp)]];
        }
        // what the lane stores: 8 = a whole vector, 1 .. 7 = the item's last vector, 0 = pad or behind the range
        const size_t eo = (base / TRC_PLANES_VEC - SBATCH_V0(r)) * TRC_PLANES_VEC;
        const u32 cnt = eo + TRC_PLANES_VEC <= r.m ? TRC_PLANES_VEC : eo < r.m ? (u32)(r.m - eo) : 0;
        // the lane's predictor as one word: filter * 32 + order * 8 + stride - 1 ...
        const u32 key = FBATCH_FILTER(r) * 32u + OBATCH_ORDER(r) * 8u + (SBATCH_STRIDE(r) - 1u);
        const u32 key63 = __builtin_amdgcn_readlane(key, 63);           // ... and whose carry the next tile's first chunk takes
        const bool scans = FBATCH_FILTER(r) != TRC_FILTER_NONE && cnt != 0;
        u32 w[NW];
        vec_join<ESIZE>(p, w);
        T e[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
        // a pass per distinct predictor among the lanes that scan and store; the ballot is wave-uniform, so every lane takes every pass
        T next[NCARRY];
#pragma unroll
        for (int c = 0; c < NCARRY; c++) next[c] = carry[c];
#define OB_KEY(F, K, S) ((u32)(F) * 32u + (u32)(K) * 8u + (u32)(S) - 1u)
#define OB_PASS1_F(F, S) { const bool mine = scans && key == OB_KEY(F, 1, S); \
                           if (__ballot(mine) != 0) obatch_scan1<ESIZE, F, S, NC>(e, mine, key63 == OB_KEY(F, 1, S), lane, ahead, in_chunk, carry, next); }
#define OB_PASS1(S) OB_PASS1_F(TRC_FILTER_ZDELTA, S) OB_PASS1_F(TRC_FILTER_XOR, S)
#define OB_PASS(K, S) { const bool mine = scans && key == OB_KEY(TRC_FILTER_ZDELTA, K, S); \
                        if (__ballot(mine) != 0) obatch_scan<ESIZE, K, S, NC>(e, mine, key63 == OB_KEY(TRC_FILTER_ZDELTA, K, S), lane, ahead, in_chunk, carry, next); }
        SBATCH_EACH_STRIDE(OB_PASS1)
        OBATCH_EACH_HIGH(OB_PASS)
#undef OB_PASS
#undef OB_PASS1
#undef OB_PASS1_F
#undef OB_KEY
#pragma unroll
        for (int c = 0; c < NCARRY; c++) carry[c] = next[c];
        if (cnt == TRC_PLANES_VEC) {
            pack<ESIZE>(e, w);
            uint4 *dst = (uint4 *)(r.ptr + eo * ESIZE);
#pragma unroll
            for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        } else if (cnt) {
            EM *dst = (EM *)r.ptr + eo;
#pragma unroll
            for (int j = 0; j < TRC_PLANES_VEC - 1; j++) if ((u32)j < cnt) dst[j] = (EM)e[j];
        }
        if (!more) break;
    }
}

// ---- the order advisor's histograms ---------------------------------------------------------------------------------------------
// one whole vector of an item at stride S under every requested order: lv = its number in the item, rv = its place in its chunk in
// vectors, need = the vectors in front that the highest requested order reaches into (trc_oplanes_hist_kernel's counting)
template <int ESIZE, int S> __device__ __forceinline__ void ohist_vec(u32 *sm, const OrderRows &R, u32 orders, u32 cshift, const uint8_t *__restrict__ in,
                                                                      size_t lv, u32 rv, u32 top)
{
    typedef typename Elem<ESIZE>::T T;
    typedef Reach<3, S> Q;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const u32 need = (top * (u32)S + TRC_PLANES_VEC - 1) / TRC_PLANES_VEC;
    const uint4 *src = (const uint4 *)(in + lv * (TRC_PLANES_VEC * ESIZE));
    u32 w[NW];
#pragma unroll
    for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
    T a[Q::B + TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    load_reach<ESIZE, 3, S>(in, lv, rv, need, a);
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

// trc_planes_hist_sbatch_kernel with the rows of orders 0 .. 3: arguments (orders: the bit set), walk, flushes and reads are that
// kernel's (keep the two alike); hist: 4 * ESIZE * 256 counters per record.  Dynamic LDS: (requested orders * ESIZE * 256 * 4) << cshift.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_obatch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 nc, u32 cpw, u32 chunk,
                                   u32 orders, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const OrderRows R = order_rows<ESIZE>(sm, orders, cshift);
    const u32 top = orders & 8u ? 3u : orders & 4u ? 2u : orders & 2u ? 1u : 0u;         // the highest order counted

    const u32 vpc = chunk / TRC_PLANES_VEC, rstep = TRC_PLANES_BLOCK % vpc;
    const u32 c_lo = blockIdx.x * cpw, c_hi = nc - c_lo < cpw ? nc : c_lo + cpw;      // (the host: c_lo < nc)
    for (u32 c = c_lo; c < c_hi; ) {
        const u32 item = __builtin_amdgcn_readfirstlane(chunk_item[c]);
        const BatchRec r = rec[item];
        const u32 st = __builtin_amdgcn_readfirstlane(SBATCH_STRIDE(r));
        const u32 first = (u32)r.first, nci = (u32)((r.m + chunk - 1) / chunk);
        const u32 c_end = first + nci < c_hi ? first + nci : c_hi;       // the run's part of the item: chunks [c, c_end)
        const size_t nvi = r.m / TRC_PLANES_VEC;                         // the item's whole vectors
        const size_t lv0 = (size_t)(c - first) * vpc, lv_run = (size_t)(c_end - first) * vpc, lv1 = lv_run < nvi ? lv_run : nvi;
        const size_t turns = lv1 > lv0 ? (lv1 - lv0 + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK : 0;
        const uint8_t *in = (const uint8_t *)r.ptr;
        const EM *el = (const EM *)in;
        u64a *h = hist + (size_t)item * (TRC_OHIST_ORDERS * ESIZE * 256u);
        bool alone = c == first && c_end == first + nci;                 // the item is this run's alone, and not flushed yet
        u32 rr = tid % vpc, since = 0;                                   // the vector's place in its chunk (lv0 opens one): 0 opens one
        size_t lv = lv0 + tid;
        for (size_t it = 0; it < turns; it++, lv += TRC_PLANES_BLOCK) {
            if (lv < lv1) {
                switch (st) {
#define OB_CASE(S) case S: ohist_vec<ESIZE, S>(sm, R, orders, cshift, in, lv, rr, top); break;
                SBATCH_EACH_STRIDE(OB_CASE)
#undef OB_CASE
                }
            }
            rr += rstep;
            if (rr >= vpc) rr -= vpc;
            if (++since == round_vecs && it + 1 < turns) { order_flush_item<ESIZE>(sm, R.nf, orders, cshift, h, alone); alone = false; since = 0; }
        }
        // the elements behind the item's last whole vector (at most 7), one per lane, where the run holds the item's last chunk
        if (c_end == first + nci) {
            const u32 rest = (u32)(r.m - nvi * TRC_PLANES_VEC);
            if (tid < rest) {
                const size_t i = nvi * TRC_PLANES_VEC + tid;
                const u32 at = (u32)(i % chunk);
                if (orders & 1u) count_elem<ESIZE>(sm, R.row[0], cshift, (T)el[i]);
                if (orders & 2u) count_elem<ESIZE>(sm, R.row[1], cshift, zigzag<ESIZE>(diff_elem<1, T, EM>(el, i, at, st)));
                if (orders & 4u) count_elem<ESIZE>(sm, R.row[2], cshift, zigzag<ESIZE>(diff_elem<2, T, EM>(el, i, at, st)));
                if (orders & 8u) count_elem<ESIZE>(sm, R.row[3], cshift, zigzag<ESIZE>(diff_elem<3, T, EM>(el, i, at, st)));
            }
        }
        order_flush_item<ESIZE>(sm, R.nf, orders, cshift, h, alone);
        c = c_end;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// orders[0 .. count): every entry 1 .. TRC_ORDER_MAX (host only; also the coded calls' check, trc_planes_batch.inc), looked at
// behind the strides.  *ordered (may be NULL) <- whether a ZDELTA item has an order above 1; orders == NULL is order 1
int trc_planes_batch_orders(const char *who, const uint8_t *filters, const uint8_t *orders, size_t count, bool *ordered)
{
    // A batch has up to 2^20 items and a batch of order 1 is to cost what it costs without orders: the leading entries that are 1 are
    // passed eight to a word; what lies behind them takes one pass without a branch, and the item is looked for only where one is bad.
    size_t i0 = 0;
    if (orders)
        for (uint64_t w; i0 + 8 <= count && (__builtin_memcpy(&w, orders + i0, 8), w == 0x0101010101010101ull); ) i0 += 8;
    unsigned bad = 0, a = 0;
    for (size_t i = i0; orders && i < count; i++) {
        bad |= (unsigned)(uint8_t)(orders[i] - 1u) > (unsigned)(TRC_ORDER_MAX - 1);
        a |= filters ? (unsigned)(orders[i] > 1) & (unsigned)(filters[i] == TRC_FILTER_ZDELTA) : 0u;
    }
    for (size_t i = 0; bad && i < count; i++)
        if (orders[i] < 1 || orders[i] > TRC_ORDER_MAX)
            return trc_fail(TRC_E_ARG, "%s: item %zu: order %u (1 .. %d)", who, i, (unsigned)orders[i], TRC_ORDER_MAX);
    if (ordered) *ordered = a != 0;
    return TRC_OK;
}

// behind fbatch_pack and sbatch_pack: the orders of the ZDELTA items
static void obatch_pack(std::vector<BatchRec> &recs, const uint8_t *filters, const uint8_t *orders)
{
    for (size_t i = 0; i < recs.size(); i++)
        if (filters[i] == TRC_FILTER_ZDELTA) recs[i].v0 |= (uint64_t)(orders[i] - 1) << OBATCH_SHIFT;
}

// ---- the histograms of orders 0 .. 3 per item: trc_planes_hist_obatch_dev ------------------------------------------------------------
extern "C" size_t trc_planes_hist_obatch_bytes(size_t item_count, unsigned esize)
{
    if (item_count == 0 || item_count > TRC_PLANES_BATCH_MAX) return 0;
    return item_count * trc_planes_hist_order_bytes(esize);
}

// the call behind its plan and range checks, as trc_planes_hist_batch_run (trc_planes_hist_batch.inc): items [first_item, first_item +
// item_count) of a batch that batch_plan has accepted, item_count >= 1; strides: those of the whole batch, vetted (NULL: 1).  Also
// what trc_planes_advise_obatch_dev (trc_planes_batch.inc) runs once per slab.
int trc_planes_hist_obatch_run(unsigned orders, const trc_planes_item *items, const uint8_t *strides, size_t first_item, size_t item_count,
                               unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "planes_hist_obatch";
    std::vector<BatchRec> recs;
    uint64_t chunks, elems;
    int rc = batch_range(who, items, first_item, item_count, esize, chunk, chunks, elems, &recs);
    if (rc) return rc;
    for (size_t i = 0; strides && i < item_count; i++) recs[i].v0 |= (uint64_t)(strides[first_item + i] - 1) << SBATCH_SHIFT;
    if (!d_hist || ((uintptr_t)d_hist & 7)) return trc_fail(TRC_E_ARG, "%s: the histograms must be 8-byte aligned", who);
    if ((rc = batch_table_args(who, trc_planes_batch_table_bytes(item_count, chunks), d_table, table_bytes))) return rc;
    const HistShape hs = hist_shape(orders, esize);
    unsigned grid = batch_grid((size_t)chunks * (chunk / TRC_PLANES_VEC));      // as trc_planes_hist_batch_run
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    if (grid > chunks) grid = (unsigned)chunks;
    const u32 nc = (u32)chunks, cpw = (nc + grid - 1) / grid;
    grid = (nc + cpw - 1) / cpw;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_obatch_bytes(item_count, esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
    const BatchRec *d_rec;
    const u32 *d_map;
    if ((rc = batch_table(who, recs, chunks, d_table, s, d_rec, d_map))) return rc;
    static void (*const kernels[3])(const BatchRec *, const u32 *, u32, u32, u32, u32, u32, u32, u64a *) = TRC_BY_ESIZE(trc_planes_hist_obatch_kernel);
    hipLaunchKernelGGL(kernels[esize_row(esize)], dim3(grid), dim3(TRC_PLANES_BLOCK), hs.lds, s, d_rec, d_map, nc, cpw, chunk, orders, hs.cshift, hs.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
}

extern "C" int trc_planes_hist_obatch_dev(unsigned orders, const trc_planes_item *items, const uint8_t *strides, size_t count,
                                          size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "planes_hist_obatch";
    int rc = batch_plan(who, items, count, esize, chunk, nullptr, nullptr);
    if (rc) return rc;
    if (orders < 1 || orders > 15) return trc_fail(TRC_E_ARG, "%s: orders 0x%x (a bit set: bit k = order k, 1 .. 15)", who, orders);
    if ((rc = trc_planes_batch_strides(who, nullptr, strides, count, nullptr))) return rc;
    if (first_item > count || item_count > count - first_item)
        return trc_fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    return trc_planes_hist_obatch_run(orders, items, strides, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream);
}
