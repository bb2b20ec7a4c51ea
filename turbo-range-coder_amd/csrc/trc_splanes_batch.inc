// trc_splanes_batch.inc -- the batched split, join and histograms of trc_planes_batch.hip (which includes this file behind
// trc_fplanes_batch.inc and trc_planes_hist_batch.inc) with a filter AND A STRIDE per item: the strided filters of trc_fplanes.hip,
// restarted at every chunk, where the stride is a run-time property of the item.
//
// Definition (include/trc_hip.h): GS(i) = item i where filters[i] == TRC_FILTER_NONE, else F_{strides[i]}(filters[i], seg = chunk,
// esize, item i); VS = V([GS(0) .. GS(count - 1)]).  Plan, pad, restart and read rules are those of the filtered batch.  A batch in
// which no filtered item has a stride above 1 never comes here: it launches the kernels of trc_fplanes_batch.inc.
//
// The stride travels in the item's record next to the filter id: stride - 1 in bits 56 .. 58 of v0 (v0 itself is below 2^44), so a
// record of stride 1 is the filtered batch's record bit for bit.  The host stores 1 for an item without a filter.
//
// Everything that depends on the stride is a body that is static in S (trc_planes_vec.h, trc_planes_scan.h), entered by a branch:
//   split      per thread: a vector never straddles a chunk, so it has one item, one filter and one stride.  Lanes diverge only where
//              a wave's 64 vectors cross items of different strides.
//   histogram  per workgroup: the item is workgroup-uniform there.
//   join       per WAVE, because the wave scan's shuffles need every lane: for each (filter, stride) that a ballot finds among the
//              tile's storing lanes, the scan of trc_fplanes_join_kernel<ESIZE, FILTER, S> -- static in both -- runs once with all
//              lanes active, and a lane keeps the result only where filter and stride are its own.  The segmented scan never combines
//              across a chunk and a chunk has one stride and one filter, so what the other lanes compute in a pass is junk that
//              nobody reads.  A tile is uniform whenever a chunk is at least a tile (chunk >= 512) or its chunks share filter and
//              stride: one pass.  Only 256 .. 448-element chunks, in 8-chunk spans, can need more.  (The filter as a per-lane
//              select inside eight passes, the form of fbatch_scan, was measured slower here: profiles/planes/sbatch_notes.md.)
//              The carry is kept per class across tiles as in trc_fplanes_join_kernel: 8 classes (4 packed pairs for 16-bit
//              elements) serve every stride, since a carry is taken only by lanes whose chunk began in an earlier tile -- the chunk
//              of that tile's lane 63 -- so a pass leaves its carry only where lane 63 has the pass's filter and stride.

#define SBATCH_SHIFT 56
#define SBATCH_V0(r) ((r).v0 & (((uint64_t)1 << 44) - 1))
#define SBATCH_STRIDE(r) ((((u32)((r).v0 >> SBATCH_SHIFT)) & 7u) + 1u)
#define SBATCH_EACH_STRIDE(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

// a whole vector's words under filter f (1 or 2) at stride S; lv = the vector's number in its item, front = it does not open a chunk
template <int ESIZE, int S> __device__ __forceinline__ void svec_fwd(u32 *w, u32 f, const uint8_t *__restrict__ in, size_t lv, bool front)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    T pe[TRC_PLANES_VEC];
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) pe[j] = 0;
    if (front) {
        if constexpr (S == 1) pe[TRC_PLANES_VEC - 1] = ((const EM *)in)[lv * TRC_PLANES_VEC - 1];
        else load_front<ESIZE, S>(in, lv, pe);
    }
    T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    unpack<ESIZE>(w, e);
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd_of<ESIZE>(f, e[j], j >= S ? e[j - S] : pe[TRC_PLANES_VEC - S + j]);
    pack<ESIZE>(y, w);
}

// planes, nv, M: as trc_planes_split_batch_kernel.  Reads [0, m * ESIZE) of every item, nothing else: the vector in front of a whole
// vector that does not open a chunk is a whole vector of the item; the item's last, partial vector is read element by element, each
// with the element S in front of it where its place in the chunk is at least S (so that element lies in the item).
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_splanes_split_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp,
                                    size_t nv, size_t M, uint8_t *__restrict__ planes, size_t pitch)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const u32 c = vec_chunk(v, vpc, rcp);
        const BatchRec r = rec[chunk_item[c]];
        const u32 f = FBATCH_FILTER(r), st = SBATCH_STRIDE(r);
        const size_t lv = v - SBATCH_V0(r), e = lv * TRC_PLANES_VEC, vb = v * TRC_PLANES_VEC;
        const u32 place = (u32)(v - (size_t)c * vpc) * TRC_PLANES_VEC;      // of the vector's first element in its chunk: 0 opens one
        const uint8_t *in = (const uint8_t *)r.ptr;
        const EM *el = (const EM *)in;
        uint8_t *dst = planes + vb;
        if (e + TRC_PLANES_VEC <= r.m) {
            const uint4 *src = (const uint4 *)(in + e * ESIZE);
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            if (f != TRC_FILTER_NONE) {
                switch (st) {
#define SB_CASE(S) case S: svec_fwd<ESIZE, S>(w, f, in, lv, place != 0); break;
                SBATCH_EACH_STRIDE(SB_CASE)
#undef SB_CASE
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
                    if (f != TRC_FILTER_NONE) y = fwd_of<ESIZE>(f, x, place + j >= st ? (T)el[e + j - st] : (T)0);
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
// one pass of a tile under filter FILTER at stride S, both static: the scan of trc_fplanes_join_kernel<ESIZE, FILTER, S> as it stands
// there.  e[] = the lane's 8 elements as joined from the planes -> the item's elements where `mine` (the lane stores and its item
// has this filter and this stride), unchanged elsewhere.  A lane is `mine` in one pass at most and scans with the lanes of its own
// chunk alone, which take the same pass: what a pass reads from lanes that an earlier pass has served reaches nobody.
// nin = the place of the lane's first element in its chunk, ahead = nin / 8.
// carry[]: class c of the running value where the previous tile ended (16-bit elements: classes 2c and 2c + 1 in one word; S = 1
// keeps its one value in carry[0] unpacked); where `commit` (wave-uniform), next[] <- the same where this tile ends.  The two are
// apart because a tile's passes all read the previous tile's carry, whichever of them leaves the next one.  Every lane of the wave
// calls this (shuffles).
template <int ESIZE, int FILTER, int S> __device__ __forceinline__ void sbatch_scan(typename Elem<ESIZE>::T *e, bool mine, bool commit,
                                                                                           u32 lane, u32 ahead, u32 nin, const typename Elem<ESIZE>::T *carry,
                                                                                           typename Elem<ESIZE>::T *next)
{
    typedef typename Elem<ESIZE>::T T;
    constexpr int V = TRC_PLANES_VEC;
    const u32 reach = ahead < lane ? ahead : lane;                       // lanes in front of this one in its chunk and in this tile
    T x[V];
    if constexpr (S == 1) {
        x[0] = operand<ESIZE, FILTER>(e[0]);
#pragma unroll
        for (int j = 1; j < V; j++) x[j] = op<FILTER>(x[j - 1], operand<ESIZE, FILTER>(e[j]));
        T inc = x[V - 1];
#pragma unroll
        for (u32 d = 1; d < 64; d <<= 1) {
            const T o = __shfl_up(inc, d);
            if (reach >= d) inc = op<FILTER>(inc, o);
        }
        T before = __shfl_up(inc, 1u);
        before = op<FILTER>(ahead > lane ? carry[0] : (T)0, reach ? before : (T)0);
#pragma unroll
        for (int j = 0; j < V; j++) x[j] = op<FILTER>(x[j], before);
        const T out = __shfl(x[V - 1], 63);
        if (commit) next[0] = out;
    } else {
        constexpr bool ROT = (V % S) != 0;                               // S divides 8: a lane's element j has class j % S
        constexpr int NP = ESIZE == 2 ? (S + 1) / 2 : S;
        const u32 r8 = ROT ? nin % (u32)S : 0u;                          // the class of the lane's first element
#pragma unroll
        for (int j = 0; j < V; j++) x[j] = operand<ESIZE, FILTER>(e[j]);
#pragma unroll
        for (int j = S; j < V; j++) x[j] = op<FILTER>(x[j], x[j - S]);
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
        for (int c = 0; c < NP; c++) run[c] = carry[c];
        if constexpr (ESIZE == 2) {                                      // two classes to a word: half the shuffles
            u32 pk[NP], pb[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) {
                constexpr int LAST = S - 1;
                const int hi = 2 * i + 1 < S ? 2 * i + 1 : LAST;         // (an odd S: the last word holds one class)
                pk[i] = (inc[2 * i] & 0xffffu) | (2 * i + 1 < S ? inc[hi] << 16 : 0u);
            }
            wave_scan<FILTER, NP, u32, true>(pk, run, pb, reach, ahead > lane);
#pragma unroll
            for (int c = 0; c < S; c++) before[c] = c & 1 ? pb[c / 2] >> 16 : pb[c / 2];
        } else wave_scan<FILTER, S, T, false>(inc, run, before, reach, ahead > lane);
        if (commit) {
#pragma unroll
            for (int c = 0; c < NP; c++) next[c] = run[c];
        }
        if constexpr (ROT) {
            T loc[S];
            rotate<S>(before, r8, loc);                                  // loc[i] = before[(r8 + i) % S]: element j takes loc[j % S]
#pragma unroll
            for (int j = 0; j < V; j++) x[j] = op<FILTER>(x[j], loc[j % S]);
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) x[j] = op<FILTER>(x[j], before[j % S]);
        }
    }
#pragma unroll
    for (int j = 0; j < V; j++) if (mine) e[j] = x[j];
}

// arguments, reads and writes: as trc_fplanes_join_batch_kernel, whose walk this is (keep the two alike)
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_splanes_join_batch_kernel(const uint8_t *__restrict__ planes, size_t pitch, const BatchRec *__restrict__ rec,
                                   const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp, size_t elems, u32 chunk, u32 span, size_t nspan)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    constexpr int NCARRY = ESIZE == 2 ? TRC_STRIDE_MAX / 2 : TRC_STRIDE_MAX;
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
        const u32 f = FBATCH_FILTER(r), st = SBATCH_STRIDE(r);
        const u32 st63 = __builtin_amdgcn_readlane(st, 63), f63 = __builtin_amdgcn_readlane(f, 63);      // whose carry the next tile's first chunk takes
        const bool scans = f != TRC_FILTER_NONE && cnt != 0;
        u32 w[NW];
        vec_join<ESIZE>(p, w);
        T e[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
        // a pass per distinct (filter, stride) among the lanes that scan and store; the ballot is wave-uniform, so every lane takes every pass
        T next[NCARRY];
#pragma unroll
        for (int c = 0; c < NCARRY; c++) next[c] = carry[c];
#define SB_PASS_F(F, S) { const bool mine = scans && st == S && f == F; \
                          if (__ballot(mine) != 0) sbatch_scan<ESIZE, F, S>(e, mine, st63 == S && f63 == F, lane, ahead, in_chunk, carry, next); }
#define SB_PASS(S) SB_PASS_F(TRC_FILTER_ZDELTA, S) SB_PASS_F(TRC_FILTER_XOR, S)
        SBATCH_EACH_STRIDE(SB_PASS)
#undef SB_PASS
#undef SB_PASS_F
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

// ---- the advisor's histograms ---------------------------------------------------------------------------------------------------
// one whole vector of an item at stride S: lv = its number in the item, front = it does not open a chunk
template <int ESIZE, int S> __device__ __forceinline__ void shist_vec(u32 *sm, const HistRows &R, u32 cshift, const uint8_t *__restrict__ in, size_t lv, bool front)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const uint4 *src = (const uint4 *)(in + lv * (TRC_PLANES_VEC * ESIZE));
    u32 w[NW];
#pragma unroll
    for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
    T pe[TRC_PLANES_VEC];
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) pe[j] = 0;
    if (front) {
        if constexpr (S == 1) pe[TRC_PLANES_VEC - 1] = ((const EM *)in)[lv * TRC_PLANES_VEC - 1];
        else load_front<ESIZE, S>(in, lv, pe);
    }
    count_filtered<ESIZE, S>(sm, R, cshift, w, pe);
}

// trc_planes_hist_batch_kernel with the item's stride: arguments, walk, flushes and reads are that kernel's (keep the two alike).
// The item, and so its stride, is the same in all lanes of the workgroup: a uniform branch into the static-S counting.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_sbatch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 nc, u32 cpw, u32 chunk,
                                   u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const HistRows R = hist_rows<ESIZE>(sm, filters, cshift);

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
        u64a *h = hist + (size_t)item * (TRC_PHIST_FILTERS * ESIZE * 256u);
        bool alone = c == first && c_end == first + nci;                 // the item is this run's alone, and not flushed yet
        u32 rr = tid % vpc, since = 0;                                   // the vector's place in its chunk (lv0 opens one): 0 opens one
        size_t lv = lv0 + tid;
        for (size_t it = 0; it < turns; it++, lv += TRC_PLANES_BLOCK) {
            if (lv < lv1) {
                const bool front = rr && (filters & 6u);
                switch (st) {
#define SB_CASE(S) case S: shist_vec<ESIZE, S>(sm, R, cshift, in, lv, front); break;
                SBATCH_EACH_STRIDE(SB_CASE)
#undef SB_CASE
                }
            }
            rr += rstep;
            if (rr >= vpc) rr -= vpc;
            if (++since == round_vecs && it + 1 < turns) { hist_flush<ESIZE>(sm, R, cshift, h, alone); alone = false; since = 0; }
        }
        // the elements behind the item's last whole vector (at most 7), one per lane, where the run holds the item's last chunk
        if (c_end == first + nci) {
            const u32 rest = (u32)(r.m - nvi * TRC_PLANES_VEC);
            if (tid < rest) {
                const size_t i = nvi * TRC_PLANES_VEC + tid;
                count_filtered_elem<ESIZE>(sm, R, cshift, (T)el[i], i % chunk >= st ? (T)el[i - st] : (T)0);
            }
        }
        hist_flush<ESIZE>(sm, R, cshift, h, alone);
        c = c_end;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// strides[0 .. count): every entry 1 .. TRC_STRIDE_MAX (host only; also the coded calls' check, trc_planes_batch.inc), looked at
// behind the filters.  *strided (may be NULL) <- whether an item with a filter has a stride above 1; strides == NULL is stride 1
int trc_planes_batch_strides(const char *who, const uint8_t *filters, const uint8_t *strides, size_t count, bool *strided)
{
    bool a = false;
    for (size_t i = 0; strides && i < count; i++) {
        if (strides[i] < 1 || strides[i] > TRC_STRIDE_MAX)
            return trc_fail(TRC_E_ARG, "%s: item %zu: stride %u (1 .. %d)", who, i, (unsigned)strides[i], TRC_STRIDE_MAX);
        a |= strides[i] > 1 && filters && filters[i] != TRC_FILTER_NONE;
    }
    if (strided) *strided = a;
    return TRC_OK;
}

// behind fbatch_pack: the strides of the items that have a filter
static void sbatch_pack(std::vector<BatchRec> &recs, const uint8_t *filters, const uint8_t *strides)
{
    for (size_t i = 0; i < recs.size(); i++)
        if (filters[i] != TRC_FILTER_NONE) recs[i].v0 |= (uint64_t)(strides[i] - 1) << SBATCH_SHIFT;
}
