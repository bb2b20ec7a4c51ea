// trc_fplanes_batch.inc -- the batched split and join of trc_planes_batch.hip (which includes this file behind its own kernels) with
// a predictor filter PER ITEM in front of the planes: the filters of trc_fplanes.hip, restarted at every chunk.
//
// Definition (include/trc_hip.h): G(i) = item i where filters[i] == TRC_FILTER_NONE, else F(filters[i], seg = chunk, esize, item i);
// VF = V([G(0) .. G(count - 1)]).  Every item is filtered as if it stood alone -- items start on chunk boundaries and the predictor
// restarts at every chunk, so no item sees its neighbour -- and the pad behind an item stays zero bytes in every plane.
//
// The filter id travels in the item's record, in the two top bits of v0 (the item's first vector, below 2^44: at most 2^31 chunks of
// at most 2^13 vectors).  `first` has room as well, but the map kernel compares it as 64 bits and serves here as it stands.
//
// Split = trc_planes_split_batch_kernel + the forward step of trc_fplanes_split_kernel: the one element a thread lacks is the one in
// front of its vector, in the same item unless the vector opens a chunk.  Join = the scanning join of trc_fplanes_join_kernel at
// stride 1 (trc_planes_scan.h: one wave per span of V, tiles of 512 elements, the next tile's loads in flight while this one is
// scanned, a segmented wave scan, the carry of lane 63; the walk stands here as in that kernel -- keep the two alike) with the map of
// the batch kernels behind the scan: a lane finds its item only to know which operation it scans with, how much of its vector it
// stores and where.  A span of 8 short chunks may cross items of different filters; the segmented scan never combines across a chunk
// and a chunk has one filter, so the operation is the lane's own (selects: a scan per filter, taken where a tile's lanes agree,
// measured no faster -- profiles/planes/fbatch_notes.md).

#define FBATCH_SHIFT 62
#define FBATCH_V0(r) ((r).v0 & (((uint64_t)1 << FBATCH_SHIFT) - 1))
#define FBATCH_FILTER(r) ((u32)((r).v0 >> FBATCH_SHIFT))

// the forward step under a filter known at run time (1 or 2)
template <int ESIZE> __device__ __forceinline__ typename Elem<ESIZE>::T fwd_of(u32 f, typename Elem<ESIZE>::T x, typename Elem<ESIZE>::T p)
{
    return f == TRC_FILTER_XOR ? fwd<ESIZE, TRC_FILTER_XOR>(x, p) : fwd<ESIZE, TRC_FILTER_ZDELTA>(x, p);
}

// a whole vector's words under filter FILTER; prev = the element in front of it (0 where it opens a chunk)
template <int ESIZE, int FILTER> __device__ __forceinline__ void vec_fwd(u32 *w, typename Elem<ESIZE>::T prev)
{
    typedef typename Elem<ESIZE>::T T;
    T e[TRC_PLANES_VEC], y[TRC_PLANES_VEC];
    unpack<ESIZE>(w, e);
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) y[j] = fwd<ESIZE, FILTER>(e[j], j ? e[j - 1] : prev);
    pack<ESIZE>(y, w);
}

// planes, nv, M: as trc_planes_split_batch_kernel.  Reads [0, m * ESIZE) of every item, nothing else: the element in front of a
// vector lies in the item (the vector does not open a chunk, so it is not the item's first), the item's last, partial vector is read
// element by element.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_split_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp,
                                    size_t nv, size_t M, uint8_t *__restrict__ planes, size_t pitch)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const u32 c = vec_chunk(v, vpc, rcp);
        const BatchRec r = rec[chunk_item[c]];
        const u32 f = FBATCH_FILTER(r);
        const size_t e = (v - FBATCH_V0(r)) * TRC_PLANES_VEC, vb = v * TRC_PLANES_VEC;
        const bool opens = v == (size_t)c * vpc;   // the vector opens a chunk: its first element has no predecessor
        const EM *el = (const EM *)r.ptr;
        uint8_t *dst = planes + vb;
        T prev = 0;                                // (asked for ahead of the vector's own loads, so that they travel together)
        if (f != TRC_FILTER_NONE && !opens && e < r.m) prev = el[e - 1];
        if (e + TRC_PLANES_VEC <= r.m) {
            const uint4 *src = (const uint4 *)(r.ptr + e * ESIZE);
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            if (f != TRC_FILTER_NONE) {
                if (f == TRC_FILTER_ZDELTA) vec_fwd<ESIZE, TRC_FILTER_ZDELTA>(w, prev);
                else vec_fwd<ESIZE, TRC_FILTER_XOR>(w, prev);
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
                    y = f == TRC_FILTER_NONE ? x : fwd_of<ESIZE>(f, x, prev);
                    prev = x;
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

// operand and operation of the scan under the lane's own filter f (bits above a 16-bit element's width are junk from the operand on;
// pack drops them).  NONE: the operand is the element, and the caller keeps what the scan makes of it out of the lane's elements.
template <typename T> __device__ __forceinline__ T operand_of(u32 f, T y) { return f == TRC_FILTER_ZDELTA ? (y >> 1) ^ ((T)0 - (y & 1)) : y; }
template <typename T> __device__ __forceinline__ T op_of(u32 f, T a, T b) { return f == TRC_FILTER_XOR ? a ^ b : a + b; }

// one tile of the join: the lane's 8 elements e[] (as joined from the planes) -> the item's elements, and the carry for the next
// tile.  ahead = lanes' worth of elements in front of this lane in its chunk.  Every lane of the wave calls this (shuffles).
template <int ESIZE> __device__ __forceinline__ void fbatch_scan(typename Elem<ESIZE>::T *e, u32 f, u32 lane, u32 ahead,
                                                                         typename Elem<ESIZE>::T &carry)
{
    typedef typename Elem<ESIZE>::T T;
    const bool scans = f != TRC_FILTER_NONE;
    T x[TRC_PLANES_VEC];
    x[0] = operand_of(f, e[0]);
#pragma unroll
    for (int j = 1; j < TRC_PLANES_VEC; j++) x[j] = op_of(f, x[j - 1], operand_of(f, e[j]));
    const u32 reach = ahead < lane ? ahead : lane;
    T inc = x[TRC_PLANES_VEC - 1];
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d);
        if (reach >= d) inc = op_of(f, inc, o);
    }
    T before = __shfl_up(inc, 1u);
    before = op_of(f, ahead > lane ? carry : (T)0, reach ? before : (T)0);
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) { x[j] = op_of(f, x[j], before); if (scans) e[j] = x[j]; }
    carry = __shfl(e[TRC_PLANES_VEC - 1], 63);
}

// planes: 64-byte aligned, element 0 = the first requested item's first; elems = the elements of the range (its last item unpadded),
// span = chunk, or 8 * chunk where a chunk is shorter than a tile; nspan = ceil(elems / span).  Reads [0, elems) of every plane,
// writes [0, m * ESIZE) of every item in rec[], nothing else.  What a lane loads from an item's pad, or behind the item's last element
// in its partial vector, lies behind every element of the item in that chunk: it reaches the lane's own later elements, later lanes
// of the chunk and the carry into the chunk's later tiles -- pad all of them, none of it stored.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_fplanes_join_batch_kernel(const uint8_t *__restrict__ planes, size_t pitch, const BatchRec *__restrict__ rec,
                                   const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp, size_t elems, u32 chunk, u32 span, size_t nspan)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
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
    T carry = 0;
    for (;;) {
        uint2 p[ESIZE];
#pragma unroll
        for (int k = 0; k < ESIZE; k++) p[k] = pn[k];
        const BatchRec r = rn;
        const size_t base = nbase;
        const u32 ahead = nin / TRC_PLANES_VEC;
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
        const size_t eo = (base / TRC_PLANES_VEC - FBATCH_V0(r)) * TRC_PLANES_VEC;
        const u32 cnt = eo + TRC_PLANES_VEC <= r.m ? TRC_PLANES_VEC : eo < r.m ? (u32)(r.m - eo) : 0;
        const u32 f = FBATCH_FILTER(r);
        u32 w[NW];
        vec_join<ESIZE>(p, w);
        T e[TRC_PLANES_VEC];
        unpack<ESIZE>(w, e);
        fbatch_scan<ESIZE>(e, f, lane, ahead, carry);
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

// ---- host ------------------------------------------------------------------------------------------------------------------------
// filters[0 .. count): every entry 0, 1 or 2 (host only; also the coded calls' check, trc_planes_batch.inc).  *any (may be NULL)
// <- whether one of them is not TRC_FILTER_NONE; filters == NULL is a batch without filters
int trc_planes_batch_filters(const char *who, const uint8_t *filters, size_t count, bool *any)
{
    bool a = false;
    for (size_t i = 0; filters && i < count; i++) {
        if (filters[i] > TRC_FILTER_XOR) return trc_fail(TRC_E_ARG, "%s: item %zu: filter %u (0 none, 1 zigzag delta, 2 xor)", who, i, (unsigned)filters[i]);
        a |= filters[i] != TRC_FILTER_NONE;
    }
    if (any) *any = a;
    return TRC_OK;
}

static void fbatch_pack(std::vector<BatchRec> &recs, const uint8_t *filters)
{
    for (size_t i = 0; i < recs.size(); i++) recs[i].v0 |= (uint64_t)filters[i] << FBATCH_SHIFT;
}
