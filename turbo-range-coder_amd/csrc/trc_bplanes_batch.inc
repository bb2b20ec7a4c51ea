// trc_bplanes_batch.inc -- the batched split and join of trc_planes_batch.hip (which includes this file behind trc_fplanes_batch.inc)
// with a filter against a BASE per item: the filters of trc_bplanes.hip, item i against bases[i].
//
// Definition (include/trc_hip.h): G(i) = item i where filters[i] == TRC_FILTER_NONE (bases[i] is not looked at), else
// D(filters[i], esize, item i, bases[i]); VD = V([G(0) .. G(count - 1)]); the pad behind an item stays zero bytes in every plane.
//
// The filter id travels where fbatch_pack puts it (the two top bits of the record's v0), the base pointers in a uint64 array of one
// entry per item behind the chunk map, so BatchRec stays 32 bytes.  Element i depends on element i of the base only, so the join is
// elementwise: it has the shape of trc_planes_join_batch_kernel, not of the scanning trc_fplanes_join_batch_kernel.  A base may be
// the item itself on the way back (in place): a thread has its base vector in registers before it stores to those addresses.
// READS of a base: [0, n[i]) and nothing else -- whole vectors as 16-byte words, the last partial vector element by element.

template <int ESIZE> __device__ __forceinline__ typename Elem<ESIZE>::T inv_of(u32 f, typename Elem<ESIZE>::T y, typename Elem<ESIZE>::T p)
{
    return f == TRC_FILTER_XOR ? inv<ESIZE, TRC_FILTER_XOR>(y, p) : inv<ESIZE, TRC_FILTER_ZDELTA>(y, p);
}

// a whole vector's words w against the base's words bw, forwards or backwards, under the filter f known at run time (1 or 2)
template <int ESIZE, bool FWD> __device__ __forceinline__ void vec_vs_base(u32 f, u32 *w, const uint4 *bq)
{
    typedef typename Elem<ESIZE>::T T;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    u32 bw[NW];
#pragma unroll
    for (int q = 0; q < NQ; q++) { bw[4 * q] = bq[q].x; bw[4 * q + 1] = bq[q].y; bw[4 * q + 2] = bq[q].z; bw[4 * q + 3] = bq[q].w; }
    T e[TRC_PLANES_VEC], b[TRC_PLANES_VEC];
    unpack<ESIZE>(w, e);
    unpack<ESIZE>(bw, b);
#pragma unroll
    for (int j = 0; j < TRC_PLANES_VEC; j++) e[j] = FWD ? fwd_of<ESIZE>(f, e[j], b[j]) : inv_of<ESIZE>(f, e[j], b[j]);
    pack<ESIZE>(e, w);
}

// planes, nv, M: as trc_planes_split_batch_kernel.  base[i] = the base of item i (not looked at where the item's filter is NONE).
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_bplanes_split_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, const uint64_t *__restrict__ base,
                                    u32 vpc, u32 rcp, size_t nv, size_t M, uint8_t *__restrict__ planes, size_t pitch)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const u32 it = chunk_item[vec_chunk(v, vpc, rcp)];
        const BatchRec r = rec[it];
        const u32 f = FBATCH_FILTER(r);
        const size_t e = (v - FBATCH_V0(r)) * TRC_PLANES_VEC, vb = v * TRC_PLANES_VEC;
        uint8_t *dst = planes + vb;
        if (e + TRC_PLANES_VEC <= r.m) {
            const uint4 *src = (const uint4 *)(r.ptr + e * ESIZE);
            uint4 xq[NQ], bq[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) xq[q] = src[q];
            if (f != TRC_FILTER_NONE) {
                const uint4 *bsrc = (const uint4 *)(base[it] + e * ESIZE);
#pragma unroll
                for (int q = 0; q < NQ; q++) bq[q] = bsrc[q];
            }
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { w[4 * q] = xq[q].x; w[4 * q + 1] = xq[q].y; w[4 * q + 2] = xq[q].z; w[4 * q + 3] = xq[q].w; }
            if (f != TRC_FILTER_NONE) vec_vs_base<ESIZE, true>(f, w, bq);
            uint2 p[ESIZE];
            vec_split<ESIZE>(w, p);
#pragma unroll
            for (int k = 0; k < ESIZE; k++) *(uint2 *)(dst + k * pitch) = p[k];
        } else if (e < r.m) {                      // the item's last vector: rest of its elements, then zeros as split_rest
            const u32 rest = (u32)(r.m - e), lim = vb + TRC_PLANES_VEC <= M ? TRC_PLANES_VEC : rest;
            const EM *el = (const EM *)r.ptr, *bel = (const EM *)(f != TRC_FILTER_NONE ? base[it] : r.ptr);
#pragma unroll 1
            for (u32 j = 0; j < lim; j++) {
                T y = 0;
                if (j < rest) {
                    const T x = el[e + j];
                    y = f == TRC_FILTER_NONE ? x : fwd_of<ESIZE>(f, x, (T)bel[e + j]);
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

// the mirror image over the chunks of the requested items, as trc_planes_join_batch_kernel: writes [0, m * ESIZE) of every item in
// rec[], nothing else.  base[i] counts from the first requested item and may be the item's own address.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_bplanes_join_batch_kernel(const uint8_t *__restrict__ planes, size_t pitch, const BatchRec *__restrict__ rec,
                                   const u32 *__restrict__ chunk_item, const uint64_t *__restrict__ base, u32 vpc, u32 rcp, size_t nv)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M EM;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const u32 it = chunk_item[vec_chunk(v, vpc, rcp)];
        const BatchRec r = rec[it];
        const u32 f = FBATCH_FILTER(r);
        const size_t e = (v - FBATCH_V0(r)) * TRC_PLANES_VEC;
        const uint8_t *src = planes + v * TRC_PLANES_VEC;
        if (e + TRC_PLANES_VEC <= r.m) {
            uint2 p[ESIZE];
            uint4 bq[NQ];
#pragma unroll
            for (int k = 0; k < ESIZE; k++) p[k] = *(const uint2 *)(src + k * pitch);
            if (f != TRC_FILTER_NONE) {
                const uint4 *bsrc = (const uint4 *)(base[it] + e * ESIZE);
#pragma unroll
                for (int q = 0; q < NQ; q++) bq[q] = bsrc[q];
            }
            u32 w[NW];
            vec_join<ESIZE>(p, w);
            if (f != TRC_FILTER_NONE) vec_vs_base<ESIZE, false>(f, w, bq);
            uint4 *dst = (uint4 *)(r.ptr + e * ESIZE);
#pragma unroll
            for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        } else if (e < r.m) {
            const u32 rest = (u32)(r.m - e);
            EM *el = (EM *)r.ptr;
            const EM *bel = (const EM *)(f != TRC_FILTER_NONE ? base[it] : r.ptr);
#pragma unroll 1
            for (u32 j = 0; j < rest; j++) {
                T y = 0;
#pragma unroll
                for (int k = 0; k < ESIZE; k++) y |= (T)src[k * pitch + j] << (8 * k);
                el[e + j] = (EM)(f == TRC_FILTER_NONE ? y : inv_of<ESIZE>(f, y, (T)bel[e + j]));
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the batch table with the base pointers behind the chunk map
extern "C" size_t trc_planes_bbatch_table_bytes(size_t count, uint64_t chunks)
{
    return batch_pred_table_bytes(BATCH_PRED_BASED, count, chunks);
}

// the bases of items [first_item, first_item + item_count) whose filter is 1 or 2 (also the coded calls' check, trc_bplanes.inc)
int trc_planes_bbatch_bases(const char *who, const void *const *bases, const uint8_t *filters, size_t first_item, size_t item_count)
{
    for (size_t i = first_item; filters && i < first_item + item_count; i++)
        if (filters[i] != TRC_FILTER_NONE && (!bases || !bases[i] || ((uintptr_t)bases[i] & 15)))
            return trc_fail(TRC_E_ARG, "%s: item %zu: a filter against a base needs the base, 16-byte aligned", who, i);
    return TRC_OK;
}

// the base pointers of a range to the table, behind the map (the host array is free again when this returns)
static int bbatch_bases_up(const char *who, const void *const *bases, const uint8_t *filters, size_t first_item, size_t item_count, uint64_t chunks,
                           void *d_table, hipStream_t s, const uint64_t *&d_base)
{
    std::vector<uint64_t> b(item_count);
    for (size_t i = 0; i < item_count; i++) b[i] = filters[first_item + i] != TRC_FILTER_NONE ? (uint64_t)(uintptr_t)bases[first_item + i] : 0;
    uint8_t *at = (uint8_t *)d_table + trc_planes_batch_table_bytes(item_count, chunks);
    const hipError_t e = hipMemcpyWithStream(at, b.data(), item_count * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return trc_fail(TRC_E_HIP, "%s: base table upload: %s", who, hipGetErrorString(e));
    d_base = (const uint64_t *)at;
    return TRC_OK;
}
