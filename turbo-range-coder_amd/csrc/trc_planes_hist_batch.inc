// trc_planes_hist_batch.inc -- the planes advisor over a BATCH (included by trc_planes_batch.hip behind its kernels): the histograms
// of trc_planes_hist.hip, every plane under every requested filter, for every item of an item range from ONE launch, through the
// batch's pointer table.  Slice j of d_hist is what trc_planes_hist_dev writes for item first_item + j with seg = chunk.
//
// The counting is that of trc_planes_hist_kernel (trc_planes_count.h: the same LDS rows of replicated bins, the same adds, the same
// flush); what differs is who counts what.  A workgroup's LDS counters can belong to one item at a time, and a grid-stride loop over the vectors
// of the virtual buffer would mix items within a turn.  So workgroup b owns the contiguous chunk run [b * cpw, (b + 1) * cpw) of the
// range and walks it item by item: chunk_item[c] names the item of the run's next chunk, all 256 threads count the item's vectors
// that lie in the run, the counters are flushed to that item's global rows (one 64-bit atomicAdd per non-zero bin, bins rotated by
// the workgroup's number), and the walk goes on behind the item's last chunk.  A long item is shared by several workgroups, whose
// atomics merge; a run of short items costs one flush -- a scan of all the LDS rows -- per item.  Where the run holds ALL of an item's
// chunks and the flush is the item's only one, nobody else adds to those rows (the host has zeroed them): the sums are STORED, a
// whole row at a time.  That is every item of a batch of short items, whose 3 * ESIZE * 256 counters per item -- 24 KiB for the 4 KiB of a
// 1024-element fp32 item -- would otherwise arrive at the rate of the device's atomics (profiles/planes/abatch_notes.md).
//
// READS: bytes [0, m * ESIZE) of an item and nothing else.  Only whole vectors (8 * lv + 8 <= m) are loaded as 16-byte words; the
// element in front of a vector is asked for only where the vector does not open a chunk, so it is not the item's first; the item's
// last m % 8 elements go one per lane, each with the element in front of it.  The pad behind an item has no vector here: the loop
// ends at the item's last whole vector, so pad elements are counted nowhere.

// nc chunks in the range, cpw of them per workgroup (gridDim.x * cpw >= nc).  hist: 3 * ESIZE * 256 counters per record of rec[],
// zero on entry.  Dynamic LDS: (requested filters * ESIZE * 256 * 4) << cshift bytes.  round_vecs >= 1.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 nc, u32 cpw, u32 chunk,
                                  u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const HistRows R = hist_rows<ESIZE>(sm, filters, cshift);

    const u32 vpc = chunk / TRC_PLANES_VEC, rstep = TRC_PLANES_BLOCK % vpc;
    const u32 c_lo = blockIdx.x * cpw, c_hi = nc - c_lo < cpw ? nc : c_lo + cpw;      // (the host: c_lo < nc)
    for (u32 c = c_lo; c < c_hi; ) {
        // everything that shapes the walk is the same in all lanes: the item, its record, the turns of the loop (the flush holds barriers)
        const u32 item = __builtin_amdgcn_readfirstlane(chunk_item[c]);
        const BatchRec r = rec[item];
        const u32 first = (u32)r.first, nci = (u32)((r.m + chunk - 1) / chunk);
        const u32 c_end = first + nci < c_hi ? first + nci : c_hi;       // the run's part of the item: chunks [c, c_end)
        const size_t nvi = r.m / TRC_PLANES_VEC;                         // the item's whole vectors
        const size_t lv0 = (size_t)(c - first) * vpc, lv_run = (size_t)(c_end - first) * vpc, lv1 = lv_run < nvi ? lv_run : nvi;
        const size_t turns = lv1 > lv0 ? (lv1 - lv0 + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK : 0;
        const uint8_t *in = (const uint8_t *)r.ptr;
        const M *el = (const M *)in;
        u64a *h = hist + (size_t)item * (TRC_PHIST_FILTERS * ESIZE * 256u);
        bool alone = c == first && c_end == first + nci;                 // the item is this run's alone, and not flushed yet
        u32 rr = tid % vpc, since = 0;                                   // the vector's place in its chunk (lv0 opens one): 0 opens one
        size_t lv = lv0 + tid;
        for (size_t it = 0; it < turns; it++, lv += TRC_PLANES_BLOCK) {
            if (lv < lv1) {
                const uint4 *src = (const uint4 *)(in + lv * (TRC_PLANES_VEC * ESIZE));
                u32 w[NW];
#pragma unroll
                for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
                T pe[TRC_PLANES_VEC];
#pragma unroll
                for (int j = 0; j < TRC_PLANES_VEC; j++) pe[j] = 0;
                if (rr && (filters & 6u)) pe[TRC_PLANES_VEC - 1] = el[lv * TRC_PLANES_VEC - 1];
                count_filtered<ESIZE, 1>(sm, R, cshift, w, pe);
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
                count_filtered_elem<ESIZE>(sm, R, cshift, (T)el[i], i % chunk ? (T)el[i - 1] : (T)0);
            }
        }
        hist_flush<ESIZE>(sm, R, cshift, h, alone);
        c = c_end;
    }
}

extern "C" size_t trc_planes_hist_batch_bytes(size_t item_count, unsigned esize)
{
    if (item_count > TRC_PLANES_BATCH_MAX) return 0;
    return item_count * trc_planes_hist_bytes(esize);
}

// the call behind its plan and range checks: items [first_item, first_item + item_count) of a batch that batch_plan has accepted,
// item_count >= 1.  Also what trc_planes_advise_batch_dev (trc_planes_batch.inc) runs once per slab.  strides: those of the whole
// batch, vetted (NULL: 1); where a predicted row is counted and a requested item's stride is above 1, every item is counted against
// the element strides[i] back by trc_planes_hist_sbatch_kernel (trc_splanes_batch.inc), else by the kernel above.
int trc_planes_hist_batch_run(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t first_item, size_t item_count,
                              unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    bool strided = false;
    for (size_t i = 0; strides && (filters & 6u) && i < item_count; i++) strided |= strides[first_item + i] > 1;
    const char *who = strided ? "planes_hist_sbatch" : "planes_hist_batch";
    std::vector<BatchRec> recs;
    uint64_t chunks, elems;
    int rc = batch_range(who, items, first_item, item_count, esize, chunk, chunks, elems, &recs);
    if (rc) return rc;
    if (strided)
        for (size_t i = 0; i < item_count; i++) recs[i].v0 |= (uint64_t)(strides[first_item + i] - 1) << SBATCH_SHIFT;
    if (!d_hist || ((uintptr_t)d_hist & 7)) return trc_fail(TRC_E_ARG, "%s: the histograms must be 8-byte aligned", who);
    if ((rc = batch_table_args(who, trc_planes_batch_table_bytes(item_count, chunks), d_table, table_bytes))) return rc;
    const HistShape hs = hist_shape(filters, esize);
    // a workgroup per 256 vectors of the range under the caps of trc_planes_hist_dev, then whole chunks per workgroup
    unsigned grid = batch_grid((size_t)chunks * (chunk / TRC_PLANES_VEC));
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    if (grid > chunks) grid = (unsigned)chunks;
    const u32 nc = (u32)chunks, cpw = (nc + grid - 1) / grid;
    grid = (nc + cpw - 1) / cpw;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_batch_bytes(item_count, esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
    const BatchRec *d_rec;
    const u32 *d_map;
    if ((rc = batch_table(who, recs, chunks, d_table, s, d_rec, d_map))) return rc;
    static void (*const kernels[2][3])(const BatchRec *, const u32 *, u32, u32, u32, u32, u32, u32, u64a *) =
        { TRC_BY_ESIZE(trc_planes_hist_batch_kernel), TRC_BY_ESIZE(trc_planes_hist_sbatch_kernel) };       // [a stride above 1][esize_row]
    hipLaunchKernelGGL(kernels[strided][esize_row(esize)], dim3(grid), dim3(TRC_PLANES_BLOCK), hs.lds, s, d_rec, d_map, nc, cpw, chunk, filters, hs.cshift, hs.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
}

// both calls: strides == NULL is trc_planes_hist_batch_dev
static int hist_batch(const char *who, unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count,
                      size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                      uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    int rc = batch_plan(who, items, count, esize, chunk, nullptr, nullptr);
    if (rc) return rc;
    if (filters < 1 || filters > 7) return trc_fail(TRC_E_ARG, "%s: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", who, filters);
    if ((rc = trc_planes_batch_strides(who, nullptr, strides, count, nullptr))) return rc;
    if (first_item > count || item_count > count - first_item)
        return trc_fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    return trc_planes_hist_batch_run(filters, items, strides, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream);
}

extern "C" int trc_planes_hist_batch_dev(unsigned filters, const trc_planes_item *items, size_t count,
                                         size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                         uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    return hist_batch("planes_hist_batch", filters, items, nullptr, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream);
}
extern "C" int trc_planes_hist_sbatch_dev(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count,
                                          size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    return hist_batch("planes_hist_sbatch", filters, items, strides, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream);
}

// ---- the histograms of a batch against a BASE per item: trc_planes_hist_bbatch_dev -----------------------------------------------
// The walk of trc_planes_hist_batch_kernel with the second load stream of trc_bplanes_hist_kernel (trc_bplanes.hip): the predictor
// of element e of an item is element e of its base, so there is no element-in-front load, no restart and no seg; slice j is what
// trc_planes_hist_base_dev writes for item first_item + j and its base alone.  The base's address travels in the record's v0, which
// this walk does not need (a run is cut by chunks, not by vectors of V), so the table is the plain batch's.  An item WITHOUT a base
// (address 0) is counted under the unfiltered row only: rows 1 and 2 of its slice stay zero.
// READS: bytes [0, m * ESIZE) of an item and of its base, nothing else: whole vectors as 16-byte words, both streams issued before
// the first use, the last m % 8 elements one per lane.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_hist_bbatch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 nc, u32 cpw, u32 chunk,
                                   u32 filters, u32 cshift, u32 round_vecs, u64a *__restrict__ hist)
{
    typedef typename Elem<ESIZE>::T T;
    typedef typename Elem<ESIZE>::M M;
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    const u32 tid = threadIdx.x;
    const HistRows R = hist_rows<ESIZE>(sm, filters, cshift);

    const u32 vpc = chunk / TRC_PLANES_VEC;
    const u32 c_lo = blockIdx.x * cpw, c_hi = nc - c_lo < cpw ? nc : c_lo + cpw;      // (the host: c_lo < nc)
    for (u32 c = c_lo; c < c_hi; ) {
        const u32 item = __builtin_amdgcn_readfirstlane(chunk_item[c]);
        const BatchRec r = rec[item];
        const u32 first = (u32)r.first, nci = (u32)((r.m + chunk - 1) / chunk);
        const u32 c_end = first + nci < c_hi ? first + nci : c_hi;       // the run's part of the item: chunks [c, c_end)
        const size_t nvi = r.m / TRC_PLANES_VEC;
        const size_t lv0 = (size_t)(c - first) * vpc, lv_run = (size_t)(c_end - first) * vpc, lv1 = lv_run < nvi ? lv_run : nvi;
        const uint8_t *in = (const uint8_t *)r.ptr, *bp = (const uint8_t *)r.v0;      // (v0: the base, 0 where the item has none)
        const bool pred = bp && (filters & 6u);
        HistRows Ri = R;                           // the rows this item counts into; the flush walks all of R's, the others being zero
        if (!bp) Ri.with_z = Ri.with_x = false;
        const size_t turns = (Ri.with_n || pred) && lv1 > lv0 ? (lv1 - lv0 + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK : 0;
        u64a *h = hist + (size_t)item * (TRC_PHIST_FILTERS * ESIZE * 256u);
        bool alone = c == first && c_end == first + nci;                 // the item is this run's alone, and not flushed yet
        u32 since = 0;
        size_t lv = lv0 + tid;
        for (size_t it = 0; it < turns; it++, lv += TRC_PLANES_BLOCK) {
            if (lv < lv1) {
                const uint4 *src = (const uint4 *)(in + lv * (TRC_PLANES_VEC * ESIZE)), *bsrc = (const uint4 *)(bp + lv * (TRC_PLANES_VEC * ESIZE));
                uint4 xq[NQ], bq[NQ];
#pragma unroll
                for (int q = 0; q < NQ; q++) { xq[q] = src[q]; bq[q] = make_uint4(0u, 0u, 0u, 0u); }
                if (pred) {
#pragma unroll
                    for (int q = 0; q < NQ; q++) bq[q] = bsrc[q];
                }
                u32 w[NW], bw[NW];
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    w[4 * q] = xq[q].x; w[4 * q + 1] = xq[q].y; w[4 * q + 2] = xq[q].z; w[4 * q + 3] = xq[q].w;
                    bw[4 * q] = bq[q].x; bw[4 * q + 1] = bq[q].y; bw[4 * q + 2] = bq[q].z; bw[4 * q + 3] = bq[q].w;
                }
                T b[TRC_PLANES_VEC];
                unpack<ESIZE>(bw, b);
                count_predicted<ESIZE>(sm, Ri, cshift, w, b);
            }
            if (++since == round_vecs && it + 1 < turns) { hist_flush<ESIZE>(sm, R, cshift, h, alone); alone = false; since = 0; }
        }
        // the elements behind the item's last whole vector (at most 7), one per lane, where the run holds the item's last chunk
        if (c_end == first + nci && (Ri.with_n || pred)) {
            const u32 rest = (u32)(r.m - nvi * TRC_PLANES_VEC);
            if (tid < rest) {
                const size_t i = nvi * TRC_PLANES_VEC + tid;
                count_filtered_elem<ESIZE>(sm, Ri, cshift, (T)((const M *)in)[i], pred ? (T)((const M *)bp)[i] : (T)0);
            }
        }
        hist_flush<ESIZE>(sm, R, cshift, h, alone);
        c = c_end;
    }
}

// the bases of items [first_item, first_item + item_count) for the histograms: NULL (no base: the unfiltered row only) or 16-byte aligned
static int hist_bbatch_bases(const char *who, const void *const *bases, size_t first_item, size_t item_count)
{
    for (size_t i = first_item; bases && i < first_item + item_count; i++)
        if ((uintptr_t)bases[i] & 15) return trc_fail(TRC_E_ARG, "%s: item %zu: the base must be 16-byte aligned (or NULL: no base)", who, i);
    return TRC_OK;
}

// the call behind its plan and range checks, as trc_planes_hist_batch_run; also what trc_planes_advise_bbatch_dev runs once per slab
int trc_planes_hist_bbatch_run(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t first_item, size_t item_count,
                               unsigned esize, uint32_t chunk, uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "planes_hist_bbatch";
    std::vector<BatchRec> recs;
    uint64_t chunks, elems;
    int rc = batch_range(who, items, first_item, item_count, esize, chunk, chunks, elems, &recs);
    if (rc) return rc;
    if ((rc = hist_bbatch_bases(who, bases, first_item, item_count))) return rc;
    for (size_t i = 0; i < item_count; i++) recs[i].v0 = bases ? (uint64_t)(uintptr_t)bases[first_item + i] : 0;
    if (!d_hist || ((uintptr_t)d_hist & 7)) return trc_fail(TRC_E_ARG, "%s: the histograms must be 8-byte aligned", who);
    if ((rc = batch_table_args(who, trc_planes_batch_table_bytes(item_count, chunks), d_table, table_bytes))) return rc;
    const HistShape hs = hist_shape(filters, esize);
    unsigned grid = batch_grid((size_t)chunks * (chunk / TRC_PLANES_VEC));      // as trc_planes_hist_batch_run
    if (grid > TRC_PHIST_GRID_MAX) grid = TRC_PHIST_GRID_MAX;
    if (grid > chunks) grid = (unsigned)chunks;
    const u32 nc = (u32)chunks, cpw = (nc + grid - 1) / grid;
    grid = (nc + cpw - 1) / cpw;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = hipMemsetAsync(d_hist, 0, trc_planes_hist_batch_bytes(item_count, esize), s);
    if (he != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
    const BatchRec *d_rec;
    const u32 *d_map;
    if ((rc = batch_table(who, recs, chunks, d_table, s, d_rec, d_map))) return rc;
    static void (*const kernels[3])(const BatchRec *, const u32 *, u32, u32, u32, u32, u32, u32, u64a *) = TRC_BY_ESIZE(trc_planes_hist_bbatch_kernel);
    hipLaunchKernelGGL(kernels[esize_row(esize)], dim3(grid), dim3(TRC_PLANES_BLOCK), hs.lds, s, d_rec, d_map, nc, cpw, chunk, filters, hs.cshift, hs.round_vecs, (u64a *)d_hist);
    he = hipGetLastError();
    return he == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(he));
}

extern "C" int trc_planes_hist_bbatch_dev(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t count,
                                          size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "planes_hist_bbatch";
    int rc = batch_plan(who, items, count, esize, chunk, nullptr, nullptr);
    if (rc) return rc;
    if (filters < 1 || filters > 7) return trc_fail(TRC_E_ARG, "%s: filters 0x%x (a bit set of filter ids: 1 none, 2 zigzag delta, 4 xor)", who, filters);
    if (first_item > count || item_count > count - first_item)
        return trc_fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    return trc_planes_hist_bbatch_run(filters, items, bases, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream);
}
