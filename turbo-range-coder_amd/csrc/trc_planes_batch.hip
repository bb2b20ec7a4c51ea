// trc_planes_batch.hip -- byte planes of MANY separate allocations (tensors of a checkpoint, pages of a cache, columns of a table):
// a split that gathers from a pointer table into one long plane per byte position, the join that scatters back, and the plan; behind
// them the same with a filter per item (trc_fplanes_batch.inc), with a filter and a stride per item (trc_splanes_batch.inc), with a
// predictor order per item as well (trc_oplanes_batch.inc) and the advisor's histograms per item (trc_planes_hist_batch.inc).
//
// Layout (include/trc_hip.h): item i has m[i] elements and nc[i] = ceil(m[i] / chunk) chunks; every item starts on
// a chunk boundary of the VIRTUAL buffer V, every item but the last is followed by zero elements up to nc[i] * chunk, so V has
// M = (NC - nc[last]) * chunk + m[last] elements and item i owns chunks [first[i], first[i] + nc[i]) of every plane.  V exists
// nowhere: the planes of V are written straight from the items.
//
// The kernels keep the shape of trc_planes.hip: a thread owns a VECTOR of 8 consecutive elements of V (1, 2 or 4 aligned 16-byte
// loads, v_perm_b32, one 8-byte store per plane; join the mirror image), 256 threads, a grid-stride loop under the same cap.  A chunk
// is a multiple of 64 elements, so an item starts on a multiple of 8 vectors and a vector never straddles two items.  What is new
// is the map from a vector of V to (item, offset):
//   * the call uploads one record per item (pointer, m, first vector, first chunk: 32 bytes),
//   * trc_planes_batch_map_kernel writes chunk_item[c] = the item of chunk c, once per CHUNK (a search over the records' first
//     chunks per chunk, not per vector: 1 / (chunk / 8) of the vectors, every chunk the same work however long its item is),
//   * split and join read chunk_item[v / (chunk / 8)] -- at least 32 neighbouring threads read the same word -- and then the
//     item's record; the division is a multiplication by a reciprocal the host supplies, with one correction.
//
// READS: nothing outside [0, n[i]) of an item.  A whole vector (e + 8 <= m) lies inside the item with all of its 16-byte words; the
// item's last, partial vector (m % 8 elements) is moved byte by byte by the thread that owns it (split_rest / join_rest below: the
// only other accesses to an item), so no 16-byte word that reaches past an item's last byte is loaded or stored.  Items need no
// readable slack behind them.
#include <vector>

#include "trc_planes_scan.h"                      // the scanning join (trc_fplanes_batch.inc)
#include "trc_planes_count.h"                     // the advisor's LDS counters (trc_planes_hist_batch.inc)
#include "trc_planes_order.h"                     // the predictors of order 2 and 3 (trc_oplanes_batch.inc)
#include "trc_planes_pred.h"                      // the predictors of a batch, shared with trc_planes_batch.inc

// one item as the kernels see it; `first` and `v0` count from the first chunk of the call's chunk range
struct BatchRec { uint64_t ptr, m, v0, first; };        // base address, elements, first vector (first * chunk / 8), first chunk
static_assert(sizeof(BatchRec) == 32, "two 16-byte loads per record");

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static bool batch_chunk_ok(uint32_t c) { return c >= TRC_CHUNK_MIN && c <= TRC_CHUNK_MAX && (c % 64u) == 0; }

// chunk_item[c] = the last item whose first chunk is <= c (first chunks increase strictly: every item has a chunk)
__global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_batch_map_kernel(const BatchRec *__restrict__ rec, u32 count, u32 nc, u32 *__restrict__ chunk_item)
{
    const u32 step = gridDim.x * TRC_PLANES_BLOCK;
    for (u32 c = blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; c < nc; c += step) {
        u32 lo = 0, hi = count;                    // rec[lo].first <= c < rec[hi].first  (rec[count].first = nc)
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (rec[mid].first <= c) lo = mid; else hi = mid;
        }
        chunk_item[c] = lo;
    }
}

// the chunk of vector v: v / vpc with rcp = floor(2^32 / vpc).  For v < 2^32 the estimate umulhi(v, rcp) falls short of the
// quotient by less than v / 2^32 < 1, so one correction makes it exact; longer planes take the plain division.
__device__ __forceinline__ u32 vec_chunk(size_t v, u32 vpc, u32 rcp)
{
    if (v >> 32) return (u32)(v / vpc);
    const u32 n = (u32)v;
    u32 q = __umulhi(n, rcp);
    if (n - q * vpc >= vpc) q++;
    return q;
}

// an item's last vector, r = m % 8 elements of it inside the item: their bytes one by one, then zero elements up to the vector's
// end -- unless the item is the last one, behind whose last element (element M of V) nothing is written
template <int ESIZE> __device__ inline void split_rest(const uint8_t *src, u32 r, u32 lim, uint8_t *dst, size_t pitch)
{
#pragma unroll 1
    for (u32 j = 0; j < lim; j++)
#pragma unroll 1
        for (u32 k = 0; k < ESIZE; k++) dst[k * pitch + j] = j < r ? src[j * ESIZE + k] : (uint8_t)0;
}
template <int ESIZE> __device__ inline void join_rest(const uint8_t *src, size_t pitch, u32 r, uint8_t *dst)
{
#pragma unroll 1
    for (u32 j = 0; j < r; j++)
#pragma unroll 1
        for (u32 k = 0; k < ESIZE; k++) dst[j * ESIZE + k] = src[k * pitch + j];
}

// planes: 256-byte aligned, pitch a multiple of 256 and at least M.  nv = ceil(M / 8) vectors.  Writes [0, M) of every plane, the
// pad zeros included, nothing else; reads [0, m * ESIZE) of every item, nothing else.
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_split_batch_kernel(const BatchRec *__restrict__ rec, const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp,
                                   size_t nv, size_t M, uint8_t *__restrict__ planes, size_t pitch)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const BatchRec r = rec[chunk_item[vec_chunk(v, vpc, rcp)]];
        const size_t e = (v - r.v0) * TRC_PLANES_VEC, vb = v * TRC_PLANES_VEC;       // the vector's first element in the item, in V
        uint8_t *dst = planes + vb;
        if (e + TRC_PLANES_VEC <= r.m) {
            const uint4 *src = (const uint4 *)(r.ptr + e * ESIZE);
            u32 w[NW];
#pragma unroll
            for (int q = 0; q < NQ; q++) { const uint4 x = src[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
            uint2 p[ESIZE];
            vec_split<ESIZE>(w, p);
#pragma unroll
            for (int k = 0; k < ESIZE; k++) *(uint2 *)(dst + k * pitch) = p[k];
        } else if (e < r.m) {
            const u32 rest = (u32)(r.m - e);
            split_rest<ESIZE>((const uint8_t *)(r.ptr + e * ESIZE), rest, vb + TRC_PLANES_VEC <= M ? TRC_PLANES_VEC : rest, dst, pitch);
        } else {                                   // pad: only behind an item that is not the last, so all 8 elements lie below M
#pragma unroll
            for (int k = 0; k < ESIZE; k++) *(uint2 *)(dst + k * pitch) = make_uint2(0u, 0u);
        }
    }
}

// the mirror image over the chunks of the requested items (planes: 64-byte aligned, element 0 = the first requested item's first):
// writes [0, m * ESIZE) of every item in rec[], nothing else; the pad is skipped
template <int ESIZE> __global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_planes_join_batch_kernel(const uint8_t *__restrict__ planes, size_t pitch, const BatchRec *__restrict__ rec,
                                  const u32 *__restrict__ chunk_item, u32 vpc, u32 rcp, size_t nv)
{
    constexpr int NW = 2 * ESIZE, NQ = NW / 4;
    const size_t step = (size_t)gridDim.x * TRC_PLANES_BLOCK;
    for (size_t v = (size_t)blockIdx.x * TRC_PLANES_BLOCK + threadIdx.x; v < nv; v += step) {
        const BatchRec r = rec[chunk_item[vec_chunk(v, vpc, rcp)]];
        const size_t e = (v - r.v0) * TRC_PLANES_VEC;
        const uint8_t *src = planes + v * TRC_PLANES_VEC;
        if (e + TRC_PLANES_VEC <= r.m) {
            uint2 p[ESIZE];
#pragma unroll
            for (int k = 0; k < ESIZE; k++) p[k] = *(const uint2 *)(src + k * pitch);
            u32 w[NW];
            vec_join<ESIZE>(p, w);
            uint4 *dst = (uint4 *)(r.ptr + e * ESIZE);
#pragma unroll
            for (int q = 0; q < NQ; q++) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        } else if (e < r.m) {
            join_rest<ESIZE>(src, pitch, (u32)(r.m - e), (uint8_t *)(r.ptr + e * ESIZE));
        }
    }
}

// ---- the plan (host only) ----------------------------------------------------------------------------------------------------------
// who == NULL: no text is left in trc_last_error() (the work-bytes functions, which answer 0)
#define PLAN_BAD(...) return who ? trc_fail(TRC_E_ARG, __VA_ARGS__) : (int)TRC_E_ARG
static int batch_plan(const char *who, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                      trc_planes_batch_plan *plan, uint64_t *first_chunk)
{
    if (!items || count == 0 || count > TRC_PLANES_BATCH_MAX) PLAN_BAD("%s: %zu items (1 .. %u)", who, count, TRC_PLANES_BATCH_MAX);
    if (!esize_ok(esize)) PLAN_BAD("%s: esize %u (2, 4 or 8)", who, esize);
    if (!batch_chunk_ok(chunk)) PLAN_BAD("%s: chunk %u: must be a multiple of 64 in [%u,%u]", who, chunk, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    uint64_t nc = 0, last_nc = 0, m_sum = 0;
    for (size_t i = 0; i < count; i++) {
        const uint64_t n = items[i].n;
        if (n < esize || n % esize) PLAN_BAD("%s: item %zu has %llu bytes: not a whole number (at least one) of %u-byte elements", who, i, (unsigned long long)n, esize);
        if (first_chunk) first_chunk[i] = nc;
        last_nc = (n / esize + chunk - 1) / chunk;
        nc += last_nc;                             // (at most 2^20 items of fewer than 2^63 chunks: no overflow before the check below)
        if (nc > 0x7fffffffu) PLAN_BAD("%s: too many chunks", who);
        m_sum += n / esize;
    }
    if (first_chunk) first_chunk[count] = nc;
    if (plan) {
        plan->chunks = nc;
        plan->m_total = (nc - last_nc) * chunk + items[count - 1].n / esize;
        plan->n_virtual = plan->m_total * esize;
        plan->pitch = trc_planes_pitch((size_t)plan->n_virtual, esize);
        plan->pad_elems = plan->m_total - m_sum;
    }
    return TRC_OK;
}
#undef PLAN_BAD
// for the work-bytes functions of trc_planes_batch.inc: the plan without a word
int trc_planes_batch_plan_quiet(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, trc_planes_batch_plan *plan, uint64_t *first_chunk)
{
    return batch_plan(nullptr, items, count, esize, chunk, plan, first_chunk);
}
extern "C" int trc_planes_batch_plan_host(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                          trc_planes_batch_plan *plan, uint64_t *first_chunk)
{
    if (!plan) return trc_fail(TRC_E_ARG, "planes_batch_plan: null plan");
    return batch_plan("planes_batch_plan", items, count, esize, chunk, plan, first_chunk);
}

// records of `count` items | chunk_item of `chunks` chunks
extern "C" size_t trc_planes_batch_table_bytes(size_t count, uint64_t chunks)
{
    if (count == 0 || count > TRC_PLANES_BATCH_MAX || chunks < count || chunks > 0x7fffffffu) return 0;
    return up256(count * sizeof(BatchRec)) + up256(4 * (size_t)chunks);
}

// items [first_item, first_item + item_count) of a batch that batch_plan has accepted: their pointers, the chunk and element counts
// of the range, and -- recs given -- their records
static int batch_range(const char *who, const trc_planes_item *items, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                       uint64_t &chunks, uint64_t &elems, std::vector<BatchRec> *recs)
{
    chunks = elems = 0;
    if (recs) recs->resize(item_count);
    for (size_t i = 0; i < item_count; i++) {
        const trc_planes_item &it = items[first_item + i];
        if (!it.d_ptr || ((uintptr_t)it.d_ptr & 15)) return trc_fail(TRC_E_ARG, "%s: item %zu: the pointer must be non-null and 16-byte aligned", who, first_item + i);
        const uint64_t m = it.n / esize;
        if (recs) (*recs)[i] = BatchRec{ (uint64_t)(uintptr_t)it.d_ptr, m, chunks * (chunk / TRC_PLANES_VEC), chunks };
        elems = chunks * chunk + m;                // (the last item of the range is not padded)
        chunks += (m + chunk - 1) / chunk;
    }
    return TRC_OK;
}
// the pointer rule alone, for the work-bytes functions of trc_planes_batch.inc
int trc_planes_batch_ptrs_ok(const trc_planes_item *items, size_t first_item, size_t item_count)
{
    for (size_t i = 0; i < item_count; i++)
        if (!items[first_item + i].d_ptr || ((uintptr_t)items[first_item + i].d_ptr & 15)) return 0;
    return 1;
}

static unsigned batch_grid(size_t units)
{
    const size_t want = (units + TRC_PLANES_BLOCK - 1) / TRC_PLANES_BLOCK;
    const unsigned cap = planes_grid_cap();
    return want < 1 ? 1u : want > cap ? cap : (unsigned)want;
}

// the records to the table (the host array is free again when this returns: the copy waits for the stream), then the map kernel
static int batch_table(const char *who, const std::vector<BatchRec> &recs, uint64_t chunks, void *d_table, hipStream_t s, const BatchRec *&d_rec, const u32 *&d_map)
{
    const size_t count = recs.size();
    const hipError_t e = hipMemcpyWithStream(d_table, recs.data(), count * sizeof(BatchRec), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return trc_fail(TRC_E_HIP, "%s: table upload: %s", who, hipGetErrorString(e));
    d_rec = (const BatchRec *)d_table;
    u32 *map = (u32 *)((uint8_t *)d_table + up256(count * sizeof(BatchRec)));
    d_map = map;
    hipLaunchKernelGGL(trc_planes_batch_map_kernel, dim3(batch_grid((size_t)chunks)), dim3(TRC_PLANES_BLOCK), 0, s, d_rec, (u32)count, (u32)chunks, map);
    return TRC_OK;
}

static int batch_table_args(const char *who, size_t need, const void *d_table, size_t table_bytes)
{
    if (!d_table || ((uintptr_t)d_table & 255)) return trc_fail(TRC_E_ARG, "%s: the table must be 256-byte aligned", who);
    if (table_bytes < need) return trc_fail(TRC_E_WORK, "%s: table %zu B < required %zu B", who, table_bytes, need);
    return TRC_OK;
}

// ---- the kernels with a predictor filter per item --------------------------------------------------------------------------------
#include "trc_fplanes_batch.inc"

// ---- the kernels with a filter and a stride per item -----------------------------------------------------------------------------
#include "trc_splanes_batch.inc"

// ---- the kernels with a filter, a stride and a predictor order per item -----------------------------------------------------------
#include "trc_oplanes_batch.inc"

// ---- the kernels with a filter against a base per item ----------------------------------------------------------------------------
#include "trc_bplanes_batch.inc"

// ---- split and join: plain, with filters, with filters and strides, with filters against bases ------------------------------------
typedef void (*split_batch_fn)(const BatchRec *, const u32 *, u32, u32, size_t, size_t, uint8_t *, size_t);
static const split_batch_fn split_batch_kernels[3][3] = { TRC_BY_ESIZE(trc_planes_split_batch_kernel), TRC_BY_ESIZE(trc_fplanes_split_batch_kernel),
                                                          TRC_BY_ESIZE(trc_splanes_split_batch_kernel) };     // [none, any filter, a stride above 1][esize_row]
static void (*const join_batch_kernels[3])(const uint8_t *, size_t, const BatchRec *, const u32 *, u32, u32, size_t) = TRC_BY_ESIZE(trc_planes_join_batch_kernel);
typedef void (*fjoin_batch_fn)(const uint8_t *, size_t, const BatchRec *, const u32 *, u32, u32, size_t, u32, u32, size_t);
static const fjoin_batch_fn fjoin_batch_kernels[2][3] = { TRC_BY_ESIZE(trc_fplanes_join_batch_kernel), TRC_BY_ESIZE(trc_splanes_join_batch_kernel) };     // [a stride above 1][esize_row]
static const split_batch_fn osplit_batch_kernels[3] = TRC_BY_ESIZE(trc_oplanes_split_batch_kernel);         // [esize_row]: an order above 1
static const fjoin_batch_fn ojoin_batch_kernels[3] = TRC_BY_ESIZE(trc_oplanes_join_batch_kernel);
static void (*const bsplit_batch_kernels[3])(const BatchRec *, const u32 *, const uint64_t *, u32, u32, size_t, size_t, uint8_t *, size_t) = TRC_BY_ESIZE(trc_bplanes_split_batch_kernel);
static void (*const bjoin_batch_kernels[3])(const uint8_t *, size_t, const BatchRec *, const u32 *, const uint64_t *, u32, u32, size_t) = TRC_BY_ESIZE(trc_bplanes_join_batch_kernel);

// Every kind of batch (BatchPred, trc_planes_pred.h).  Checks: the plan, the filters, the strides, then pointers and buffers.
// filters == NULL: the batch call; a batch whose filters are all TRC_FILTER_NONE is that call too -- whatever else the descriptor
// holds -- and says so in its messages.  strides == NULL: the filtered batch call; a batch in which no item with a filter has a
// stride above 1 is that call too, likewise.  orders == NULL: the strided batch call; a batch in which no ZDELTA item has an order above
// 1 is that call too, likewise (checks: the orders behind the strides).  A base that overlaps its item in any other way than being it (join) is NOT checked.
int split_batch(const char *who, const trc_planes_item *items, BatchPred pred, size_t count, unsigned esize, uint32_t chunk,
                void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    trc_planes_batch_plan P;
    int rc = batch_plan(who, items, count, esize, chunk, &P, nullptr);
    if (rc) return rc;
    bool any, strided;
    if ((rc = trc_planes_batch_filters(who, pred.filters, count, &any))) return rc;
    if ((rc = trc_planes_batch_strides(who, pred.filters, pred.strides, count, &strided))) return rc;
    bool ordered;
    if ((rc = trc_planes_batch_orders(who, pred.filters, pred.orders, count, &ordered))) return rc;
    if (!ordered && pred.orders) who = "planes_split_sbatch";
    if (!ordered && !strided && pred.strides) who = "planes_split_fbatch";
    if (!any) { who = "planes_split_batch"; pred = batch_pred_none(); }
    if (!d_planes || ((uintptr_t)d_planes & 255)) return trc_fail(TRC_E_ARG, "%s: the planes must be 256-byte aligned", who);
    if ((pitch & 255) || pitch < P.m_total) return trc_fail(TRC_E_ARG, "%s: pitch %zu must be a multiple of 256 and at least %llu", who, pitch, (unsigned long long)P.m_total);
    if ((rc = batch_table_args(who, batch_pred_table_bytes(pred, count, P.chunks), d_table, table_bytes))) return rc;
    std::vector<BatchRec> recs;
    uint64_t chunks, elems;
    if ((rc = batch_range(who, items, 0, count, esize, chunk, chunks, elems, &recs))) return rc;
    if (pred.based && (rc = trc_planes_bbatch_bases(who, pred.bases, pred.filters, 0, count))) return rc;
    if (any) fbatch_pack(recs, pred.filters);
    if (strided) sbatch_pack(recs, pred.filters, pred.strides);
    if (ordered) obatch_pack(recs, pred.filters, pred.orders);
    hipStream_t s = (hipStream_t)stream;
    const BatchRec *d_rec;
    const u32 *d_map;
    const uint64_t *d_base = nullptr;
    if ((rc = batch_table(who, recs, chunks, d_table, s, d_rec, d_map))) return rc;
    if (pred.based && (rc = bbatch_bases_up(who, pred.bases, pred.filters, 0, count, chunks, d_table, s, d_base))) return rc;
    const size_t M = (size_t)elems, nv = (M + TRC_PLANES_VEC - 1) / TRC_PLANES_VEC;
    const u32 vpc = chunk / TRC_PLANES_VEC, rcp = (u32)(((uint64_t)1 << 32) / vpc);
    if (pred.based)
        hipLaunchKernelGGL(bsplit_batch_kernels[esize_row(esize)], dim3(batch_grid(nv)), dim3(TRC_PLANES_BLOCK), 0, s, d_rec, d_map, d_base, vpc, rcp, nv, M, (uint8_t *)d_planes, pitch);
    else if (ordered)
        hipLaunchKernelGGL(osplit_batch_kernels[esize_row(esize)], dim3(batch_grid(nv)), dim3(TRC_PLANES_BLOCK), 0, s, d_rec, d_map, vpc, rcp, nv, M, (uint8_t *)d_planes, pitch);
    else
        hipLaunchKernelGGL(split_batch_kernels[strided ? 2 : any][esize_row(esize)], dim3(batch_grid(nv)), dim3(TRC_PLANES_BLOCK), 0, s, d_rec, d_map, vpc, rcp, nv, M, (uint8_t *)d_planes, pitch);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

int join_batch(const char *who, const void *d_planes, size_t pitch, const trc_planes_item *items, BatchPred pred, size_t count, size_t first_item, size_t item_count,
               unsigned esize, uint32_t chunk, void *d_table, size_t table_bytes, void *stream)
{
    int rc = batch_plan(who, items, count, esize, chunk, nullptr, nullptr);
    if (rc) return rc;
    bool any, strided;
    if ((rc = trc_planes_batch_filters(who, pred.filters, count, &any))) return rc;
    if ((rc = trc_planes_batch_strides(who, pred.filters, pred.strides, count, &strided))) return rc;
    bool ordered;
    if ((rc = trc_planes_batch_orders(who, pred.filters, pred.orders, count, &ordered))) return rc;
    if (!ordered && pred.orders) who = "planes_join_sbatch";
    if (!ordered && !strided && pred.strides) who = "planes_join_fbatch";
    if (!any) { who = "planes_join_batch"; pred = batch_pred_none(); }
    if (first_item > count || item_count > count - first_item)
        return trc_fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    std::vector<BatchRec> recs;
    uint64_t chunks, elems;
    if ((rc = batch_range(who, items, first_item, item_count, esize, chunk, chunks, elems, &recs))) return rc;
    if (pred.based && (rc = trc_planes_bbatch_bases(who, pred.bases, pred.filters, first_item, item_count))) return rc;
    if (any) fbatch_pack(recs, pred.filters + first_item);
    if (strided) sbatch_pack(recs, pred.filters + first_item, pred.strides + first_item);
    if (ordered) obatch_pack(recs, pred.filters + first_item, pred.orders + first_item);
    if (!d_planes || ((uintptr_t)d_planes & 63)) return trc_fail(TRC_E_ARG, "%s: the planes must be 64-byte aligned", who);
    if ((pitch & 255) || pitch < elems) return trc_fail(TRC_E_ARG, "%s: pitch %zu must be a multiple of 256 and at least %llu", who, pitch, (unsigned long long)elems);
    if ((rc = batch_table_args(who, batch_pred_table_bytes(pred, item_count, chunks), d_table, table_bytes))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const BatchRec *d_rec;
    const u32 *d_map;
    const uint64_t *d_base = nullptr;
    if ((rc = batch_table(who, recs, chunks, d_table, s, d_rec, d_map))) return rc;
    if (pred.based && (rc = bbatch_bases_up(who, pred.bases, pred.filters, first_item, item_count, chunks, d_table, s, d_base))) return rc;
    const u32 vpc = chunk / TRC_PLANES_VEC, rcp = (u32)(((uint64_t)1 << 32) / vpc);
    const size_t nv = ((size_t)elems + TRC_PLANES_VEC - 1) / TRC_PLANES_VEC;
    if (pred.based) {                              // elementwise, as the plain join
        hipLaunchKernelGGL(bjoin_batch_kernels[esize_row(esize)], dim3(batch_grid(nv)), dim3(TRC_PLANES_BLOCK), 0, s, (const uint8_t *)d_planes, pitch, d_rec, d_map, d_base, vpc, rcp, nv);
    } else if (any) {                              // the scanning join: a wave per span
        u32 span;
        size_t nspan;
        const unsigned grid = join_grid((size_t)elems, chunk, span, nspan);
        hipLaunchKernelGGL(ordered ? ojoin_batch_kernels[esize_row(esize)] : fjoin_batch_kernels[strided][esize_row(esize)], dim3(grid), dim3(TRC_PLANES_BLOCK), 0, s, (const uint8_t *)d_planes, pitch, d_rec, d_map, vpc, rcp,
                           (size_t)elems, chunk, span, nspan);
    } else {
        hipLaunchKernelGGL(join_batch_kernels[esize_row(esize)], dim3(batch_grid(nv)), dim3(TRC_PLANES_BLOCK), 0, s, (const uint8_t *)d_planes, pitch, d_rec, d_map, vpc, rcp, nv);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int trc_planes_split_batch_dev(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                          void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    return split_batch("planes_split_batch", items, batch_pred_none(), count, esize, chunk, d_planes, pitch, d_table, table_bytes, stream);
}
extern "C" int trc_planes_split_fbatch_dev(const trc_planes_item *items, const uint8_t *filters, size_t count, unsigned esize, uint32_t chunk,
                                           void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    return split_batch("planes_split_fbatch", items, batch_pred_strides(filters, nullptr), count, esize, chunk, d_planes, pitch, d_table, table_bytes, stream);
}
extern "C" int trc_planes_split_sbatch_dev(const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count, unsigned esize,
                                           uint32_t chunk, void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    return split_batch("planes_split_sbatch", items, batch_pred_strides(filters, strides), count, esize, chunk, d_planes, pitch, d_table, table_bytes, stream);
}
extern "C" int trc_planes_split_obatch_dev(const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders, size_t count,
                                           unsigned esize, uint32_t chunk, void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    return split_batch(orders ? "planes_split_obatch" : "planes_split_sbatch", items, batch_pred_orders(filters, strides, orders), count, esize, chunk, d_planes, pitch, d_table, table_bytes, stream);
}
extern "C" int trc_planes_split_bbatch_dev(const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                           unsigned esize, uint32_t chunk, void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream)
{
    return split_batch("planes_split_bbatch", items, batch_pred_bases(filters, bases), count, esize, chunk, d_planes, pitch, d_table, table_bytes, stream);
}
extern "C" int trc_planes_join_batch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, size_t count,
                                         size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                         void *d_table, size_t table_bytes, void *stream)
{
    return join_batch("planes_join_batch", d_planes, pitch, items, batch_pred_none(), count, first_item, item_count, esize, chunk, d_table, table_bytes, stream);
}
extern "C" int trc_planes_join_fbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, size_t count,
                                          size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          void *d_table, size_t table_bytes, void *stream)
{
    return join_batch("planes_join_fbatch", d_planes, pitch, items, batch_pred_strides(filters, nullptr), count, first_item, item_count, esize, chunk, d_table, table_bytes, stream);
}
extern "C" int trc_planes_join_sbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                                          size_t count, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          void *d_table, size_t table_bytes, void *stream)
{
    return join_batch("planes_join_sbatch", d_planes, pitch, items, batch_pred_strides(filters, strides), count, first_item, item_count, esize, chunk, d_table, table_bytes, stream);
}
extern "C" int trc_planes_join_obatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                                          const uint8_t *orders, size_t count, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                          void *d_table, size_t table_bytes, void *stream)
{
    return join_batch(orders ? "planes_join_obatch" : "planes_join_sbatch", d_planes, pitch, items, batch_pred_orders(filters, strides, orders), count, first_item, item_count, esize, chunk,
                      d_table, table_bytes, stream);
}
extern "C" int trc_planes_join_bbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const void *const *bases,
                                          const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                          unsigned esize, uint32_t chunk, void *d_table, size_t table_bytes, void *stream)
{
    return join_batch("planes_join_bbatch", d_planes, pitch, items, batch_pred_bases(filters, bases), count, first_item, item_count, esize, chunk, d_table, table_bytes, stream);
}

// ---- the advisor's histograms, per item ---------------------------------------------------------------------------------------
#include "trc_planes_hist_batch.inc"

// ---- the fingerprints of a batch's bases, per item ------------------------------------------------------------------------------
#include "trc_fp_batch.inc"
