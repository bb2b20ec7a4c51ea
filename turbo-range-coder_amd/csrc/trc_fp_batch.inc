// trc_fp_batch.inc -- the fingerprints of the bases of a BATCH (included by trc_planes_batch.hip behind its kernels): what
// trc_base_fingerprint_dev (trc_bplanes.hip) gives for one buffer, for every item of an item range from ONE launch, and the
// comparison of such fingerprints with those a TRCE container holds (include/trc_hip.h).
//
// A launch per base is what this replaces: thousands of 4 KiB bases would pay a launch apiece.  A workgroup per base would leave the
// one 200 MB embedding of a checkpoint to one workgroup.  So the work is cut by BYTES: a base of np whole 16-byte pairs is
// max(1, ceil(np / TRC_FP_TILE)) tiles of TRC_FP_TILE pairs, the tiles of the requested bases are numbered through, and workgroup b
// owns the contiguous run [b * tpw, (b + 1) * tpw) of them.  It finds the record of its first tile by a search over the records'
// first tiles and walks on record by record; of each base it sums the pairs of its run (pair i of the base weighs words 2i and 2i + 1:
// fp_pair), four 16-byte loads in flight per thread, reduces across the wave and the workgroup, and issues ONE 64-bit atomicAdd per
// (workgroup, base).  Where the run holds all of a base's tiles nobody else adds to that fingerprint, which the call has zeroed: the
// sum is stored.  The lane that sums a base's first tile adds the bytes behind the last whole pair and the length term.
//
// READS: bytes [0, nbytes) of a requested base and nothing else: whole 16-byte pairs, the (at most 15) bytes behind them one by one.
#include "trc_fp.h"

#define TRC_FP_TILE 256u                          // 16-byte pairs per tile: 4 KiB, one pair per thread
// one requested base as the kernel sees it: address, bytes, first tile, where its fingerprint goes (the item's index in the range)
struct FpRec { uint64_t ptr, nbytes, first, out; };
static_assert(sizeof(FpRec) == 32, "two 16-byte loads per record");

__host__ __device__ static inline uint64_t fp_tiles(uint64_t nbytes)
{
    const uint64_t t = (nbytes / 16 + TRC_FP_TILE - 1) / TRC_FP_TILE;
    return t ? t : 1;                              // a base shorter than a pair still has its rest and its length term
}

// rec: nrec >= 1 records, first tiles increasing from 0; ntiles = the sum of their tiles; gridDim.x * tpw >= ntiles > (gridDim.x - 1) * tpw.
// fp[rec[].out] += the base's fingerprint; zero on entry.
__global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_base_fingerprint_batch_kernel(const FpRec *__restrict__ rec, u32 nrec, uint64_t ntiles, uint64_t tpw, u64a *__restrict__ fp)
{
    __shared__ uint64_t wave_sum[TRC_PLANES_BLOCK / 64];
    const u32 tid = threadIdx.x;
    const uint64_t t_lo = (uint64_t)blockIdx.x * tpw, t_hi = ntiles - t_lo < tpw ? ntiles : t_lo + tpw;
    // everything that shapes the walk is the same in all lanes: the record of tile t_lo is the last whose first tile is <= t_lo
    u32 lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (rec[mid].first <= t_lo) lo = mid; else hi = mid;
    }
    u32 it = lo;
    for (uint64_t t = t_lo; t < t_hi; it++) {
        const FpRec r = rec[it];
        const size_t np = (size_t)(r.nbytes / 16);
        const uint64_t last = r.first + fp_tiles(r.nbytes), t_end = last < t_hi ? last : t_hi;      // the run's part of the base: tiles [t, t_end)
        const size_t p_run = (size_t)(t_end - r.first) * TRC_FP_TILE, p1 = p_run < np ? p_run : np;
        const uint4 *src = (const uint4 *)r.ptr;
        uint64_t sum = 0;
        size_t i = (size_t)(t - r.first) * TRC_FP_TILE + tid;
        for (; i + 3 * TRC_PLANES_BLOCK < p1; i += 4 * TRC_PLANES_BLOCK) {      // four loads in flight per thread
            uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) x[u] = src[i + u * TRC_PLANES_BLOCK];
#pragma unroll
            for (int u = 0; u < 4; u++) sum += fp_pair(i + u * TRC_PLANES_BLOCK, x[u]);
        }
        for (; i < p1; i += TRC_PLANES_BLOCK) sum += fp_pair(i, src[i]);
        if (t == r.first && tid == 0) sum += fp_rest((const uint8_t *)r.ptr, (size_t)r.nbytes);
#pragma unroll
        for (u32 d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
        if ((tid & 63u) == 0) wave_sum[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) {
            uint64_t s = 0;
#pragma unroll
            for (int w = 0; w < TRC_PLANES_BLOCK / 64; w++) s += wave_sum[w];
            if (t == r.first && t_end == last) fp[r.out] = (u64a)s;          // the base is this run's alone
            else atomicAdd(&fp[r.out], (u64a)s);
        }
        __syncthreads();                           // wave_sum is the next base's as well
        t = t_end;
    }
}

// bad = the lowest first_item + j, j in [0, item_count), with fp[j] != cont_fp[first_item + j]; -1 where there is none.  One workgroup.
__global__ __launch_bounds__(TRC_PLANES_BLOCK)
void trc_base_verify_batch_kernel(const uint64_t *__restrict__ cont_fp, const uint64_t *__restrict__ fp, uint64_t first_item, uint64_t item_count,
                                  long long *__restrict__ bad)
{
    __shared__ uint64_t wave_min[TRC_PLANES_BLOCK / 64];
    uint64_t m = ~(uint64_t)0;
    for (uint64_t j = threadIdx.x; j < item_count; j += TRC_PLANES_BLOCK)
        if (fp[j] != cont_fp[first_item + j]) { m = first_item + j; break; }          // (a thread's j only grow)
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_down(m, d); m = o < m ? o : m; }
    if ((threadIdx.x & 63u) == 0) wave_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TRC_PLANES_BLOCK / 64; w++) m = wave_min[w] < m ? wave_min[w] : m;
        *bad = m == ~(uint64_t)0 ? -1ll : (long long)m;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// records of item_count bases | item_count fingerprints (trc_base_verify_batch_dev keeps the range's there; the fingerprint call
// itself uses the records alone)
extern "C" size_t trc_base_fingerprint_batch_table_bytes(size_t item_count)
{
    if (item_count == 0 || item_count > TRC_PLANES_BATCH_MAX) return 0;
    return up256(item_count * sizeof(FpRec)) + up256(item_count * sizeof(uint64_t));
}

// where trc_base_verify_batch_dev keeps the range's fingerprints: the table's second part
static uint64_t *const FP_IN_TABLE = (uint64_t *)(uintptr_t)1;
static inline uint64_t *fp_in_table(void *d_table, size_t item_count) { return (uint64_t *)((uint8_t *)d_table + up256(item_count * sizeof(FpRec))); }

// Checks, in this order: the items (a batch of 1 .. TRC_PLANES_BATCH_MAX items that hold bytes; no element size is known here), the
// filters, the range, the pointers, the table.
static int fp_batch(const char *who, const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                    size_t first_item, size_t item_count, uint64_t *d_fp, void *d_table, size_t table_bytes, void *stream)
{
    if (!items || count == 0 || count > TRC_PLANES_BATCH_MAX) return trc_fail(TRC_E_ARG, "%s: %zu items (1 .. %u)", who, count, TRC_PLANES_BATCH_MAX);
    for (size_t i = 0; i < count; i++)
        if (items[i].n == 0) return trc_fail(TRC_E_ARG, "%s: item %zu has no bytes", who, i);
    int rc = trc_planes_batch_filters(who, filters, count, nullptr);
    if (rc) return rc;
    if (first_item > count || item_count > count - first_item)
        return trc_fail(TRC_E_ARG, "%s: items [%zu, %zu + %zu) of %zu", who, first_item, first_item, item_count, count);
    if (item_count == 0) return TRC_OK;
    if ((rc = trc_planes_bbatch_bases(who, bases, filters, first_item, item_count))) return rc;
    if (d_fp != FP_IN_TABLE && (!d_fp || ((uintptr_t)d_fp & 7))) return trc_fail(TRC_E_ARG, "%s: d_fp must be 8-byte aligned", who);
    if ((rc = batch_table_args(who, trc_base_fingerprint_batch_table_bytes(item_count), d_table, table_bytes))) return rc;
    if (d_fp == FP_IN_TABLE) d_fp = fp_in_table(d_table, item_count);
    std::vector<FpRec> recs;
    uint64_t tiles = 0;
    for (size_t j = 0; filters && j < item_count; j++) {
        const size_t i = first_item + j;
        if (filters[i] == TRC_FILTER_NONE) continue;
        recs.push_back(FpRec{ (uint64_t)(uintptr_t)bases[i], items[i].n, tiles, j });
        tiles += fp_tiles(items[i].n);
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_fp, 0, item_count * sizeof(uint64_t), s);
    if (e != hipSuccess) return trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
    if (recs.empty()) return TRC_OK;
    // (the host array is free again when this returns: the copy waits for the stream, as the batched calls' table upload does)
    e = hipMemcpyWithStream(d_table, recs.data(), recs.size() * sizeof(FpRec), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return trc_fail(TRC_E_HIP, "%s: table upload: %s", who, hipGetErrorString(e));
    // a workgroup per four tiles (four loads per thread in a long base) under the cap of the other plane kernels, then whole tiles
    unsigned grid = batch_grid((size_t)tiles * (TRC_PLANES_BLOCK / 4));
    if (grid > tiles) grid = (unsigned)tiles;
    const uint64_t tpw = (tiles + grid - 1) / grid;
    grid = (unsigned)((tiles + tpw - 1) / tpw);
    hipLaunchKernelGGL(trc_base_fingerprint_batch_kernel, dim3(grid), dim3(TRC_PLANES_BLOCK), 0, s, (const FpRec *)d_table, (u32)recs.size(), tiles, tpw, (u64a *)d_fp);
    e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int trc_base_fingerprint_batch_dev(const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                              size_t first_item, size_t item_count, uint64_t *d_fp,
                                              void *d_table, size_t table_bytes, void *stream)
{
    return fp_batch("base_fingerprint_batch", items, bases, filters, count, first_item, item_count, d_fp, d_table, table_bytes, stream);
}

extern "C" int trc_base_verify_batch_dev(const void *d_cont, const trc_planes_item *items, const void *const *bases, const uint8_t *filters,
                                         size_t count, size_t first_item, size_t item_count, int64_t *d_bad,
                                         void *d_table, size_t table_bytes, void *stream)
{
    const char *who = "base_verify_batch";
    if (!d_cont || ((uintptr_t)d_cont & 7)) return trc_fail(TRC_E_ARG, "%s: d_cont must be 8-byte aligned", who);
    if (!d_bad || ((uintptr_t)d_bad & 7)) return trc_fail(TRC_E_ARG, "%s: d_bad must be 8-byte aligned", who);
    const int rc = fp_batch(who, items, bases, filters, count, first_item, item_count, FP_IN_TABLE, d_table, table_bytes, stream);
    if (rc) return rc;
    const uint64_t *d_fp = item_count ? fp_in_table(d_table, item_count) : nullptr;      // (no item: nothing is compared)
    hipLaunchKernelGGL(trc_base_verify_batch_kernel, dim3(1), dim3(TRC_PLANES_BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)((const uint8_t *)d_cont + 16), d_fp, (uint64_t)first_item, (uint64_t)item_count, (long long *)d_bad);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "%s: %s", who, hipGetErrorString(e));
}
