// trc_planes_pred.h -- how the elements of a BATCH are predicted, for the two files that have to agree on it: trc_planes_batch.hip
// (split_batch / join_batch, which launch for every kind) and trc_planes_batch.inc (the coded calls around them).  Host only.
#pragma once

// filters == NULL: nothing is predicted.  strides: a stride per item with a filter (NULL: 1).  based: a filter id is against
// bases[i] -- and a missing base is the caller's error, so `bases` may be NULL where `based` is set.  orders: a predictor order per item
// whose filter is TRC_FILTER_ZDELTA (NULL: 1)
struct BatchPred { const uint8_t *filters, *strides; const void *const *bases; bool based; const uint8_t *orders = nullptr; };
static inline BatchPred batch_pred_none() { return BatchPred{ nullptr, nullptr, nullptr, false }; }
static inline BatchPred batch_pred_strides(const uint8_t *filters, const uint8_t *strides) { return BatchPred{ filters, strides, nullptr, false }; }
static inline BatchPred batch_pred_orders(const uint8_t *filters, const uint8_t *strides, const uint8_t *orders) { return BatchPred{ filters, strides, nullptr, false, orders }; }
static inline BatchPred batch_pred_bases(const uint8_t *filters, const void *const *bases) { return BatchPred{ filters, nullptr, bases, filters != nullptr }; }
static const BatchPred BATCH_PRED_BASED = { nullptr, nullptr, nullptr, true };      // for the sizes of a call against bases, which look at nothing else

// the table of a call: records and chunk map, and behind them a base pointer per item where the filters are against bases
static inline size_t batch_pred_table_bytes(const BatchPred &p, size_t count, uint64_t chunks)
{
    const size_t t = trc_planes_batch_table_bytes(count, chunks);
    return t && p.based ? t + ((8 * count + 255) & ~(size_t)255) : t;
}

// trc_planes_batch.hip; `who` speaks until the predictors are known (the all-NONE and unstrided renamings happen inside)
__attribute__((visibility("hidden")))
int split_batch(const char *who, const trc_planes_item *items, BatchPred pred, size_t count, unsigned esize, uint32_t chunk,
                void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream);
__attribute__((visibility("hidden")))
int join_batch(const char *who, const void *d_planes, size_t pitch, const trc_planes_item *items, BatchPred pred, size_t count, size_t first_item, size_t item_count,
               unsigned esize, uint32_t chunk, void *d_table, size_t table_bytes, void *stream);
