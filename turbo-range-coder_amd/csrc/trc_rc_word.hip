// trc_rc_word.hip -- bitwise word range coders for 16 / 32-bit data, "s" predictor: codecs TRC_RCW16 (rcsenc16 / rcsdec16),
// TRC_RCW32 (rcsenc32 / rcsdec32), TRC_RCCW32 (rccsenc32 / rccsdec32) and TRC_RCC2W32 (rcc2senc32 / rcc2sdec32), reference
// rc_.c:60-138, 248-342, `turborc -e6/7/8`.
//
// Per chunk the payload is what the reference function returns for that slice, with two exceptions, both stored raw: a chunk
// shorter than one element (only a final chunk can be one; the reference returns its tail bytes plus an empty flush), and a
// TRC_RCW16 chunk whose coded length would be >= its length (rcsenc16 has no OVERFLOW test and returns more than its input).
// Geometry as TRC_RCC1: 64-bit range, 32-bit words, 15-bit probabilities, all 0x4000 at chunk start, update mbc_s.h:53-55,
// every byte coded with mb8enc (mb_o0.h:89-112: renormalisation before bits 7, 5, 3, 1) in a tree the context picks.
// A word's bytes are coded top byte first; the trees of one chunk (`prev` = the previous word, 0 at chunk start):
//   RCW16    the high byte in tree 0, the low byte in tree 1 + high byte                               257 trees
//   RCW32    byte 3 in tree 0; byte 2 in F + b3; byte 1 in F + 256 + ((b3 & 3) << 8 | b2);
//            byte 0 in F + 1280 + ((b2 & 3) << 8 | b1) (BZHI32(cx, XN1 = 10) of the bytes above), F = 1   2305 trees
//   RCCW32   as RCW32, byte 3 in tree (prev >> 25) & 127 (CX32 with XN = 7), F = 128                    2432 trees
//   RCC2W32  as RCW32, byte 3 in tree (prev >> 20) & 0x7ff (CX32 with XNS = 12, XN = 11), F = 2048        4352 trees
// The len % es tail bytes go to the FRONT of the payload (INDEC, rcutil_.h:134).  The 32-bit coders test OVERFLOW
// (rcutil_.h:130, tail bytes counted) after every word, as the reference does; the 16-bit coder tests its output against the
// chunk length after every word instead -- past that the chunk ends raw anyway -- which also bounds its scratch region.
//
// Model residency.  A tree is a row of 272 u16 in the TRC_RCC1 block layout (block 0: the 15 nodes of the high nibble,
// block 1 + h: the 15 nodes under high nibble h, 32 bytes each), so a chunk's model is 136.5 KiB .. 2.26 MiB.  Models live in
// the workspace, but not one per chunk: a call holds `slots` of them (trc_word_slots: at most TRC_WORD_MODEL_BUDGET bytes,
// whole waves), and the launchers run the chunks in rounds of `slots`, each round on freshly filled slots, all on the
// caller's stream.  The encoder writes clen and its group sums per round; the gather runs once after the last.
// Per nibble the decoder loads the 15 nodes it may visit as one 32-byte block (two dependent loads per byte); the block of a
// word's first tree is requested as soon as it is known (RCW16 / RCW32 / RCCW32: once the previous word's top byte is
// decoded; RCC2W32: once its byte 2 is) and arrives while the rest of that word decodes.  The encoder knows all eight
// blocks of a word from the word and requests them before it codes its first bit.
// Decoder bounds: every tree index is a masked byte combination and every nibble is 0..15, so no corrupt payload indexes
// outside the lane's model; reads are clamped to the chunk's clen, the tail copy to the chunk's length.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_launch.h"
#include "trc_tree.h"
#include "../../include/trc_hip.h"

#define WORD_TREE_U16 272u                                      // one tree: 17 blocks of 16 u16

// K = codec - TRC_RCW16: 0 rcs16, 1 rcs32, 2 rccs32, 3 rcc2s32
template <int K>
struct WordCfg {
    static constexpr u32 ES = K == 0 ? 2u : 4u, NB = ES;        // bytes per word = trees per word
    static constexpr u32 F = K == 2 ? 128u : K == 3 ? 2048u : 1u;  // trees for the top byte
    static constexpr u32 TREES = ES == 2 ? 257u : F + 256u + 2048u;
    static constexpr u32 KNOW = K == 3 ? 2u : 1u;               // decoded bytes after which the next word's first tree is known
    // the top byte's tree from the previous word
    static __device__ __forceinline__ u32 first(u32 prev) { return K == 2 ? (prev >> 25) & 127u : K == 3 ? (prev >> 20) & 0x7ffu : 0u; }
    // the tree of decoded byte d >= 1 from the bytes above it (r: those bytes, top byte highest)
    static __device__ __forceinline__ u32 tree(u32 d, u32 r)
    {
        if (ES == 2) return 1u + r;
        return d == 1 ? F + r : d == 2 ? F + 256u + (r & 0x3ffu) : F + 1280u + (r & 0x3ffu);
    }
};

static inline uint32_t word_tree_count(int k) { return k == 0 ? 257u : k == 1 ? 2305u : k == 2 ? 2432u : 4352u; }

__device__ __forceinline__ void word_load_block(u32 (&q)[8], const u16 *p)
{
    const uint4 a = *(const uint4 *)p, b = *(const uint4 *)(p + 8u);
    q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
}

// chunks c0 .. c0 + nround - 1 of this round; lane's model = slot c - c0; c0 is a multiple of 64 (slots are whole waves)
template <int K>
__global__ __launch_bounds__(64) void trc_rc_word_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u32 c0, u32 nround, u16 *__restrict__ models,
    u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ clen, u32 *__restrict__ gsum)
{
    using W = WordCfg<K>;
    const u32 lane = trc_lane(), c = c0 + blockIdx.x * 64u + lane;
    const bool alive = c < nchunks && c < c0 + nround;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    const u32 nel = len / W::ES, tail = len - nel * W::ES;
    const int lim = W::ES == 2 ? (int)len : trc_rc_limit(len);  // rcs16: no OVERFLOW, stop at the chunk length (raw)
    u16 *const m = models + (u64)(alive ? c - c0 : 0u) * (W::TREES * WORD_TREE_U16);
    const u8 *src = in + (u64)c * chunk;
    u8 *const dst = scratch + (u64)c * stride;
    IntOut so; so.start(dst, tail);
    for (u32 i = 0; i < tail; i++) dst[i] = src[nel * W::ES + i];
    RcEnc e; e.start();

    bool raw = alive && nel == 0u;                             // shorter than one element: stored raw
    u32 prev = 0;
    for (u32 i = 0; alive && !raw && i < nel; i++) {
        const u32 v = W::ES == 2 ? (u32)*(const u16 *)(src + 2u * i) : *(const u32 *)(src + 4u * i);
        u16 *blk[2 * W::NB];
        u32 q[16 * W::NB];                                     // block b's nodes at q[8 b ..]
        u32 r = 0;
#pragma unroll
        for (u32 d = 0; d < W::NB; d++) {
            const u32 x = (v >> (8u * (W::NB - 1u - d))) & 255u;
            u16 *const t = m + (d == 0 ? W::first(prev) : W::tree(d, r)) * WORD_TREE_U16;
            blk[2 * d] = t;
            blk[2 * d + 1] = t + 16u * (1u + (x >> 4));
            r = r << 8 | x;
        }
#pragma unroll
        for (u32 b = 0; b < 2 * W::NB; b++) {
            const uint4 lo = *(const uint4 *)blk[b], hi = *(const uint4 *)(blk[b] + 8u);
            q[8 * b] = lo.x; q[8 * b + 1] = lo.y; q[8 * b + 2] = lo.z; q[8 * b + 3] = lo.w;
            q[8 * b + 4] = hi.x; q[8 * b + 5] = hi.y; q[8 * b + 6] = hi.z; q[8 * b + 7] = hi.w;
        }
        // each nibble of block b, renormalising before its first and third bits
#pragma unroll
        for (u32 b = 0; b < 2 * W::NB; b++) {
            const u32 x = (v >> (8u * (W::NB - 1u - b / 2u))) & 255u, nib = (b & 1u) ? x & 15u : x >> 4;
            u32 j = 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(k & 1)) e.renorm(so);
                const u32 bit = (nib >> (3 - k)) & 1u;
                u32 pw = q[8 * b];                             // o1b_pick on block b
#pragma unroll
                for (u32 s2 = 1; s2 < 8; s2++) pw = (j >> 1) == s2 ? q[8 * b + s2] : pw;
                const u32 p = (j & 1u) ? pw >> 16 : pw & 0xffffu;
                trc_rcbe(e, p, bit);
                blk[b][j] = (u16)trc_bit_adapt(p, bit);
                j = 2u * j + bit;
            }
        }
        prev = v;
        raw = (int)(tail + 4u * e.cw.nwords) >= lim;
    }
    u32 out_len = 0;
    if (alive) {
        if (!raw) { e.finish(so); out_len = so.wpos; }
        if (raw || out_len >= len) out_len = len;               // (rcs16: a coded length >= the chunk's is stored raw)
        clen[c] = out_len;
    }
    const u32 gs = trc_wave_sum(out_len);
    if (lane == 0) gsum[c0 / 64u + blockIdx.x] = gs;
}

template <int K>
__global__ __launch_bounds__(64) void trc_rc_word_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u32 c0, u32 nround, u16 *__restrict__ models, u8 *__restrict__ out)
{
    using W = WordCfg<K>;
    // (own text: taking this prologue from trc_rc_lane.h changes the generated code, profiles/lanecore_notes.md)
    const u32 lane = trc_lane(), g = c0 / 64u + blockIdx.x, cw0 = g * 64u, c = cw0 + lane;
    const bool alive = c < nchunks && c < c0 + nround;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    const u32 cl = alive ? trc_min(clen[c], len) : 0u;        // a directory entry above the chunk length (corrupt input) reads as raw
    const u32 ex = trc_wave_incl_scan(cl) - cl;
    const u64 off = trc_group_base(goff, gsum, g) + ex;
    const u32 nel = len / W::ES, tail = len - nel * W::ES;
    const bool coded = alive && cl != len && cl >= tail;
    u8 *const dst = out + (u64)c * chunk;

    if (coded) {
        u16 *const m = models + (u64)(c - c0) * (W::TREES * WORD_TREE_U16);
        const u8 *s = payload + off;
        for (u32 i = 0; i < tail; i++) dst[nel * W::ES + i] = s[i];
        s += tail;
        const u32 sl = cl - tail, lim = sl >= 4u ? sl - 4u : 0u;   // no read from beyond the chunk's stream (corrupt input: re-reads its end)
        u32 rpos = 8u;
        u64 range = ~(u64)0, code = ((u64)*(const u32_a1 *)s << 32) | *(const u32_a1 *)(s + trc_min(4u, lim));
        // one nibble: the 15 nodes it may visit are in q; returns the nibble
        auto get_nibble = [&](const u32 (&q)[8], u16 *blk) __attribute__((always_inline)) -> u32 {
            u32 j = 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!(k & 1) && range < TRC_TOP32) {
                    range <<= 32;
                    code = code << 32 | *(const u32_a1 *)(s + trc_min(rpos, lim));
                    rpos += 4u;
                }
                const u32 p = o1b_pick(q, j);
                const u64 cut = (range >> TRC_PROB_BITS) * p;
                const u32 bit = code < cut ? 1u : 0u;
                range = bit ? cut : range - cut;
                code = bit ? code : code - cut;
                blk[j] = (u16)trc_bit_adapt(p, bit);
                j = 2u * j + bit;
            }
            return j - 16u;
        };
        u32 qf[8];                                             // block 0 of the next word's first tree
        u16 *tf = m + W::first(0) * WORD_TREE_U16;
        word_load_block(qf, tf);
        u32 acc = 0;
        for (u32 i = 0; i < nel; i++) {
            u32 r = 0;
#pragma unroll
            for (u32 d = 0; d < W::NB; d++) {
                u32 q[8];
                u16 *const t = d == 0 ? tf : m + W::tree(d, r) * WORD_TREE_U16;
                if (d == 0) {
#pragma unroll
                    for (u32 k = 0; k < 8; k++) q[k] = qf[k];
                } else word_load_block(q, t);
                const u32 hi = get_nibble(q, t);
                u16 *const t2 = t + 16u * (1u + hi);
                word_load_block(q, t2);
                r = r << 8 | hi << 4 | get_nibble(q, t2);
                if (d + 1u == W::KNOW) {                        // the next word's first tree: bits of the bytes decoded so far
                    tf = m + W::first(r << (8u * (W::NB - 1u - d))) * WORD_TREE_U16;
                    word_load_block(qf, tf);
                }
            }
            if constexpr (W::ES == 4) *(u32 *)(dst + 4u * i) = r;
            else {
                acc |= (r & 0xffffu) << (16u * (i & 1u));
                if (i & 1u) { *(u32 *)(dst + 2u * (i & ~1u)) = acc; acc = 0; }
            }
        }
        if constexpr (W::ES == 2)                               // ragged end (the last chunk only): byte stores, nothing past n
            for (u32 pos = (nel * 2u) & ~3u; pos < nel * 2u; pos++) dst[pos] = (u8)(acc >> (8u * (pos & 3u)));
    }
    trc_wave_copy_raw(__ballot(alive && cl == len && len != 0), off, len, out + (u64)cw0 * chunk, chunk, payload);
}

size_t trc_word_model_bytes(int k) { return (size_t)word_tree_count(k) * WORD_TREE_U16 * 2u; }

size_t trc_word_slots(int k, size_t nchunks)
{
    static const size_t budget = [] {                          // tuning aid: a lower budget (never a higher one)
        const char *e = getenv("TRC_WORD_BUDGET");
        const size_t b = e ? (size_t)strtoull(e, nullptr, 10) : 0;
        return b && b < (size_t)TRC_WORD_MODEL_BUDGET ? b : (size_t)TRC_WORD_MODEL_BUDGET;
    }();
    size_t slots = budget / trc_word_model_bytes(k) / 64u * 64u;
    if (slots < 64u) slots = 64u;
    return nchunks < slots ? nchunks : slots;
}

template <int K>
static void word_launch(bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk, const TrcWork &w,
                        uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
    const size_t slots = trc_word_slots(K, w.nchunks), mb = trc_word_model_bytes(K);
    for (size_t c0 = 0; c0 < w.nchunks; c0 += slots) {
        const uint32_t nround = (uint32_t)(w.nchunks - c0 < slots ? w.nchunks - c0 : slots);
        trc_o1bit_fill(w.model, nround * mb, s);
        const dim3 grid((nround + 63u) / 64u);
        if (dec) TRC_LAUNCH_TIMED(trc_rc_word_dec_kernel<K>, grid, dim3(64), 0, s,
                                  d_src, d_clen_in, w.goff, w.gsum, (u64)n, chunk, w.nchunks, (u32)c0, nround, (u16 *)w.model, d_out);
        else TRC_LAUNCH_TIMED(trc_rc_word_enc_kernel<K>, grid, dim3(64), 0, s,
                              d_src, (u64)n, chunk, w.nchunks, (u32)c0, nround, (u16 *)w.model, w.scratch, w.stride, d_clen, w.gsum);
    }
}

static void word_dispatch(int k, bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk,
                          const TrcWork &w, uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
#define WORD_CASE(i) case i: word_launch<i>(dec, d_src, d_clen_in, n, chunk, w, d_clen, d_out, s); break;
    switch (k) {
    WORD_CASE(0) WORD_CASE(1) WORD_CASE(2) WORD_CASE(3)
    default: break;
    }
#undef WORD_CASE
}

void trc_launch_word_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    word_dispatch(c.k, false, d_in, nullptr, n, chunk, w, d_clen, nullptr, s);
}
void trc_launch_word_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                         const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    word_dispatch(c.k, true, d_payload, d_clen, n, chunk, w, nullptr, d_out, s);
}
