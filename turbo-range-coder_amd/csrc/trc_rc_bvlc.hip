// trc_rc_bvlc.hip -- Turbo-VLC integer coders on the bitwise range coder, "s" predictor: codecs TRC_RCBV16 .. TRC_RCBVGZ32
// (rcvsenc16 .. rcvgzsdec32, reference rc_.c:1012-1336, `turborc -e30/33/35/36`).
//
// Per chunk the payload is exactly what the reference function returns for that slice:
//     [u32 total][vb: rcvs32 only][len % es tail bytes][range-coder words][mantissa bytes]
// Range coder as TRC_RCB / TRC_RCC1 (64-bit range, 32-bit words, 15-bit probabilities, all 0x4000 at chunk start, update
// mbc_s.h:53-55).  Element rule (VLC_VN8 = 3, VLC_VB8 = 16, include_/vlcbit.h): u = x (or zigzag(x - prev), prev = 0 at chunk
// start, wrap at the element width); u >= 16 + vb becomes the symbol expo(u - vb) + vb and f = bsr(u - vb) - 3 mantissa bits
// (low bits of u - vb), else u is the symbol.  vb = 16, except rcvs32: vb = min(255, 255 - vlcexpo(max of the chunk, 3)),
// 255 for a maximum below 8.  The symbol (<= 127 at 16 bits, <= 255 at 32) is coded with
//   tree   mb8enc (mb_o0.h:89-112): 8 binary decisions from the MSB, renormalising only before bits 7, 5, 3, 1; the tree is
//          selected by prev >> 8 (rcvs16, rcvzs16), prev >> 24 (rcvzs32) or is the only one (rcvs32);
//   gamma  mbgenc (mb_vint.h:85-94) of values <= 255, renormalising before every bit: mg0, unary mgu[0..gb-1], mgb[gb-1].
// Mantissas go MSB-first into a bit string that grows down from the end of the output (LaneBitsDown, trc_vlc.h) and is moved
// behind the range-coder words at the end.  The reference gives up (raw) once op + 12 > out + len - 8 - (mantissa bytes
// flushed) after an element (its local OVERFLOWR), and on OVERFLOW (rcutil_.h:130) of the total.
//
// One lane = one chunk.  Models:
//   gamma      73 entries (mg0, mgu[8], mgb[8][8]: trc_rc_int.hip gamma 8), LDS, per-wave [entry][lane] u16;
//   rcvs32     one tree, LDS, per-wave [slot][lane] u16 in the block layout below (272 slots);
//   context    256 trees per chunk in the workspace (w.model), one row per context in the block layout; reset by
//              trc_rc_bvlc_fill_kernel.  16-bit coders: the symbol is <= 127, so its high nibble is <= 7 and only blocks
//              0..8 are reachable: 144 slots per context (72 KiB per chunk); rcvzs32: 272 slots (136 KiB, as TRC_RCC1).
// Block layout (TRC_RCC1's, trc_rc_o1bit.hip): block 0 holds the 15 nodes of the high-nibble tree at slots 1..15, block 1 + h
// the 15 nodes under high nibble h.  The decoder reads the 15 nodes a nibble may visit at once (one 32-byte block in HBM), so a
// symbol waits on two dependent loads instead of eight; the encoder knows every node from the symbol and loads both blocks
// before it codes.
// Decoder bounds (a corrupt payload neither leaves the lane's model nor its chunk): the 16-bit tree coders take the high
// nibble & 7 for the block; the gamma unary walk stops at mgu[7]; the mantissa length is clamped to 28 bits; the header total
// is clamped to [8, clen] and the mantissa window to the bytes above the chunk's start; range-coder reads stop at clen.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_vlc.h"
#include "trc_tree.h"
#include "trc_launch.h"

// K: 0 rcvs16, 1 rcvs32, 2 rcvzs16, 3 rcvzs32, 4 rcvgs16, 5 rcvgs32, 6 rcvgzs16, 7 rcvgzs32 (= codec - TRC_RCBV16)
template <int K>
struct BvCfg {
    static constexpr u32 ES = (K & 1) ? 4u : 2u;
    static constexpr bool ZZ = (K & 2) != 0, GAMMA = K >= 4, VB = K == 1, CTX = K == 0 || K == 2 || K == 3;
    static constexpr u32 HDR = VB ? 5u : 4u;
    static constexpr u32 ROW = ES == 2 ? 144u : 272u;          // tree slots per context (blocks of 16 u16)
    static constexpr u32 HMASK = ES == 2 ? 7u : 15u;           // reachable high nibbles
    static constexpr u32 LDS_SLOTS = GAMMA ? 73u : VB ? ROW : 0u;
};
#define BV_GAMMA_MGU 1u
#define BV_GAMMA_MGB 9u                                         // mgb[r][g] at 9 + 8 r + g

__global__ __launch_bounds__(256) void trc_rc_bvlc_fill_kernel(u8 *__restrict__ model, u64 bytes)
{
    const uint4 v = make_uint4(0x40004000u, 0x40004000u, 0x40004000u, 0x40004000u);
    for (u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 16u; i < bytes; i += (u64)gridDim.x * blockDim.x * 16u)
        *(uint4 *)(model + i) = v;
}

__device__ __forceinline__ u32 bv_bsr(u32 x) { return 31u - (u32)__clz((int)x); }
template <u32 ES>
__device__ __forceinline__ u32 bv_zz_enc(u32 d) { return vlc_zigzag_enc(d, ES == 4); }
// vb of rcvs32: 255 - vlcexpo(max, 3), clamped to 255 (a maximum below 8 has no exponent)
__device__ __forceinline__ u32 bv_vb32(u32 mx)
{
    if (mx < 8u) return 255u;
    const u32 f = bv_bsr(mx) - 3u, expo = ((f + 1u) << 3) + ((mx >> f) & 7u);
    return 255u - expo;
}

// The byte sink of the encoder: header and tail come first, so the words may be unaligned.  Not IntOut (trc_lane_io.h), which
// takes any offset but 0 for unaligned: rcvs32's 5-byte header and a 3-byte tail make an aligned start here.
struct BvOut {
    u8 *dst;
    u32 wpos;
    bool un;
    __device__ __forceinline__ void start(u8 *d, u32 pos) { dst = d; wpos = pos; un = (pos & 3u) != 0u; }
    __device__ __forceinline__ void put32(u32 v)
    {
        u8 *p = dst + wpos;
        if (un) { p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24); }
        else *(u32 *)p = v;
        wpos += 4u;
    }
    __device__ __forceinline__ void put32_slow(u32 v) { put32(v); }
    __device__ __forceinline__ void put32_if(bool take, u32 v) { if (take) put32(v); }
};

// A lane's tree: slot s at m[s * 64] in LDS (lane-interleaved: LDS = true), at m[s] in the workspace, where the 16 slots of
// a block are read at once into q
template <bool LDS>
struct BvTree {
    u16 *m;
    u32 q[8];
    __device__ __forceinline__ void load(u32 base)
    {
        if constexpr (!LDS) {
            const uint4 a = *(const uint4 *)(m + base), b = *(const uint4 *)(m + base + 8u);
            q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
        }
    }
    __device__ __forceinline__ u32 prob(u32 base, u32 j) const { if constexpr (LDS) return m[(base + j) * 64u]; else return o1b_pick(q, j); }
    __device__ __forceinline__ void store(u32 base, u32 j, u32 v) const { if constexpr (LDS) m[(base + j) * 64u] = (u16)v; else m[base + j] = (u16)v; }
};

template <int K>
__global__ __launch_bounds__(64) void trc_rc_bvlc_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models,
    u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ aux, u32 *__restrict__ clen, u32 *__restrict__ gsum)
{
    using C = BvCfg<K>;
    constexpr u32 ES = C::ES;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    // (own text: taking this prologue from trc_rc_lane.h changes the generated code, profiles/lanecore_notes.md)
    const u32 lane = trc_lane(), c = blockIdx.x * 64u + lane;
    const bool alive = c < nchunks;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    const u32 nel = len / ES, tail = len - nel * ES;
    const int lim = trc_rc_limit(len);
    u16 *m;
    if constexpr (C::LDS_SLOTS != 0) {
        m = (u16 *)smem + lane;
        trc_lds_fill<C::LDS_SLOTS>(smem, lane);
    } else m = models + (u64)(alive ? c : 0u) * (256u * C::ROW);
    const u8 *src = in + (u64)c * chunk;
    u8 *const dst = scratch + (u64)c * stride;
    u32 vb = 16u;
    if constexpr (C::VB) {                                      // the chunk's maximum first (expvb32)
        u32 mx = 0;
        for (u32 i = 0; alive && i < nel; i++) { const u32 x = *(const u32_a1 *)(src + 4u * i); mx = x > mx ? x : mx; }
        vb = bv_vb32(mx);
        if (alive) dst[4] = (u8)vb;
    }
    for (u32 i = 0; alive && i < tail; i++) dst[C::HDR + i] = src[nel * ES + i];
    BvOut so; so.start(dst, C::HDR + tail);
    LaneBitsDown bo; bo.start(dst + stride);
    RcEnc e; e.start();

    auto bit = [&](u16 *p, u32 b) __attribute__((always_inline)) {     // one decision on *p, no renormalisation
        // (own text: trc_rcbe of trc_rc_lane.h changes this kernel's generated code)
        const u32 pr = *p;
        const u64 cut = (e.range >> TRC_PROB_BITS) * pr;
        e.low += b ? 0 : cut;
        e.range = b ? cut : e.range - cut;
        *p = (u16)trc_bit_adapt(pr, b);
    };
    // the tree: both blocks of the symbol's path loaded before the first decision
    auto code_tree = [&](u32 row, u32 s) __attribute__((always_inline)) {
        const u32 hi = s >> 4, lo = s & 15u, row2 = row + 16u * (1u + hi);
        BvTree<C::LDS_SLOTS != 0> ta{m}, tb{m};
        ta.load(row); tb.load(row2);
        auto nibble = [&](const BvTree<C::LDS_SLOTS != 0> &t, u32 base, u32 v) __attribute__((always_inline)) {
            u32 j = 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((k & 1) == 0) e.renorm(so);                 // before bits 7, 5 (3, 1)
                const u32 b = (v >> (3 - k)) & 1u;
                const u32 pr = t.prob(base, j);
                trc_rcbe(e, pr, b);
                t.store(base, j, trc_bit_adapt(pr, b));
                j = 2u * j + b;
            }
        };
        nibble(ta, row, hi);
        nibble(tb, row2, lo);
    };
    auto code_gamma = [&](u32 s) __attribute__((always_inline)) {       // mbgenc of s <= 255
        const u32 x1 = s + 1u;
        e.renorm(so);
        if (x1 == 1u) { bit(m, 1); return; }
        bit(m, 0);
        const u32 gb = bv_bsr(x1);
        for (u32 u = 0; u < gb - 1u; u++) { e.renorm(so); bit(m + (BV_GAMMA_MGU + u) * 64u, 0); }
        e.renorm(so); bit(m + (BV_GAMMA_MGU + gb - 1u) * 64u, 1);
        for (u32 g = gb; g-- > 0;) { e.renorm(so); bit(m + (BV_GAMMA_MGB + 8u * (gb - 1u) + g) * 64u, (x1 >> g) & 1u); }
    };

    bool raw = false;
    u32 prev = 0;
    for (u32 i = 0; alive && !raw && i < nel; i++) {
        const u32 v = ES == 4 ? *(const u32_a1 *)(src + 4u * i) : (u32)*(const u16 *)(src + 2u * i);
        const u32 u = C::ZZ ? bv_zz_enc<ES>(v - prev) : v;
        u32 s = u;
        if (u >= 16u + vb) {
            const u32 y = u - vb, f = bv_bsr(y) - 3u;
            s = ((f + 1u) << 3) + ((y >> f) & 7u) + vb;
            bo.put_if(true, f, y & ((1u << f) - 1u));
        }
        if constexpr (C::GAMMA) code_gamma(s);
        else code_tree(C::CTX ? (ES == 2 ? prev >> 8 : prev >> 24) * C::ROW : 0u, s);
        prev = v;
        // OVERFLOWR: op + 12 > op_, op = out + hdr + tail + words, op_ = out + len - 8 - (mantissa bytes flushed)
        raw = (int)(C::HDR + tail + 4u * e.cw.nwords) + 12 > (int)len - 8 - (int)(bo.total >> 3);
    }
    u32 out_len = 0, la = 0;
    if (alive) {
        if (!raw) {
            e.finish(so);
            la = so.wpos;
            out_len = la + bo.bytes();
            raw = (int)out_len >= lim;                          // OVERFLOW on the total
        }
        if (raw) out_len = len;
    }
    bo.finish(alive && !raw);
    if (alive && !raw) { *(u32 *)dst = out_len; aux[2u * c] = la; }
    if (alive) clen[c] = out_len;
    const u32 gs = trc_wave_sum(out_len);
    if (lane == 0) gsum[blockIdx.x] = gs;
}

template <int K>
__global__ __launch_bounds__(64) void trc_rc_bvlc_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models, u8 *__restrict__ out)
{
    using C = BvCfg<K>;
    constexpr u32 ES = C::ES;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    // (own text: taking this prologue from trc_rc_lane.h changes the generated code, profiles/lanecore_notes.md)
    const u32 lane = trc_lane(), c0 = blockIdx.x * 64u, c = c0 + lane;
    const bool alive = c < nchunks;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    const u32 cl = alive ? trc_min(clen[c], len) : 0u;        // a directory entry above the chunk length (corrupt input) reads as raw
    const u32 ex = trc_wave_incl_scan(cl) - cl;
    const u64 off = trc_group_base(goff, gsum, blockIdx.x) + ex;
    const u32 nel = len / ES, tail = len - nel * ES;
    const bool coded = alive && cl != len && cl >= C::HDR + tail + 4u;   // header, tail and at least one flushed word
    u16 *m;
    if constexpr (C::LDS_SLOTS != 0) {
        m = (u16 *)smem + lane;
        // (own text: trc_lds_fill of trc_rc_lane.h changes this kernel's generated code)
        for (u32 i = lane; i < C::LDS_SLOTS * 32u; i += 64u) ((u32 *)smem)[i] = 0x40004000u;
        __syncthreads();
    } else m = models + (u64)(alive ? c : 0u) * (256u * C::ROW);
    u8 *const dst = out + (u64)c * chunk;

    if (coded) {
        const u8 *const base = payload + off;
        const u32 tot = trc_min(*(const u32_a1 *)base, cl) < 8u ? 8u : trc_min(*(const u32_a1 *)base, cl);   // the bit string ends at base + tot
        const u32 vb = C::VB ? (u32)base[4] : 16u;
        for (u32 i = 0; i < tail; i++) dst[nel * ES + i] = base[C::HDR + i];
        const u8 *const s = base + C::HDR + tail;
        const u32 sl = cl - C::HDR - tail, lim = sl - 4u;      // no read from beyond the chunk (corrupt input: re-reads its end)
        const u8 *const bend = base + tot;
        u32 rpos = 8u, bpos = 0;
        u64 range = ~(u64)0, code = ((u64)*(const u32_a1 *)s << 32) | *(const u32_a1 *)(s + trc_min(4u, lim));
        auto renorm = [&]() __attribute__((always_inline)) {
            if (range < TRC_TOP32) {
                range <<= 32;
                code = code << 32 | *(const u32_a1 *)(s + trc_min(rpos, lim));
                rpos += 4u;
            }
        };
        auto dbit = [&](u32 pr, u32 &b) __attribute__((always_inline)) -> u32 {   // one decision; returns the adapted probability
            const u64 cut = (range >> TRC_PROB_BITS) * pr;
            b = code < cut ? 1u : 0u;
            range = b ? cut : range - cut;
            code = b ? code : code - cut;
            return trc_bit_adapt(pr, b);
        };
        auto get_nibble = [&](u32 blk) __attribute__((always_inline)) -> u32 {
            BvTree<C::LDS_SLOTS != 0> t{m};
            t.load(blk);
            u32 j = 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((k & 1) == 0) renorm();                     // before bits 7, 5 (3, 1)
                u32 b;
                t.store(blk, j, dbit(t.prob(blk, j), b));
                j = 2u * j + b;
            }
            return j - 16u;
        };
        auto get_tree = [&](u32 row) __attribute__((always_inline)) -> u32 {
            const u32 hi = get_nibble(row) & C::HMASK;
            return hi << 4 | get_nibble(row + 16u * (1u + hi));
        };
        auto gbit = [&](u32 a) __attribute__((always_inline)) -> u32 {
            renorm();
            u32 b;
            m[a * 64u] = (u16)dbit(m[a * 64u], b);
            return b;
        };
        auto get_gamma = [&]() __attribute__((always_inline)) -> u32 {
            if (gbit(0)) return 0u;
            u32 ub = 0;
            while (!gbit(BV_GAMMA_MGU + ub) && ub < 7u) ub++;  // stops at mgu[7] whatever the bit
            u32 x = 1;
            for (u32 g = ub + 1u; g-- > 0;) x = x << 1 | gbit(BV_GAMMA_MGB + 8u * ub + g);
            return x - 1u;
        };

        u32 prev = 0, acc = 0;
        for (u32 i = 0; i < nel; i++) {
            u32 x;
            if constexpr (C::GAMMA) x = get_gamma();
            else x = get_tree(C::CTX ? (ES == 2 ? prev >> 8 : prev >> 24) * C::ROW : 0u);
            if (x >= 16u + vb) {
                const u32 e = x - vb, f = trc_min((e >> 3) - 1u, 28u);
                const u32 byteoff = trc_min(bpos >> 3, tot - 8u);  // 8-byte window ending at bend - byteoff, never below the chunk
                const u64 w = *(const u64_a1 *)(bend - 8u - byteoff);
                const u32 ma = (u32)((w << (bpos & 7u)) >> (64u - f));
                bpos += f;
                x = (((8u + (e & 7u)) << f) + ma) + vb;
            }
            u32 v = C::ZZ ? prev + vlc_zigzag_dec(x) : x;
            if constexpr (ES == 2) v &= 0xffffu;
            prev = v;
            if constexpr (ES == 4) *(u32_a1 *)(dst + 4u * i) = v;
            else {
                acc |= v << (16u * (i & 1u));
                if (i & 1u) { *(u32 *)(dst + 2u * (i - 1u)) = acc; acc = 0; }
            }
        }
        if constexpr (ES == 2)                                  // odd element count (the last chunk only): byte stores
            if (nel & 1u) { dst[2u * (nel - 1u)] = (u8)acc; dst[2u * (nel - 1u) + 1u] = (u8)(acc >> 8); }
    }
    trc_wave_copy_raw(__ballot(alive && cl == len && len != 0), off, len, out + (u64)c0 * chunk, chunk, payload);
}

// ------------------------------------------------------------------------------------- launch ---
static inline bool bv_ctx(int k) { return k == 0 || k == 2 || k == 3; }

size_t trc_bvlc_model_bytes(int k, size_t nchunks)
{
    if (!bv_ctx(k)) return 0;                                  // in LDS
    return nchunks * 256u * 2u * (k == 3 ? BvCfg<3>::ROW : BvCfg<0>::ROW);
}

template <int K>
static void bv_launch(bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk, const TrcWork &w,
                      uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
    using C = BvCfg<K>;
    const uint32_t lds = C::LDS_SLOTS * 128u;
    if (C::CTX) hipLaunchKernelGGL(trc_rc_bvlc_fill_kernel, dim3(4096), dim3(256), 0, s, w.model, (u64)trc_bvlc_model_bytes(K, w.nchunks));
    if (dec) TRC_LAUNCH_TIMED((trc_rc_bvlc_dec_kernel<K>), dim3(w.ngroups), dim3(64), lds, s,
                              d_src, d_clen_in, w.goff, w.gsum, (u64)n, chunk, w.nchunks, (u16 *)w.model, d_out);
    else TRC_LAUNCH_TIMED((trc_rc_bvlc_enc_kernel<K>), dim3(w.ngroups), dim3(64), lds, s,
                          d_src, (u64)n, chunk, w.nchunks, (u16 *)w.model, w.scratch, w.stride, w.aux, d_clen, w.gsum);
}

static void bv_dispatch(int k, bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk,
                        const TrcWork &w, uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
#define BV_CASE(i) case i: bv_launch<i>(dec, d_src, d_clen_in, n, chunk, w, d_clen, d_out, s); break;
    switch (k) {
    BV_CASE(0) BV_CASE(1) BV_CASE(2) BV_CASE(3) BV_CASE(4) BV_CASE(5) BV_CASE(6) BV_CASE(7)
    default: break;
    }
#undef BV_CASE
}

void trc_launch_bvlc_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    bv_dispatch(c.k, false, d_in, nullptr, n, chunk, w, d_clen, nullptr, s);
}
void trc_launch_bvlc_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                         const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    bv_dispatch(c.k, true, d_payload, d_clen, n, chunk, w, nullptr, d_out, s);
}
