// trc_rc_nib.hip -- the bitwise nibble and varint byte coders on the bitwise range coder, "s" predictor: codecs TRC_RC4,
// TRC_RC4C, TRC_RCU3 (rc4senc / rc4csenc / rcu3senc and their decoders, reference rc_.c:141-184, 442-462; `turborc -n -e41`,
// `-n -e40`, `-e17`).
//
// Per chunk the payload is exactly what the reference function returns for that slice (the element is a byte: no exception).
// Geometry as TRC_RCB: 64-bit range, 32-bit words, 15-bit probabilities, all 0x4000 at chunk start, update mbc_s.h:53-55.
//   rc4s   mb4enc (mb_o0.h:181-187) of in[i] & 15: a 15-node tree, index (16 | x) >> (k + 1) for bit k = 3 .. 0
//   rc4cs  mb4senc (mb_o0.h:232-238): the same walk, every bit at the initial probability, nothing adapts: no model at all
//   rcu3s  mbu3enc (mb_vint.h:266-279) of in[i]: flag f0 = 1: x == 0; else f0 = 0, x -= 1 and f1 = 1: mb3enc(x) for x < 8; else
//          f1 = 0, x -= 8 and f2 = 0: mb5enc(x) for x < 32; else f2 = 1, x -= 32: mb8enc(x) (x <= 214)
// Renormalisation points (part of the bit stream): RC_SIZE 64, RC_IO 32, RC_BITS 15 make _RCENORM1 empty and _RCENORM2 a
// renormalisation (mb_o0.h:27-41), so a tree of nb bits renormalises before its bits nb-1, nb-3, .. (every second one, the
// first included: mb3enc R - R, mb4enc R - R -, mb5enc R - R - R, mb8enc R - R - R - R -); the flag bits and every bit of
// mb4senc go through rcbenc (turborc_.h:430-433), which renormalises before the bit.  The decoders mirror this (mb*dec,
// _mbu3dec: if_rc0 renormalises per flag).  Between two renormalisations `low` grows by less than the range at the first, so
// RcEnc's carry test holds for two bits as for one.
// The raw test (OVERFLOW, rcutil_.h:130) runs after every symbol: a chunk of 9 bytes or fewer is always raw; the final flush
// is not tested.  rc4s / rc4cs code the low nibble of every byte; their decoders return in[i] & 15 (the reference's behaviour).
//
// Model: per-wave LDS block [entry][lane] (u16), so the lanes' reads of one entry are one access: rc4s 16 entries (entry 0 is
// never read: 2 KiB per wave), rcu3s 3 flags + 8 + 32 + 256 (entry 0 of each tree never read: 299 entries, 37.4 KiB per wave).
// Decoder bounds (a corrupt payload neither leaves the lane's model nor spins): a tree index is 1 followed by at most nb-1
// decoded bits (< 2^nb), a flag index is 0 .. 2; every loop runs a fixed count; stream reads stop at the chunk's clen (a
// directory entry above the chunk length reads as raw), writes at the chunk's length.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_launch.h"

// KIND: 0 rc4s, 1 rc4cs, 2 rcu3s
template <int KIND>
struct NibCfg {
    static constexpr bool U3 = KIND == 2, ADAPT = KIND != 1;
    static constexpr u32 T3 = 3u, T5 = 3u + 8u, T8 = 3u + 8u + 32u;               // rcu3s: the trees behind the three flags
    static constexpr u32 E = KIND == 0 ? 16u : KIND == 1 ? 0u : T8 + 256u;          // model entries
};

template <int KIND>
__global__ __launch_bounds__(64) void trc_rc_nib_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ clen,
    u32 *__restrict__ gsum)
{
    using K = NibCfg<KIND>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const auto [lane, c, c0, alive, len] = trc_lane_enc(n, chunk, nchunks);
    const int lim = trc_rc_limit(len);
    u16 *const m = (u16 *)smem + lane;
    // (own text: trc_lds_fill of trc_rc_lane.h changes this kernel's generated code)
    if constexpr (K::E != 0u) {
        for (u32 i = lane; i < K::E * 32u; i += 64u) ((u32 *)smem)[i] = 0x40004000u;
        __syncthreads();
    }
    const u8 *src = in + (u64)c * chunk;                         // 16-byte aligned (d_in is, a chunk is a multiple of 64)
    LaneOutDirect so; so.start(scratch + (u64)c * stride);
    RcEnc e; e.start();

    auto bit = [&](u32 a, u32 b) __attribute__((always_inline)) {  // rcbe: no renormalisation (own text: trc_rcbe changes enc<0>)
        const u32 p = K::ADAPT ? (u32)m[a * 64u] : TRC_PROB_ONE >> 1;
        const u64 cut = (e.range >> TRC_PROB_BITS) * p;
        e.low += b ? 0 : cut;
        e.range = b ? cut : e.range - cut;
        if constexpr (K::ADAPT) m[a * 64u] = (u16)trc_bit_adapt(p, b);
    };
    auto flag = [&](u32 a, u32 b) __attribute__((always_inline)) { e.renorm(so); bit(a, b); };   // rcbenc

    bool raw = false;
    u32 w = 0;
    for (u32 i = 0; alive && !raw && i < len; i++) {
        if ((i & 3u) == 0u) w = *(const u32 *)(src + i);          // (the last word may reach into the buffer's slack)
        u32 x = w & 0xffu, nb = 4u, base = 0u;
        w >>= 8;
        if constexpr (K::U3) {
            nb = 0u;
            flag(0, x == 0u);
            if (x != 0u) {
                x -= 1u;
                flag(1, x < 8u);
                nb = 3u; base = K::T3;
                if (x >= 8u) {
                    x -= 8u;
                    flag(2, x >= 32u);
                    nb = 5u; base = K::T5;
                    if (x >= 32u) { x -= 32u; nb = 8u; base = K::T8; }
                }
            }
        } else x &= 15u;
        const u32 t = (1u << nb) | x;
        for (u32 k = 0; k < nb; k++) {                             // bit nb-1-k on node t >> (nb - k)
            if (!K::ADAPT || !(k & 1u)) e.renorm(so);
            bit(base + (t >> (nb - k)), (t >> (nb - 1u - k)) & 1u);
        }
        raw = (int)(4u * e.cw.nwords) >= lim;
    }
    u32 out_len = 0;
    if (alive) {
        if (raw) out_len = len;
        else { e.finish(so); out_len = so.wpos; }
        clen[c] = out_len;
    }
    const u32 gs = trc_wave_sum(out_len);
    if (lane == 0) gsum[blockIdx.x] = gs;
}

template <int KIND>
__global__ __launch_bounds__(64) void trc_rc_nib_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u8 *__restrict__ out)
{
    using K = NibCfg<KIND>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const TrcLaneDec L = trc_lane_dec(n, chunk, nchunks, clen, goff, gsum);
    const auto [lane, c, c0, alive, len, cl, off] = L;
    const bool coded = alive && cl != len;
    u16 *const m = (u16 *)smem + lane;
    // (own text: trc_lds_fill of trc_rc_lane.h changes this kernel's generated code)
    if constexpr (K::E != 0u) {
        for (u32 i = lane; i < K::E * 32u; i += 64u) ((u32 *)smem)[i] = 0x40004000u;
        __syncthreads();
    }
    u8 *const dst = out + (u64)c * chunk;

    if (coded) {
        const u8 *s = payload + off;
        const u32 lim = cl >= 4u ? cl - 4u : 0u;                 // no read from beyond the chunk's stream (corrupt input: re-reads its end)
        u32 rpos = 8u;
        u64 range = ~(u64)0, code = ((u64)*(const u32_a1 *)s << 32) | *(const u32_a1 *)(s + trc_min(4u, lim));
        auto renorm = [&]() __attribute__((always_inline)) {
            if (range < TRC_TOP32) {
                range <<= 32;
                code = code << 32 | *(const u32_a1 *)(s + trc_min(rpos, lim));
                rpos += 4u;
            }
        };
        auto bit = [&](u32 a) __attribute__((always_inline)) -> u32 {   // rcbd: no renormalisation
            const u32 p = K::ADAPT ? (u32)m[a * 64u] : TRC_PROB_ONE >> 1;
            const u64 cut = (range >> TRC_PROB_BITS) * p;
            const u32 b = code < cut ? 1u : 0u;
            range = b ? cut : range - cut;
            code = b ? code : code - cut;
            if constexpr (K::ADAPT) m[a * 64u] = (u16)trc_bit_adapt(p, b);
            return b;
        };
        auto flag = [&](u32 a) __attribute__((always_inline)) -> u32 { renorm(); return bit(a); };
        u32 acc = 0;
        for (u32 i = 0; i < len; i++) {
            u32 nb = 4u, base = 0u, add = 0u;
            if constexpr (K::U3) {
                nb = 0u;
                if (!flag(0)) {
                    nb = 3u; base = K::T3; add = 1u;
                    if (!flag(1)) {
                        const u32 f2 = flag(2);
                        nb = f2 ? 8u : 5u; base = f2 ? K::T8 : K::T5; add = f2 ? 41u : 9u;
                    }
                }
            }
            u32 t = 1u;
            for (u32 k = 0; k < nb; k++) {
                if (!K::ADAPT || !(k & 1u)) renorm();
                t = t << 1 | bit(base + t);                        // t < 2^nb before the step: inside the tree
            }
            const u32 v = ((t & ((1u << nb) - 1u)) + add) & 0xffu;
            acc |= v << (8u * (i & 3u));
            if ((i & 3u) == 3u) { *(u32 *)(dst + (i & ~3u)) = acc; acc = 0; }
        }
        for (u32 pos = len & ~3u; pos < len; pos++) dst[pos] = (u8)(acc >> (8u * (pos & 3u)));   // ragged end (the last chunk only)
    }
    trc_lane_copy_raw(L, chunk, payload, out);
}

// codec index k = codec - TRC_RC4: 0 rc4s, 1 rc4cs, 2 rcu3s
template <int KIND>
static void nib_launch(bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk, const TrcWork &w,
                       uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
    const uint32_t lds = NibCfg<KIND>::E * 128u;
    if (dec) TRC_LAUNCH_TIMED((trc_rc_nib_dec_kernel<KIND>), dim3(w.ngroups), dim3(64), lds, s,
                              d_src, d_clen_in, w.goff, w.gsum, (u64)n, chunk, w.nchunks, d_out);
    else TRC_LAUNCH_TIMED((trc_rc_nib_enc_kernel<KIND>), dim3(w.ngroups), dim3(64), lds, s,
                          d_src, (u64)n, chunk, w.nchunks, w.scratch, w.stride, d_clen, w.gsum);
}

static void nib_dispatch(int k, bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk,
                         const TrcWork &w, uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
#define NIB_CASE(i) case i: nib_launch<i>(dec, d_src, d_clen_in, n, chunk, w, d_clen, d_out, s); break;
    switch (k) {
    NIB_CASE(0) NIB_CASE(1) NIB_CASE(2)
    default: break;
    }
#undef NIB_CASE
}

void trc_launch_nibbit_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    nib_dispatch(c.k, false, d_in, nullptr, n, chunk, w, d_clen, nullptr, s);
}
void trc_launch_nibbit_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                           const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    nib_dispatch(c.k, true, d_payload, d_clen, n, chunk, w, nullptr, d_out, s);
}
