// trc_rc_ss.hip -- the byte-level bitwise coders on the dual-rate "ss" predictor: codecs TRC_RCSS, TRC_RC4SS, TRC_RC4CSS,
// TRC_RCU3SS (rcssenc / rc4ssenc / rc4cssenc / rcu3ssenc and their decoders: the functions of rc_.c:37-58, 141-184, 442-462
// as rc_ss.c builds them; `turborc -pss -e1`, `-n -e41`, `-n -e40`, `-e17`, parameters `-rNM`).
//
// Per chunk the payload is exactly what the reference function returns for that slice when called with the same two
// parameters (prm0, prm1), each 1 .. 15.
//
// The predictor.  A context holds TWO 16-bit counters P and Q, both estimates of the probability of a ONE bit scaled to 2^16,
// both 0x8000 at chunk start.  A bit is coded at their mean, p = (P + Q) >> 1 (1 <= p <= 0xffff), a 16-bit probability:
// cut = (range >> 16) * p; a ONE keeps low and takes cut as its range, a ZERO adds cut to low and keeps range - cut (the
// decoder: the bit is ONE where code < cut).  Then each counter moves towards the bit at its own rate: a ZERO takes X >> s away, a ONE adds
// (0xffff - X) >> s, with s = prm0 for P and s = prm1 for Q (X never leaves [1, 0xffff] for s >= 1, so p is never 0).  The
// counter with the small shift follows the data fast, the one with the large shift settles accurately; a chunk's cold model
// learns at the fast one's pace.  rc4css uses no counter at all: every bit at p = 0x8000, whatever the parameters.
// Everything else is the geometry of the "s" build (trc_rc_nib.hip): 64-bit range, 32-bit words, a renormalisation once the
// range is below 2^32.  With 16-bit probabilities (64 - 32) / 2 >= 16 still holds and (64 - 32) / 4 >= 16 still does not, so a
// tree of nb bits renormalises before its bits nb-1, nb-3, .. as before (mb3enc R - R, mb4enc R - R -, mb5enc R - R - R,
// mb8enc R - R - R - R -); after a renormalisation the range is at least 2^32, one bit leaves at least 2^16 and the second
// at least 1: two bits per renormalisation never empty the range.  Flags and every bit of rc4css renormalise before the bit.
//   rcss    the mb8enc walk of in[i]: a 255-node tree, index (256 | x) >> (k + 1) for bit k = 7 .. 0
//   rc4ss   the mb4enc walk of in[i] & 15: a 15-node tree
//   rc4css  the same walk at the fixed probability
//   rcu3ss  flag f0 = 1: x == 0; else f0 = 0, x -= 1 and f1 = 1: a 3-bit tree for x < 8; else f1 = 0, x -= 8 and f2 = 0: a
//           5-bit tree for x < 32; else f2 = 1, x -= 32: an 8-bit tree (x <= 214)
// The raw test runs after every symbol (written bytes >= len * 255 / 256 - 8: a chunk of 9 bytes or fewer is always raw), the
// final flush is not tested.  The two nibble coders' decoders return in[i] & 15.
//
// Kernels: one lane per chunk, 64 chunks per wave, one wave per workgroup (trc_rc_lane.h, trc_lane_io.h).  Model: per-wave LDS
// block [entry][lane], an entry is ONE u32 (P | Q << 16): a bit costs one LDS read and one write, and the lanes' accesses to
// one entry are one row of 256 bytes.  rc4ss 16 entries (4 KiB per wave), rcss 256 (64 KiB), rcu3ss 3 flags + 8 + 32 + 256 =
// 299 (74.75 KiB), rc4css none.  Entry 0 of every tree is never read and is kept all the same: rcss and rcu3ss have two waves
// per CU of its 160 KiB with it and without it (a third would need 53.3 KiB or less).  prm0 and prm1 are kernel arguments, the
// same for the whole wave.
// Decoder bounds (a corrupt payload neither leaves the lane's model nor spins): a tree index is 1 followed by at most nb-1
// decoded bits (< 2^nb), a flag index is 0 .. 2; every loop runs a fixed count; stream reads stop at the chunk's clen (a
// directory entry above the chunk length reads as raw), writes at the chunk's length.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_launch.h"

#define TRC_SS_BITS 16u
#define TRC_SS_HALF 0x8000u

// KIND: 0 rc4ss, 1 rc4css, 2 rcu3ss, 3 rcss
template <int KIND>
struct SsCfg {
    static constexpr bool U3 = KIND == 2, ADAPT = KIND != 1;
    static constexpr u32 NB = KIND == 3 ? 8u : 4u;                                  // bits of the one tree (rcu3ss picks per symbol)
    static constexpr u32 T3 = 3u, T5 = 3u + 8u, T8 = 3u + 8u + 32u;               // rcu3ss: the trees behind the three flags
    static constexpr u32 E = KIND == 0 ? 16u : KIND == 1 ? 0u : KIND == 2 ? T8 + 256u : 256u;   // model entries
};

// both counters of an entry towards `bit`, each at its own shift (the halves cannot carry into each other: X stays in 16 bits)
__device__ __forceinline__ u32 trc_ss_adapt(u32 pq, u32 bit, u32 s0, u32 s1)
{
    const u32 P = pq & 0xffffu, Q = pq >> 16;
    const u32 P2 = bit ? P + ((P ^ 0xffffu) >> s0) : P - (P >> s0);
    const u32 Q2 = bit ? Q + ((Q ^ 0xffffu) >> s1) : Q - (Q >> s1);
    return P2 | Q2 << 16;
}
__device__ __forceinline__ u32 trc_ss_prob(u32 pq) { return ((pq & 0xffffu) + (pq >> 16)) >> 1; }

template <int KIND>
__global__ __launch_bounds__(64) void trc_rc_ss_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ clen,
    u32 *__restrict__ gsum, u32 s0, u32 s1)
{
    using K = SsCfg<KIND>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const auto [lane, c, c0, alive, len] = trc_lane_enc(n, chunk, nchunks);
    const int lim = trc_rc_limit(len);
    u32 *const m = (u32 *)smem + lane;
    if constexpr (K::E != 0u) {
        for (u32 i = lane; i < K::E * 64u; i += 64u) ((u32 *)smem)[i] = TRC_SS_HALF | TRC_SS_HALF << 16;
        __syncthreads();
    }
    const u8 *src = in + (u64)c * chunk;                         // 16-byte aligned (d_in is, a chunk is a multiple of 64)
    LaneOutDirect so; so.start(scratch + (u64)c * stride);
    RcEnc e; e.start();

    auto bit = [&](u32 a, u32 b) __attribute__((always_inline)) {  // one bit, no renormalisation
        u32 pq = 0, p = TRC_SS_HALF;
        if constexpr (K::ADAPT) { pq = m[a * 64u]; p = trc_ss_prob(pq); }
        const u64 cut = (e.range >> TRC_SS_BITS) * p;
        e.low += b ? 0 : cut;
        e.range = b ? cut : e.range - cut;
        if constexpr (K::ADAPT) m[a * 64u] = trc_ss_adapt(pq, b, s0, s1);
    };
    auto flag = [&](u32 a, u32 b) __attribute__((always_inline)) { e.renorm(so); bit(a, b); };

    bool raw = false;
    u32 w = 0;
    for (u32 i = 0; alive && !raw && i < len; i++) {
        if ((i & 3u) == 0u) w = *(const u32 *)(src + i);          // (the last word may reach into the buffer's slack)
        u32 x = w & 0xffu, nb = K::NB, base = 0u;
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
        } else if constexpr (K::NB == 4u) x &= 15u;
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
__global__ __launch_bounds__(64) void trc_rc_ss_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u8 *__restrict__ out, u32 s0, u32 s1)
{
    using K = SsCfg<KIND>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const TrcLaneDec L = trc_lane_dec(n, chunk, nchunks, clen, goff, gsum);
    const auto [lane, c, c0, alive, len, cl, off] = L;
    const bool coded = alive && cl != len;
    u32 *const m = (u32 *)smem + lane;
    if constexpr (K::E != 0u) {
        for (u32 i = lane; i < K::E * 64u; i += 64u) ((u32 *)smem)[i] = TRC_SS_HALF | TRC_SS_HALF << 16;
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
        auto bit = [&](u32 a) __attribute__((always_inline)) -> u32 {   // one bit, no renormalisation
            u32 pq = 0, p = TRC_SS_HALF;
            if constexpr (K::ADAPT) { pq = m[a * 64u]; p = trc_ss_prob(pq); }
            const u64 cut = (range >> TRC_SS_BITS) * p;
            const u32 b = code < cut ? 1u : 0u;
            range = b ? cut : range - cut;
            code = b ? code : code - cut;
            if constexpr (K::ADAPT) m[a * 64u] = trc_ss_adapt(pq, b, s0, s1);
            return b;
        };
        auto flag = [&](u32 a) __attribute__((always_inline)) -> u32 { renorm(); return bit(a); };
        u32 acc = 0;
        for (u32 i = 0; i < len; i++) {
            u32 nb = K::NB, base = 0u, add = 0u;
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

// codec index k: 0 rc4ss, 1 rc4css, 2 rcu3ss, 3 rcss; the parameters come with the call (TrcWork::ss_prm = prm0 | prm1 << 8)
template <int KIND>
static void ss_launch(bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk, const TrcWork &w,
                      uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
    const uint32_t lds = SsCfg<KIND>::E * 256u, s0 = w.ss_prm & 0xffu, s1 = w.ss_prm >> 8 & 0xffu;
    if (lds >= 65536u) {
        if (dec) TRC_RAISE_LDS_ONCE((trc_rc_ss_dec_kernel<KIND>), lds);
        else TRC_RAISE_LDS_ONCE((trc_rc_ss_enc_kernel<KIND>), lds);
    }
    if (dec) TRC_LAUNCH_TIMED((trc_rc_ss_dec_kernel<KIND>), dim3(w.ngroups), dim3(64), lds, s,
                              d_src, d_clen_in, w.goff, w.gsum, (u64)n, chunk, w.nchunks, d_out, s0, s1);
    else TRC_LAUNCH_TIMED((trc_rc_ss_enc_kernel<KIND>), dim3(w.ngroups), dim3(64), lds, s,
                          d_src, (u64)n, chunk, w.nchunks, w.scratch, w.stride, d_clen, w.gsum, s0, s1);
}

static void ss_dispatch(int k, bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk,
                        const TrcWork &w, uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
#define SS_CASE(i) case i: ss_launch<i>(dec, d_src, d_clen_in, n, chunk, w, d_clen, d_out, s); break;
    switch (k) {
    SS_CASE(0) SS_CASE(1) SS_CASE(2) SS_CASE(3)
    default: break;
    }
#undef SS_CASE
}

void trc_launch_ssbit_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    ss_dispatch(c.k, false, d_in, nullptr, n, chunk, w, d_clen, nullptr, s);
}
void trc_launch_ssbit_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                          const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    ss_dispatch(c.k, true, d_payload, d_clen, n, chunk, w, nullptr, d_out, s);
}
