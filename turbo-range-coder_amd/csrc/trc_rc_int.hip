// trc_rc_int.hip -- adaptive gamma and Rice integer coders on the bitwise range coder, "s" predictor: codecs TRC_RCG8 ..
// TRC_RCRZ32 (rcgsenc8 .. rcrzsdec32, reference rc_.c:464-842, `turborc -e26/27/28/29`).
//
// Per chunk the payload is exactly what the reference function returns for that slice, with one exception: a chunk shorter
// than one element (only a final chunk can be one) is stored raw (the reference returns its tail bytes plus an empty 4-byte
// flush, more than the chunk).  Geometry as TRC_RCB / TRC_RCX1: 64-bit range, 32-bit words, 15-bit probabilities, all 0x4000
// at chunk start, update mbc_s.h:53-55, and a renormalisation before EVERY bit (mbu_enc -> rcbenc, turborc_.h:410-466).
// Element coding (mb_vint.h:56-186), x the element (8/16-bit coders) or zigzag(x - prev) (the z coders, prev = 0 at chunk start,
// wrap at the element width):
//   gamma 8/16   mbgenc: x+1 == 1 -> bit 1 on mg0; else bit 0 on mg0, gb = bsr(x+1), gb-1 zeros and a one on mgu[0..gb-1],
//                the low gb bits of x+1, MSB first, on mgb[gb-1][gb-1..0]
//   gamma 32     mbgenc32 (GQMAX32 = 12, no mg0): q = bsr64(x+1); q > 12: unary 12+qb on mgu with qb = bits of q-12, then its
//                qb-1 low bits on mgb[0]; else unary q; then the low q bits of x+1 on mgb[bsr(q+1)+1]
//   Rice         mbrenc32 (RICEMAX = 12) with k = RICEK(ema) = bsr(ema+1): q = x >> k, unary / escape as gamma 32, then the low
//                k bits of x on mgb[bsr(q+1)+1]; ema = EMA(n, ema, a, x) (rcutil_.h:126, rounded, 64-bit): (6, 63) for rcrs8/16 and
//                rcrzs16/32, (4, 15) for rcrzs8, (8, 255) for rcrs32 with one ema per context CXR(prev) = (u8)(prev >> 23)
// The 16/32-bit coders copy the len % es tail bytes to the FRONT of the payload (INDEC, rcutil_.h:134); the raw test (OVERFLOW,
// rcutil_.h:130) runs after every element and counts them.
//
// Model.  Only the entries an input can reach are kept, in a flat layout: mg0 at 0, mgu at 1 .. U, mgb row r at 1 + U + r*C,
// R rows.  Reachable (x < 2^W; k <= bsr(max ema + 1), the ema never exceeds the largest element):
//   gamma 8/16   U = W (the one of gb-1 zeros lands on mgu[W-1]), R = C = W                  8: 73 entries, 16: 273
//   gamma 32     q <= 32, q-12 <= 20 -> qb <= 5, unary <= 17: U = 18; rows 0 .. bsr(33)+1 = 6: R = 7; C = 32    243
//   Rice 8       k <= 8, q <= 255, qb <= 8: U = 21; rows 0 .. bsr(256)+1 = 9: R = 10; C = 8                     102
//   Rice 16      k <= 16, q <= 65535, qb <= 16: U = 29; R = 18; C = 16                                        318
//   Rice 32      k <= 31, q < 2^32, qb <= 32: U = 45; R = 33; C = 31 (q = 2^32-1 only with k = 0: no mantissa)  1069
// The coders of up to 318 entries keep it in LDS, the two 32-bit Rice coders (1069 entries; rcrs32 also 256 ema words) in the
// workspace, each per-wave block [entry][lane] (u16), so the lanes' reads of one entry are one access.  trc_rc_int_fill_kernel
// resets the workspace blocks.
// Decoder bounds (a corrupt payload neither leaves the lane's model nor spins): the unary walk stops at mgu[U-1] whatever the
// bit (`unary` below); the escape reads qb-1 <= U-14 bits into row 0 (< C for every variant); the gamma-32 quotient is clamped
// to 32, the Rice mantissa row to R-1 and k to C; every loop runs at most a fixed count; stream reads stop at the chunk's end.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_launch.h"

// KIND: 0 gamma, 1 gamma on zigzag deltas, 2 Rice, 3 Rice on zigzag deltas; ES: element bytes
template <int KIND, int ES>
struct IntCfg {
    static constexpr bool RICE = KIND >= 2, ZZ = KIND & 1, G32 = !RICE && ES == 4, CTX = KIND == 2 && ES == 4;
    static constexpr u32 W = 8u * ES;
    static constexpr u32 U = !RICE ? (ES == 4 ? 18u : W) : ES == 1 ? 21u : ES == 2 ? 29u : 45u;
    static constexpr u32 R = !RICE ? (ES == 4 ? 7u : W) : ES == 1 ? 10u : ES == 2 ? 18u : 33u;
    static constexpr u32 C = !RICE ? (ES == 4 ? 32u : W) : ES == 1 ? 8u : ES == 2 ? 16u : 31u;
    static constexpr u32 E = 1u + U + R * C;                   // model entries
    static constexpr bool LDS = !(RICE && ES == 4);
    static constexpr u32 EN = KIND == 3 && ES == 1 ? 4u : KIND == 2 && ES == 4 ? 8u : 6u;     // EMA(EN, ema, 2^EN - 1, x)
    static constexpr u32 MGU = 1u, MGB = 1u + U;
};

#define INT_CTX_EMA 256u                                        // rcrs32: ema words per lane (CXR is a byte)

__global__ __launch_bounds__(256) void trc_rc_int_fill_kernel(u32 *__restrict__ p, u64 words, u32 v)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (u64)gridDim.x * blockDim.x) p[i] = v;
}

__device__ __forceinline__ u32 int_bsr(u32 x) { return 31u - (u32)__clz((int)x); }           // (x == 0: ~0u)
__device__ __forceinline__ u32 int_ema(u32 n, u32 ema, u32 x)
{
    const u64 a = (1ull << n) - 1ull;
    return (u32)(((u64)ema * a + (u64)x + (1ull << (n - 2))) >> n);
}
template <int ES>
__device__ __forceinline__ u32 int_zz_enc(u32 d)                // zigzag at the element width
{
    constexpr u32 W = 8u * ES, M = ES == 4 ? 0xffffffffu : (1u << W) - 1u;
    d &= M;
    const u32 s = (d >> (W - 1)) & 1u;
    return ((d << 1) ^ (0u - s)) & M;
}
template <int ES>
__device__ __forceinline__ u32 int_zz_dec(u32 x)
{
    constexpr u32 M = ES == 4 ? 0xffffffffu : (1u << (8 * ES)) - 1u;
    x &= M;
    return ((x >> 1) ^ (0u - (x & 1u))) & M;
}
template <int ES>
__device__ __forceinline__ u32 int_elem(const u8 *p)
{
    return ES == 1 ? (u32)*p : ES == 2 ? (u32)*(const u16 *)p : *(const u32 *)p;
}

// models: per-wave blocks of E x 64 u16 (LDS: the workgroup's own block); emas: per-wave blocks of 256 x 64 u32 (rcrs32)
template <int KIND, int ES>
__global__ __launch_bounds__(64) void trc_rc_int_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models, u32 *__restrict__ emas,
    u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ clen, u32 *__restrict__ gsum)
{
    using K = IntCfg<KIND, ES>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const auto [lane, c, c0, alive, len] = trc_lane_enc(n, chunk, nchunks);
    const u32 nel = len / ES, tail = len - nel * ES;
    const int lim = trc_rc_limit(len);
    u16 *m;
    if constexpr (K::LDS) {
        m = (u16 *)smem + lane;
        trc_lds_fill<K::E>(smem, lane);
    } else m = models + (u64)blockIdx.x * K::E * 64u + lane;
    u32 *const ema_t = K::CTX ? emas + (u64)blockIdx.x * INT_CTX_EMA * 64u + lane : nullptr;
    const u8 *src = in + (u64)c * chunk;
    u8 *const dst = scratch + (u64)c * stride;
    IntOut so; so.start(dst, tail);
    for (u32 i = 0; i < tail; i++) dst[i] = src[nel * ES + i];
    RcEnc e; e.start();

    auto bit = [&](u32 a, u32 b) __attribute__((always_inline)) {
        e.renorm(so);
        const u32 p = m[a * 64u];
        trc_rcbe(e, p, b);
        m[a * 64u] = (u16)trc_bit_adapt(p, b);
    };
    auto unary = [&](u32 cnt) __attribute__((always_inline)) {     // cnt zeros and a one on mgu[0..cnt]
        for (u32 u = 0; u < cnt; u++) bit(K::MGU + u, 0);
        bit(K::MGU + cnt, 1);
    };
    auto binary = [&](u32 row, u64 x, u32 nb) __attribute__((always_inline)) {   // the low nb bits of x, MSB first, on mgb[row]
        for (u32 g = nb; g-- > 0;) bit(K::MGB + row * K::C + g, (u32)(x >> g) & 1u);
    };
    // the quotient q of gamma 32 / Rice: unary, or unary 12+qb and the escape bits
    auto quot = [&](u32 q) __attribute__((always_inline)) {
        if (q > 12u) {
            const u32 qx = q - 12u, qb = int_bsr(qx) + 1u;
            unary(12u + qb);
            binary(0, qx, qb - 1u);
        } else unary(q);
    };

    bool raw = alive && nel == 0u;                             // shorter than one element: stored raw
    u32 prev = 0, ema = 0;
    for (u32 i = 0; alive && !raw && i < nel; i++) {
        const u32 v = int_elem<ES>(src + i * ES);
        const u32 x = K::ZZ ? int_zz_enc<ES>(v - prev) : v;
        prev = v;
        if constexpr (!K::RICE && !K::G32) {
            const u32 x1 = x + 1u;
            if (x1 == 1u) bit(0, 1);
            else {
                bit(0, 0);
                const u32 gb = int_bsr(x1);
                unary(gb - 1u);
                binary(gb - 1u, x1, gb);
            }
        } else if constexpr (K::G32) {
            const u64 x1 = (u64)x + 1u;
            const u32 q = 63u - (u32)__clzll((long long)x1);
            quot(q);
            binary(int_bsr(q + 1u) + 1u, x1, q);
        } else {
            const u32 k = int_bsr(ema + 1u), q = x >> k;
            quot(q);
            binary(q + 1u ? int_bsr(q + 1u) + 1u : 0u, x, k);  // (q = 2^32-1 only with k = 0: no bits)
            if constexpr (K::CTX) {
                u32 *const t = ema_t + (x >> 23 & 255u) * 64u;
                ema = int_ema(K::EN, *t, x);
                *t = ema;
            } else ema = int_ema(K::EN, ema, x);
        }
        raw = (int)(tail + 4u * e.cw.nwords) >= lim;
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

template <int KIND, int ES>
__global__ __launch_bounds__(64) void trc_rc_int_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models, u32 *__restrict__ emas, u8 *__restrict__ out)
{
    using K = IntCfg<KIND, ES>;
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const TrcLaneDec L = trc_lane_dec(n, chunk, nchunks, clen, goff, gsum);
    const auto [lane, c, c0, alive, len, cl, off] = L;
    const u32 nel = len / ES, tail = len - nel * ES;
    const bool coded = alive && cl != len && cl >= tail;
    u16 *m;
    if constexpr (K::LDS) {
        m = (u16 *)smem + lane;
        // (own text: trc_lds_fill of trc_rc_lane.h changes this kernel's generated code)
        for (u32 i = lane; i < K::E * 32u; i += 64u) ((u32 *)smem)[i] = 0x40004000u;
        __syncthreads();
    } else m = models + (u64)blockIdx.x * K::E * 64u + lane;
    u8 *const dst = out + (u64)c * chunk;

    if (coded) {
        u32 *const ema_t = K::CTX ? emas + (u64)blockIdx.x * INT_CTX_EMA * 64u + lane : nullptr;
        const u8 *s = payload + off;
        for (u32 i = 0; i < tail; i++) dst[nel * ES + i] = s[i];
        s += tail;
        const u32 sl = cl - tail, lim = sl >= 4u ? sl - 4u : 0u;   // no read from beyond the chunk's stream (corrupt input: re-reads its end)
        u32 rpos = 8u;
        u64 range = ~(u64)0, code = ((u64)*(const u32_a1 *)s << 32) | *(const u32_a1 *)(s + trc_min(4u, lim));
        auto bit = [&](u32 a) __attribute__((always_inline)) -> u32 {
            if (range < TRC_TOP32) {
                range <<= 32;
                code = code << 32 | *(const u32_a1 *)(s + trc_min(rpos, lim));
                rpos += 4u;
            }
            const u32 p = m[a * 64u];
            const u64 cut = (range >> TRC_PROB_BITS) * p;
            const u32 b = code < cut ? 1u : 0u;
            range = b ? cut : range - cut;
            code = b ? code : code - cut;
            m[a * 64u] = (u16)trc_bit_adapt(p, b);
            return b;
        };
        auto unary = [&]() __attribute__((always_inline)) -> u32 {   // zeros before the one; stops at mgu[U-1] whatever the bit
            u32 u = 0;
            while (!bit(K::MGU + u) && u < K::U - 1u) u++;
            return u;
        };
        auto binary = [&](u32 row, u64 x, u32 nb) __attribute__((always_inline)) -> u64 {   // nb bits below x, MSB first
            for (u32 g = nb; g-- > 0;) x = x << 1 | bit(K::MGB + row * K::C + g);
            return x;
        };
        auto quot = [&]() __attribute__((always_inline)) -> u32 {    // the quotient after escape reconstruction
            u32 q = unary();
            if (q > 12u) q = (u32)binary(0, 1, q - 13u) + 12u;   // qb - 1 = q - 13 <= U - 14 bits
            return q;
        };
        u32 prev = 0, ema = 0, acc = 0;
        for (u32 i = 0; i < nel; i++) {
            u32 x;
            if constexpr (!K::RICE && !K::G32) {
                if (bit(0)) x = 0;
                else {
                    const u32 ub = unary();
                    x = (u32)binary(ub, 1, ub + 1u) - 1u;
                }
            } else if constexpr (K::G32) {
                const u32 q = trc_min(quot(), 32u);
                x = (u32)(binary(int_bsr(q + 1u) + 1u, 1, q) - 1u);
            } else {
                const u32 k = trc_min(int_bsr(ema + 1u), K::C), q = quot();
                const u32 row = q + 1u ? trc_min(int_bsr(q + 1u) + 1u, K::R - 1u) : 0u;
                x = (u32)binary(row, q, k);
                if constexpr (K::CTX) {
                    u32 *const t = ema_t + (x >> 23 & 255u) * 64u;
                    ema = int_ema(K::EN, *t, x);
                    *t = ema;
                } else ema = int_ema(K::EN, ema, x);
            }
            const u32 v = K::ZZ ? prev + int_zz_dec<ES>(x) : x;
            prev = v;
            if constexpr (ES == 4) *(u32 *)(dst + 4u * i) = v;
            else {
                acc |= (v & (ES == 1 ? 0xffu : 0xffffu)) << (8u * ES * (i & (4u / ES - 1u)));
                if ((i & (4u / ES - 1u)) == 4u / ES - 1u) { *(u32 *)(dst + ES * (i & ~(4u / ES - 1u))) = acc; acc = 0; }
            }
        }
        if constexpr (ES < 4)                                   // ragged end (the last chunk only): byte stores, nothing past n
            for (u32 pos = (nel * ES) & ~3u; pos < nel * ES; pos++) dst[pos] = (u8)(acc >> (8u * (pos & 3u)));
    }
    trc_lane_copy_raw(L, chunk, payload, out);
}

// codec index k = codec - TRC_RCG8: 0-2 gamma 8/16/32, 3-5 gamma zigzag, 6-8 Rice, 9-11 Rice zigzag
static inline uint32_t int_es(int k) { return 1u << (k % 3); }

size_t trc_int_model_bytes(int k, size_t ngroups)
{
    if (k < 6 || int_es(k) != 4) return 0;                     // in LDS
    const size_t e = k == 8 ? IntCfg<2, 4>::E : IntCfg<3, 4>::E;
    return ngroups * 64u * (e * 2u + (k == 8 ? 4u * INT_CTX_EMA : 0u));
}

template <int KIND, int ES>
static void int_launch(bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk, const TrcWork &w,
                       uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
    using K = IntCfg<KIND, ES>;
    u32 *emas = nullptr;
    const uint32_t lds = K::LDS ? K::E * 128u : 0u;
    if (!K::LDS) {
        const u64 mw = (u64)w.ngroups * K::E * 32u;            // u32 words of counters
        hipLaunchKernelGGL(trc_rc_int_fill_kernel, dim3(2048), dim3(256), 0, s, (u32 *)w.model, mw, 0x40004000u);
        if (K::CTX) {
            emas = (u32 *)w.model + mw;
            hipLaunchKernelGGL(trc_rc_int_fill_kernel, dim3(1024), dim3(256), 0, s, emas, (u64)w.ngroups * INT_CTX_EMA * 64u, 0u);
        }
    }
    if (dec) TRC_LAUNCH_TIMED((trc_rc_int_dec_kernel<KIND, ES>), dim3(w.ngroups), dim3(64), lds, s,
                              d_src, d_clen_in, w.goff, w.gsum, (u64)n, chunk, w.nchunks, (u16 *)w.model, emas, d_out);
    else TRC_LAUNCH_TIMED((trc_rc_int_enc_kernel<KIND, ES>), dim3(w.ngroups), dim3(64), lds, s,
                          d_src, (u64)n, chunk, w.nchunks, (u16 *)w.model, emas, w.scratch, w.stride, d_clen, w.gsum);
}

static void int_dispatch(int k, bool dec, const uint8_t *d_src, const uint32_t *d_clen_in, size_t n, uint32_t chunk,
                         const TrcWork &w, uint32_t *d_clen, uint8_t *d_out, hipStream_t s)
{
#define INT_CASE(i, KD, ES) case i: int_launch<KD, ES>(dec, d_src, d_clen_in, n, chunk, w, d_clen, d_out, s); break;
    switch (k) {
    INT_CASE(0, 0, 1) INT_CASE(1, 0, 2) INT_CASE(2, 0, 4)
    INT_CASE(3, 1, 1) INT_CASE(4, 1, 2) INT_CASE(5, 1, 4)
    INT_CASE(6, 2, 1) INT_CASE(7, 2, 2) INT_CASE(8, 2, 4)
    INT_CASE(9, 3, 1) INT_CASE(10, 3, 2) INT_CASE(11, 3, 4)
    default: break;
    }
#undef INT_CASE
}

void trc_launch_int_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    int_dispatch(c.k, false, d_in, nullptr, n, chunk, w, d_clen, nullptr, s);
}
void trc_launch_int_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                        const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    int_dispatch(c.k, true, d_payload, d_clen, n, chunk, w, nullptr, d_out, s);
}
