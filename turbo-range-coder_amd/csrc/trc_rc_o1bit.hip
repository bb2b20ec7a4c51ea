// trc_rc_o1bit.hip -- bitwise order-1 range coders with the "s" predictor: codecs TRC_RCC1 (rccsenc / rccsdec) and
// TRC_RCX1 (rcxsenc / rcxsdec).
//
// Per chunk the payload is exactly what the reference function returns for that slice.  Both share the TRC_RCB geometry
// (rc_s.c: 64-bit range, 32-bit I/O, 15-bit probabilities, all 0x4000 at chunk start, update mbc_s.h:53-55
// p -= ((p - (bit << 15)) >> 5) + bit, raw when OVERFLOW rcutil_.h:130 fires) and differ in the context rule:
//   RCC1  rc_.c:186-209, mb8enc / mb8dec mb_o0.h:89-112: the previous byte (0 at chunk start) selects one of 256 trees of
//         255 nodes; renormalisation only before bits 7, 5, 3, 1;
//   RCX1  rc_.c:372-400, mbcenc / mbcdec mb_on.h:27-60 with MBC_C = 8: a sliding context cx (0 at chunk start, four bits
//         shifted in per nibble); a nibble's row is m[cx & 255] (high nibble) or m[256 + (cx & 255)] (low nibble, cx already
//         holding the high nibble), its four nodes ((w4 << k | path) & 15) << 2 | (3 - k) with w4 = (cx >> 8) & 15;
//         renormalisation before every bit.
//
// One lane = one chunk = one range-coder state; 64 chunks per wave, one wave per workgroup.  The models do not fit in LDS
// (RCC1 136 KiB, RCX1 64 KiB per lane) and live in the workspace in HBM, one block per chunk (w.model, as TRC_ANSO1 keeps
// its models); trc_rc_o1bit_fill_kernel sets them to 0x4000 before the coder runs.
//   RCC1 row layout (272 x u16 per context = the 17 x 32 B of TRC_O1_MODEL_BYTES): block 0 holds the 15 nodes of the
//   high-nibble tree at slots 1..15, block 1 + h the 15 nodes under high nibble h at slots 1..15 (node j of a four-level
//   subtree: 1, 2..3, 4..7, 8..15).  RCX1 keeps the reference's own [512][64] layout.
// Per nibble both sides work on the 15 nodes the nibble may visit: the decoder reads all of them at once (RCC1: one 32-byte
// block; RCX1: 15 independent u16 reads, their addresses a function of w4), so a byte costs two dependent rounds of loads
// instead of eight; the probabilities are picked from registers as the bits are decoded, the adapted ones stored back.
// The encoder knows every node from the byte; it reads, codes and adapts them one bit after the other.
#include "trc_rc_lane.h"
#include "trc_lane_io.h"
#include "trc_launch.h"
#include "trc_tree.h"

#define O1B_RCX_MODEL_BYTES (512u * 64u * 2u)

static inline uint32_t o1b_model_bytes(int ctx) { return ctx ? O1B_RCX_MODEL_BYTES : TRC_O1_MODEL_BYTES; }

__global__ __launch_bounds__(256) void trc_rc_o1bit_fill_kernel(u8 *__restrict__ model, u64 bytes)
{
    const uint4 v = make_uint4(0x40004000u, 0x40004000u, 0x40004000u, 0x40004000u);
    for (u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 16u; i < bytes; i += (u64)gridDim.x * blockDim.x * 16u)
        *(uint4 *)(model + i) = v;
}

// u16 offset, inside the lane's model, of node j (1..15) of the nibble tree: RCC1 `row` is the block, RCX1 the 64-node row
template <int CTX>
__device__ __forceinline__ u32 o1b_node(u32 row, u32 w4, u32 j)
{
    if (CTX == 0) return row + j;
    const u32 k = 31u - __builtin_clz(j);                      // level of node j: bit 3 - k of the nibble
    return row + (((((w4 << k) | (j - (1u << k))) & 15u) << 2) | (3u - k));
}

template <int CTX>
__global__ __launch_bounds__(64) void trc_rc_o1bit_enc_kernel(
    const u8 *__restrict__ in, u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models, u32 mstride,
    u8 *__restrict__ scratch, u32 stride, u32 *__restrict__ clen, u32 *__restrict__ gsum)
{
    // (own text: taking this prologue from trc_rc_lane.h changes the generated code, profiles/lanecore_notes.md)
    const u32 lane = trc_lane(), c = blockIdx.x * 64u + lane;
    const bool alive = c < nchunks;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    const int lim = trc_rc_limit(len);
    u16 *const m = models + (u64)(alive ? c : 0u) * mstride;
    const u8 *src = in + (u64)c * chunk;
    LaneOutDirect so; so.start(scratch + (u64)c * stride);
    RcEnc e; e.start();
    bool raw = alive && lim <= 0;                              // OVERFLOW after the first byte whatever it costs
    u32 cx = 0;

    auto code_bit = [&](u32 a, u32 bit) __attribute__((always_inline)) {
        const u32 p = m[a];
        trc_rcbe(e, p, bit);
        m[a] = (u16)trc_bit_adapt(p, bit);
    };
    // one nibble v in its tree (rows and window as the context rule gives them), renormalising before the bits in `rmask`
    auto code_nibble = [&](u32 row, u32 w4, u32 v, u32 rmask) __attribute__((always_inline)) {
        u32 j = 1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (rmask & (1u << k)) e.renorm(so);
            const u32 bit = (v >> (3 - k)) & 1u;
            code_bit(o1b_node<CTX>(row, w4, j), bit);
            j = 2u * j + bit;
        }
    };

    uint4 q = make_uint4(0, 0, 0, 0);
    u32 i = 0;
    for (; alive && !raw && i < len; i++) {
        if ((i & 15u) == 0) q = *(const uint4 *)(src + i);     // (the input carries TRC_PAD bytes of slack)
        const u32 wd = (i & 8u) ? ((i & 4u) ? q.w : q.z) : ((i & 4u) ? q.y : q.x);
        const u32 x = (wd >> (8 * (i & 3u))) & 255u;
        if (CTX == 0) {
            const u32 row = cx * 272u;
            code_nibble(row, 0, x >> 4, 0x5u);                // renormalise before bits 7 and 5 ...
            code_nibble(row + 16u * (1u + (x >> 4)), 0, x & 15u, 0x5u);   // ... and 3 and 1
            cx = x;
        } else {
            code_nibble((cx & 255u) * 64u, (cx >> 8) & 15u, x >> 4, 0xfu);
            cx = cx << 4 | x >> 4;
            code_nibble((256u + (cx & 255u)) * 64u, (cx >> 8) & 15u, x & 15u, 0xfu);
            cx = cx << 4 | (x & 15u);
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

template <int CTX>
__global__ __launch_bounds__(64) void trc_rc_o1bit_dec_kernel(
    const u8 *__restrict__ payload, const u32 *__restrict__ clen, const u64 *__restrict__ goff, const u32 *__restrict__ gsum,
    u64 n, u32 chunk, u32 nchunks, u16 *__restrict__ models, u32 mstride, u8 *__restrict__ out)
{
    const TrcLaneDec L = trc_lane_dec(n, chunk, nchunks, clen, goff, gsum);
    const auto [lane, c, c0, alive, len, cl, off] = L;
    const bool coded = alive && cl != len;
    u8 *const dst = out + (u64)c * chunk;

    if (coded) {
        u16 *const m = models + (u64)c * mstride;
        const u8 *s = payload + off;
        const u32 lim = cl >= 4u ? cl - 4u : 0u;               // no read from beyond the chunk's stream (corrupt input: re-reads its end)
        u32 rpos = 8u;
        u64 range = ~(u64)0, code = ((u64)trc_ld32_a2(s) << 32) | trc_ld32_a2(s + trc_min(4u, lim));
        auto renorm = [&]() __attribute__((always_inline)) {
            if (range < TRC_TOP32) {
                range <<= 32;
                code = code << 32 | trc_ld32_a2(s + trc_min(rpos, lim));
                rpos += 4u;
            }
        };
        // one nibble: the 15 nodes it may visit are in q (slot j = node j); returns the nibble
        auto get_nibble = [&](const u32 (&q)[8], u32 row, u32 w4, u32 rmask) __attribute__((always_inline)) -> u32 {
            u32 j = 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (rmask & (1u << k)) renorm();
                const u32 p = o1b_pick(q, j);
                const u64 cut = (range >> TRC_PROB_BITS) * p;
                const u32 bit = code < cut ? 1u : 0u;
                range = bit ? cut : range - cut;
                code = bit ? code : code - cut;
                m[o1b_node<CTX>(row, w4, j)] = (u16)trc_bit_adapt(p, bit);
                j = 2u * j + bit;
            }
            return j - 16u;
        };
        auto load_nodes = [&](u32 (&q)[8], u32 row, u32 w4) __attribute__((always_inline)) {
            if (CTX == 0) {
                const uint4 a = *(const uint4 *)(m + row), b = *(const uint4 *)(m + row + 8u);
                q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
            } else {
                u32 v[16];
                v[0] = 0;
#pragma unroll
                for (u32 j = 1; j < 16; j++) v[j] = m[o1b_node<CTX>(row, w4, j)];
#pragma unroll
                for (u32 i = 0; i < 8; i++) q[i] = v[2 * i] | v[2 * i + 1] << 16;
            }
        };
        u32 cx = 0, acc = 0;
        uint4 ob = make_uint4(0, 0, 0, 0);
        for (u32 i = 0; i < len; i++) {
            u32 q[8], x;
            if (CTX == 0) {
                const u32 row = cx * 272u;
                load_nodes(q, row, 0);
                const u32 hi = get_nibble(q, row, 0, 0x5u);
                const u32 row2 = row + 16u * (1u + hi);
                load_nodes(q, row2, 0);
                x = hi << 4 | get_nibble(q, row2, 0, 0x5u);
                cx = x;
            } else {
                u32 row = (cx & 255u) * 64u, w4 = (cx >> 8) & 15u;
                load_nodes(q, row, w4);
                cx = cx << 4 | get_nibble(q, row, w4, 0xfu);
                row = (256u + (cx & 255u)) * 64u; w4 = (cx >> 8) & 15u;
                load_nodes(q, row, w4);
                cx = cx << 4 | get_nibble(q, row, w4, 0xfu);
                x = cx & 255u;
            }
            acc |= x << (8 * (i & 3u));
            if ((i & 3u) == 3u) {
                const u32 k = (i >> 2) & 3u;
                ob.x = k == 0 ? acc : ob.x; ob.y = k == 1 ? acc : ob.y; ob.z = k == 2 ? acc : ob.z; ob.w = k == 3 ? acc : ob.w;
                acc = 0;
                if (k == 3) *(uint4 *)(dst + (i & ~15u)) = ob;
            }
        }
        // ragged end (the last chunk only): byte stores, nothing past n
        const u32 ww[4] = { ob.x, ob.y, ob.z, ob.w };
        for (u32 pos = len & ~15u; pos < len; pos++)
            dst[pos] = (u8)(((pos >> 2) == (len >> 2) ? acc : ww[(pos >> 2) & 3u]) >> (8 * (pos & 3u)));
    }
    trc_lane_copy_raw(L, chunk, payload, out);
}

void trc_o1bit_fill(uint8_t *model, size_t bytes, hipStream_t s)
{
    hipLaunchKernelGGL(trc_rc_o1bit_fill_kernel, dim3(4096), dim3(256), 0, s, model, (u64)bytes);
}

void trc_launch_o1bit_enc(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s)
{
    const uint32_t mb = o1b_model_bytes(c.k);
    trc_o1bit_fill(w.model, (size_t)w.nchunks * mb, s);
    if (c.k) TRC_LAUNCH_TIMED(trc_rc_o1bit_enc_kernel<1>, dim3(w.ngroups), dim3(64), 0, s,
                              d_in, (u64)n, chunk, w.nchunks, (u16 *)w.model, mb / 2u, w.scratch, w.stride, d_clen, w.gsum);
    else TRC_LAUNCH_TIMED(trc_rc_o1bit_enc_kernel<0>, dim3(w.ngroups), dim3(64), 0, s,
                          d_in, (u64)n, chunk, w.nchunks, (u16 *)w.model, mb / 2u, w.scratch, w.stride, d_clen, w.gsum);
}
void trc_launch_o1bit_dec(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                          const TrcWork &w, uint8_t *d_out, hipStream_t s)
{
    const uint32_t mb = o1b_model_bytes(c.k);
    trc_o1bit_fill(w.model, (size_t)w.nchunks * mb, s);
    if (c.k) TRC_LAUNCH_TIMED(trc_rc_o1bit_dec_kernel<1>, dim3(w.ngroups), dim3(64), 0, s,
                              d_payload, d_clen, w.goff, w.gsum, (u64)n, chunk, w.nchunks, (u16 *)w.model, mb / 2u, d_out);
    else TRC_LAUNCH_TIMED(trc_rc_o1bit_dec_kernel<0>, dim3(w.ngroups), dim3(64), 0, s,
                          d_payload, d_clen, w.goff, w.gsum, (u64)n, chunk, w.nchunks, (u16 *)w.model, mb / 2u, d_out);
}
