// trc_rc_lane.h -- the lane-per-chunk core of the bitwise range coders (trc_rc_o1bit.hip, trc_rc_int.hip, trc_rc_bvlc.hip,
// trc_rc_word.hip, trc_rc_nib.hip): one lane codes one chunk, 64 chunks per wave, one wave per workgroup.
//
// Arithmetic = the reference's "s" predictor on rc_s.c's geometry: 64-bit range, 32-bit words (RcEnc, trc_rc.h), 15-bit
// probabilities of a ONE bit, all 0x4000 at chunk start, update mbc_s.h:53-55, bit step rcbe_ / rcbd_ (turborc_.h:417-452).
// A family decides where its renormalisations fall (they are part of the bit stream) and which model entry a bit uses.  Here
// is what the families take from one place: the chunk a lane owns, the decoder's directory read and raw copy, the probability
// update, the LDS model fill and the encoder's bit step.  A kernel takes a piece only where its gfx950 code stays the same;
// profiles/lanecore_notes.md lists, per kernel, what is taken and what is kept as the kernel's own text, and why the
// decoder's state and the encoder's tail are shared by no kernel.
#pragma once
#include "trc_rc.h"

// Chunk c = c0 + lane of the workgroup's wave, whose first chunk is c0 = 64 blockIdx.x; lanes past nchunks are not alive and have
// length 0.
struct TrcLaneEnc {
    u32 lane, c, c0;
    bool alive;
    u32 len;
};
__device__ __forceinline__ TrcLaneEnc trc_lane_enc(u64 n, u32 chunk, u32 nchunks)
{
    const u32 lane = trc_lane(), c0 = blockIdx.x * 64u, c = c0 + lane;
    const bool alive = c < nchunks;
    const u32 len = !alive ? 0u : c + 1u < nchunks ? chunk : (u32)(n - (u64)c * chunk);
    return { lane, c, c0, alive, len };
}

// The decoder's lane: the same, with the chunk's payload length cl (a directory entry above the chunk length, corrupt input,
// reads as raw) and payload offset off.  A chunk with cl == len is raw; whether any other is decodable (`coded`) is the
// family's to say.
struct TrcLaneDec {
    u32 lane, c, c0;
    bool alive;
    u32 len, cl;
    u64 off;
};
__device__ __forceinline__ TrcLaneDec trc_lane_dec(u64 n, u32 chunk, u32 nchunks, const u32 *clen, const u64 *goff, const u32 *gsum)
{
    const auto [lane, c, c0, alive, len] = trc_lane_enc(n, chunk, nchunks);
    const u32 cl = alive ? trc_min(clen[c], len) : 0u;
    const u32 ex = trc_wave_incl_scan(cl) - cl;
    const u64 off = trc_group_base(goff, gsum, blockIdx.x) + ex;
    return { lane, c, c0, alive, len, cl, off };
}

// the wave's raw chunks, copied by the whole wave (every lane calls this, whatever its own chunk is)
__device__ __forceinline__ void trc_lane_copy_raw(const TrcLaneDec &l, u32 chunk, const u8 *payload, u8 *out)
{
    trc_wave_copy_raw(__ballot(l.alive && l.cl == l.len && l.len != 0), l.off, l.len, out + (u64)l.c0 * chunk, chunk, payload);
}

// the probability update of every model entry (mbc_s.h:53-55)
__device__ __forceinline__ u32 trc_bit_adapt(u32 p, u32 bit) { return (p - (((p - (bit << 15)) >> 5) + bit)) & 0xffffu; }

// The wave's model block in LDS: E entries as [entry][lane] u16 (the lanes' reads of one entry are one access; entry a of the
// lane at ((u16 *)smem + lane)[a * 64]), all 0x4000.  128 E bytes of dynamic LDS.
template <u32 E>
__device__ __forceinline__ void trc_lds_fill(u8 *smem, u32 lane)
{
    for (u32 i = lane; i < E * 32u; i += 64u) ((u32 *)smem)[i] = 0x40004000u;
    __syncthreads();
}

// rcbe_: one bit at probability p, no renormalisation.  Between two renormalisations `low` grows by less than the range at
// the first, so RcEnc's carry test (mark > low) holds for several bits as for one; the reference's trees renormalise before
// every second bit (mb_o0.h:27-41: _RCENORM1 is empty, _RCENORM2 a renormalisation on this geometry).
__device__ __forceinline__ void trc_rcbe(RcEnc &e, u32 p, u32 bit)
{
    const u64 cut = (e.range >> TRC_PROB_BITS) * p;
    e.low += bit ? 0 : cut;
    e.range = bit ? cut : e.range - cut;
}
