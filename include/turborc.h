/*
 * turborc.h -- drop-in prototypes for the range-coder side of the hot path, served by
 * libturborc_hip.so (MI355X / gfx950).  Own text; the prototypes mirror the reference's
 * include/turborc.h so that a TurboRC-style harness compiles and links unchanged:
 *
 *   cdf_t                          reference include/turborc.h:497
 *   cdfini                         reference include/turborc.h:500   (rccdf.c:50-68)
 *   rccdfsenc / rccdfs{b,l,vb,vl}dec   include/turborc.h:502-506     (rccdf.c:71-122)
 *   rccdfs2enc / rccdfs{l,b}2dec   include/turborc.h:508-510         (rccdf.c:125-184)
 *   rccdfenc / rccdfdec            include/turborc.h:513-514         (rccdf.c:187-211)
 *   rcsenc / rcsdec                include/turborc.h:62-63           (rc_.c:37-58)
 *   rccsenc / rccsdec              include/turborc.h:65-66           (rc_.c:186-209)
 *   rcxsenc / rcxsdec              include/turborc.h:71-72           (rc_.c:372-400)
 *   rcgsenc8/16/32 .. rcrzsdec32   include/turborc.h:128-155         (rc_.c:464-842)
 *   rcvsenc16 .. rcvgzsdec32       include/turborc.h:121-132         (rc_.c:1012-1336)
 *   rcsenc16 .. rcc2sdec32         include/turborc.h:77-90           (rc_.c:60-138, 248-342)
 *
 * Calling convention (reference include/turborc.h:46-59), unchanged:
 *   encoders: `out` holds at least inlen bytes (+ the harness's usual slack); the return value is
 *             the compressed length, or exactly inlen when the data is incompressible, in which
 *             case out[0..inlen) is a copy of the input and the caller must memcpy instead of
 *             calling the decoder;
 *   decoders: return outlen.
 * Stream format: the TRC1 chunk container of include/trc_hip.h -- every chunk's payload is
 * bit-identical to what the reference function returns for that chunk alone.
 * Errors (no HIP device, HIP failure, malformed container): message on stderr, trc_last_error(),
 * return value 0 (cdfini: -1).  The library never calls exit() and has no CPU coding path.
 */
#ifndef TURBORC_H_
#define TURBORC_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef unsigned short cdf_t;

int cdfini(unsigned char *in, size_t inlen, cdf_t *cdf, unsigned cdfnum);

/* static-CDF range coder, one stream (reference rccdf.c:71-122).  The four reference decoders differ
 * only in how they search the CDF (linear / binary / division+linear / division+binary) and decode
 * the same stream; all four names are served by the same kernel. */
size_t rccdfsenc(unsigned char *src, size_t srclen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsldec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsbdec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsvldec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsvbdec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);

/* the one-stream static coder with a 32-bit range and 16-bit I/O (reference rccdf.c:648-694, include/turborc.h:521-526;
 * `turborc -e44`).  A different bitstream from rccdfsenc.  The reference decoders divide through a reciprocal table;
 * both names decode the same stream here (exact division). */
size_t rccdfsmenc(unsigned char *src, size_t srclen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsmldec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsmbdec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);

/* static-CDF range coder, two interleaved streams (reference rccdf.c:125-184; `turborc -e45`) */
size_t rccdfs2enc(unsigned char *src, size_t srclen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsl2dec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);
size_t rccdfsb2dec(unsigned char *src, size_t dstlen, unsigned char *dst, cdf_t *cdf, unsigned cdfnum);

/* adaptive-CDF byte range coder (reference rccdf.c:187-211; `turborc -e46`) */
size_t rccdfenc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rccdfdec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* adaptive-CDF byte range coder, hi nibbles on stream 0 / lo nibbles on stream 1 (reference rccdf.c:213-249,
 * include/turborc.h:515-516; `turborc -e47`) */
size_t rccdfienc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rccdfidec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* the `turborc -n` coders: adaptive-CDF range coder on values 0..15, one CDF16 table (reference rccdf.c:250-275 and,
 * two interleaved streams, rccdf.c:277-323; include/turborc.h:517-519,528-529; harness ids 46/47 when the data is
 * nibble-valued, turborc.c:499-501).  Values above 15 are outside the reference's contract; their low nibble is coded. */
size_t rccdf4enc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rccdf4dec(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdf4ienc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rccdf4idec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* Turbo-VLC integer coders over the adaptive CDF range coder (reference rccdf.c:391-632, include/turborc.h:536-549;
 * `turborc -e50/52/53` on 16- or 32-bit input): u = 6-bit exponent, v = 7-bit exponent, vz = v on the zigzag of the
 * delta to the previous element.  inlen/outlen are BYTES (multiples of the element size). */
size_t rccdfuenc16(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rccdfudec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfuenc32(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rccdfudec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfvenc16(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rccdfvdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfvenc32(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rccdfvdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfvzenc16(unsigned char *src, size_t srclen, unsigned char *dst);  size_t rccdfvzdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfvzenc32(unsigned char *src, size_t srclen, unsigned char *dst);  size_t rccdfvzdec32(unsigned char *src, size_t dstlen, unsigned char *dst);

/* "vnibble" coders (reference rccdf.c:326-390, include/turborc.h:531-534; `turborc -e48 / -e49`): a byte becomes one to
 * three CDF16 symbols on three adaptive tables (0-12 | 13,14 + nibble | 15 + two nibbles) -- for data that is mostly small
 * values; the `i` form codes the middle symbols on a second interleaved stream */
size_t rccdfenc8(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rccdfdec8(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccdfienc8(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rccdfidec8(unsigned char *src, size_t dstlen, unsigned char *dst);

/* bitwise order-0 range coder, "s" predictor (reference rc_.c:37-58; `turborc -e1`, file codec 1) */
size_t rcsenc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rcsdec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* bitwise order-1 range coders, "s" predictor: context = the previous byte (reference rc_.c:186-209; `turborc -e2`, file
 * codec 2) and a sliding 8-bit context (rc_.c:372-400, mb_on.h; `turborc -e4`, file codec 4).  Chunks of 16 KiB and more. */
size_t rccsenc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rccsdec(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcxsenc(unsigned char *src, size_t srclen, unsigned char *dst);
size_t rcxsdec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* integer coders on the bitwise range coder, "s" predictor (reference rc_.c:464-842; `turborc -e26/27/28/29`): adaptive gamma
 * (rcgs*), gamma of zigzag deltas (rcgzs*), length-limited Rice (rcrs*) and Rice of zigzag deltas (rcrzs*) of 8 / 16 / 32-bit
 * little-endian elements; a length that is not a multiple of the element size keeps its last bytes uncoded */
size_t rcgsenc8(unsigned char *src, size_t srclen, unsigned char *dst);      size_t rcgsdec8(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcgsenc16(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcgsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcgsenc32(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcgsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcgzsenc8(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcgzsdec8(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcgzsenc16(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcgzsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcgzsenc32(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcgzsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrsenc8(unsigned char *src, size_t srclen, unsigned char *dst);      size_t rcrsdec8(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrsenc16(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcrsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrsenc32(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcrsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrzsenc8(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcrzsdec8(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrzsenc16(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcrzsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcrzsenc32(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcrzsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);

/* Turbo-VLC coders on the bitwise range coder, "s" predictor (reference rc_.c:1012-1336; `turborc -e30/33/35/36`): 16 / 32-bit
 * little-endian elements; the exponent of an element >= 32 is coded with an 8-bit tree (rcvs*, rcvzs*: zigzag deltas) or an
 * adaptive gamma code (rcvgs*, rcvgzs*), its mantissa bits are stored verbatim; a length that is not a multiple of the element
 * size keeps its last bytes uncoded */
size_t rcvsenc16(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcvsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvsenc32(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rcvsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvzsenc16(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rcvzsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvzsenc32(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rcvzsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvgsenc16(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rcvgsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvgsenc32(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rcvgsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvgzsenc16(unsigned char *src, size_t srclen, unsigned char *dst);  size_t rcvgzsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcvgzsenc32(unsigned char *src, size_t srclen, unsigned char *dst);  size_t rcvgzsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);

/* bitwise word coders, "s" predictor (reference rc_.c:60-138, 248-342; `turborc -e6/7/8`): 16 / 32-bit little-endian words,
 * each byte coded with an 8-bit tree picked by the bytes above it (rcc*: and the top bits of the previous word); a length that
 * is not a multiple of the word size keeps its last bytes uncoded */
size_t rcsenc16(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcsdec16(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcsenc32(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rccsenc32(unsigned char *src, size_t srclen, unsigned char *dst);    size_t rccsdec32(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rcc2senc32(unsigned char *src, size_t srclen, unsigned char *dst);   size_t rcc2sdec32(unsigned char *src, size_t dstlen, unsigned char *dst);

/* bitwise nibble coders, "s" predictor (reference rc_.c:141-184; `turborc -n -e41 / -e40`): an adaptive 15-node tree (rc4s*)
 * and the same walk with probabilities that never adapt (rc4cs*).  They code src[i] & 15 and the decoders return src[i] & 15:
 * input values above 15 lose their high nibble, as in the reference. */
size_t rc4senc(unsigned char *src, size_t srclen, unsigned char *dst);      size_t rc4sdec(unsigned char *src, size_t dstlen, unsigned char *dst);
size_t rc4csenc(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rc4csdec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* structured 3/5/8-bit varint of a byte, "s" predictor (reference rc_.c:442-462, mb_vint.h:266-300; `turborc -e17`): 0 is one
 * flag bit, 1..8 two flags and a 3-bit tree, 9..40 three flags and a 5-bit tree, 41..255 three flags and an 8-bit tree */
size_t rcu3senc(unsigned char *src, size_t srclen, unsigned char *dst);     size_t rcu3sdec(unsigned char *src, size_t dstlen, unsigned char *dst);

/* the same four byte-level coders on the dual-rate "ss" predictor (reference rc_ss.c; `turborc -pss -rNM` with -e1, -n -e41,
 * -n -e40, -e17): every context holds two 16-bit counters that adapt with the shifts prm0 and prm1, a bit is coded at their
 * mean.  prm0, prm1: 1 .. 15 each (the reference's defaults: 5, 6; TRC_SS_PRM_DEFAULT in trc_hip.h), anything else returns 0.
 * The container's header records them; a decoder uses its arguments and returns 0 where the header holds other ones.
 * rc4css* codes every bit at probability 1/2 whatever the parameters. */
size_t rcssenc(unsigned char *src, size_t srclen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rcssdec(unsigned char *src, size_t dstlen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rc4ssenc(unsigned char *src, size_t srclen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rc4ssdec(unsigned char *src, size_t dstlen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rc4cssenc(unsigned char *src, size_t srclen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rc4cssdec(unsigned char *src, size_t dstlen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rcu3ssenc(unsigned char *src, size_t srclen, unsigned char *dst, unsigned prm0, unsigned prm1);
size_t rcu3ssdec(unsigned char *src, size_t dstlen, unsigned char *dst, unsigned prm0, unsigned prm1);

#ifdef __cplusplus
}
#endif
#endif
