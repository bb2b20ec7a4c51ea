/*
 * trc_hip.h -- C-ABI of libturborc_hip.so, the MI355X (gfx950) entropy-coding core.
 *
 * Two layers, both plain C (no torch / C++ types in any signature):
 *
 *  (1) the reference's own prototypes -- include/anscdf.h and include/turborc.h in this repo carry
 *      the same signatures as the reference's include/anscdf.h:40-52,70-96 and
 *      include/turborc.h:62-63,497-519 -- host pointers in, host pointers out, so a TurboRC-style
 *      bench harness links unchanged;
 *  (2) the device-resident entry points below (the "*_dev" extension SURVEY.md section 8b allows):
 *      everything stays in HBM, the caller owns all buffers and the HIP stream.  bench.py, the
 *      parity tests and the multi-GPU path use this layer.
 *
 * Unit of parallelism = CHUNK.  The input is cut into `chunk`-byte slices; chunk c is coded by the
 * reference algorithm exactly as if the reference function had been called on that slice alone:
 *
 *        payload(c) == reference_fn(in + c*chunk, len_c)          (bit-exact, incl. raw fallback)
 *
 * clen[c] is the reference function's return value for the slice (== len_c means "stored raw",
 * include/turborc.h:50-53).  Payloads are concatenated without padding in chunk order.
 *
 * Host-pointer calls wrap this in a self-describing container:
 *        trc_container_hdr (32 B) | uint32 clen[nchunks] | payload bytes
 * and keep the reference's return convention (== inlen  =>  out is a raw copy of in).
 *
 * How a host-pointer call runs (csrc/trc_host.inc): a PCIe pipeline per device -- the chunk chosen for the
 * stored size (trc_auto_chunk_codec), slices coded concurrently on two coder streams, pageable memory staged in 8 MB pieces by copy
 * threads, page-locked caller buffers (trc_host_pin) read and written by DMA directly.  For rccdf / rccdfi / anscdf / rcs the input
 * is delivered in striped passes (the k-th part of every chunk per 2-D copy) to an encoder that is already waiting at an arrival
 * gate, and a decoder's output is fetched part by part while it is still running; trc_set_devices / TRC_DEVICES spread a call over
 * several GPUs.  None of this changes a byte of the container.
 */
#ifndef TRC_HIP_H_
#define TRC_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* coder ids (container `codec` byte).  Reference function each one reproduces per chunk: */
enum trc_codec {
    TRC_ANS4S = 1,  /* anscdf4senc / anscdf4sdec   static-CDF rANS, 2 states      anscdf.c:57-85   (-e65) */
    TRC_RCS1  = 2,  /* rccdfsenc   / rccdfs*dec    static-CDF RC, 1 stream        rccdf.c:71-122   (-e42/43) */
    TRC_RCS2  = 3,  /* rccdfs2enc  / rccdfs*2dec   static-CDF RC, 2 streams       rccdf.c:125-184  (-e45) */
    TRC_RCA   = 4,  /* rccdfenc    / rccdfdec      adaptive-CDF byte RC           rccdf.c:187-211  (-e46) */
    TRC_ANSA  = 5,  /* anscdfenc   / anscdfdec     adaptive-CDF byte rANS, 4 st.  anscdf.c:567-605 (-e56) */
    TRC_RCB   = 6,  /* rcsenc      / rcsdec        bitwise order-0 RC             rc_.c:37-58      (-e1)  */
    TRC_RCAI  = 7,  /* rccdfienc   / rccdfidec     adaptive-CDF byte RC, 2 streams rccdf.c:213-249 (-e47) */
    /* the `turborc -n` coders: input values 0..15, one CDF16 table (harness gate m<16, turborc.c:499-520) */
    TRC_RCA4  = 8,  /* rccdf4enc   / rccdf4dec     adaptive-CDF nibble RC         rccdf.c:250-275  (-n -e46) */
    TRC_RCAI4 = 9,  /* rccdf4ienc  / rccdf4idec    ... on 2 interleaved streams   rccdf.c:277-323  (-n -e47) */
    TRC_ANSA4 = 10, /* anscdf4enc  / anscdf4dec    adaptive-CDF nibble rANS, 2 st. anscdf.c:87-133 (-n -e56) */
    TRC_RCSM  = 11, /* rccdfsmenc  / rccdfsm*dec   static-CDF RC, 32-bit range, 16-bit I/O rccdf.c:648-694 (-e44) */
    TRC_ANSO1 = 12, /* anscdf1enc  / anscdf1dec    order-1 adaptive-CDF byte rANS  anscdf.c:607-645 (-e64); 136 KiB of
                       model per chunk in the workspace: use chunks of 4 KiB and more */
    TRC_ANSB  = 13, /* ansbc       / ansbd         bitwise order-0 rANS, 4 states  anscdf.c:672-731 (-e66); chunk <= 8192
                       (one reference block) */
    /* Turbo-VLC integer coders over the adaptive CDF range coder, 16- / 32-bit elements (rccdf.c:391-632; -e50/52/53) */
    TRC_VLCU16 = 14,  TRC_VLCU32 = 15,   /* rccdfuenc16/32, rccdfudec16/32     6-bit exponent */
    TRC_VLCV16 = 16,  TRC_VLCV32 = 17,   /* rccdfvenc16/32, rccdfvdec16/32     7-bit exponent */
    TRC_VLCVZ16 = 18, TRC_VLCVZ32 = 19,  /* rccdfvzenc16/32, rccdfvzdec16/32   7-bit exponent on zigzag deltas */
    /* ... and over the adaptive CDF rANS (anscdf.c:139-483; -e60..63) */
    TRC_VLAU16 = 20,  TRC_VLAUZ16 = 21,  /* anscdfuenc16 / anscdfuzenc16 (+dec)        6-bit exponent, plain / zigzag deltas */
    TRC_VLAV16 = 22,  TRC_VLAVZ16 = 23,  /* anscdfvenc16 / anscdfvzenc16 (+dec)        7-bit exponent */
    TRC_VLAV32 = 24,  TRC_VLAVZ32 = 25,  /* anscdfvenc32 / anscdfvzenc32 (+dec) */
    /* "vnibble" coders: a byte becomes 1-3 CDF16 symbols on three adaptive tables (rccdf.c:326-390, rccdf_.h:76-98) */
    TRC_RCV8 = 26,    /* rccdfenc8  / rccdfdec8    one stream    (-e48) */
    TRC_RCVI8 = 27,   /* rccdfienc8 / rccdfidec8   two streams   (-e49) */
    /* bitwise order-1 range coders, "s" predictor (rc_s.c); a model per chunk in the workspace: chunks of 16 KiB and more */
    TRC_RCC1 = 28,    /* rccsenc    / rccsdec      context = previous byte, 128 KiB model   rc_.c:186-209 (-e2) */
    TRC_RCX1 = 29     /* rcxsenc    / rcxsdec      sliding 8-bit context, 64 KiB model      rc_.c:372-400 (-e4) */
    /* integer coders on the bitwise range coder, "s" predictor (rc_.c:464-842; -e26/27/28/29): adaptive gamma and Rice codes of
       8 / 16 / 32-bit elements, plain or on zigzag deltas.  Parity contract as for every coder (a chunk's payload = the
       reference function on that chunk), with one exception: a chunk shorter than one element (a final chunk of 1 .. es-1
       bytes) is stored raw, where the reference returns its tail bytes plus an empty 4-byte flush (len + 4 bytes). */
    , TRC_RCG8 = 30,  TRC_RCG16 = 31,  TRC_RCG32 = 32,     /* rcgsenc8/16/32   / rcgsdec*    gamma                     (-e26) */
    TRC_RCGZ8 = 33, TRC_RCGZ16 = 34, TRC_RCGZ32 = 35,      /* rcgzsenc8/16/32  / rcgzsdec*   gamma of zigzag deltas    (-e27) */
    TRC_RCR8 = 36,  TRC_RCR16 = 37,  TRC_RCR32 = 38,       /* rcrsenc8/16/32   / rcrsdec*    Rice                      (-e28) */
    TRC_RCRZ8 = 39, TRC_RCRZ16 = 40, TRC_RCRZ32 = 41       /* rcrzsenc8/16/32  / rcrzsdec*   Rice of zigzag deltas     (-e29) */
    /* Turbo-VLC coders on the bitwise range coder, "s" predictor (rc_.c:1012-1336; -e30/33/35/36): 16 / 32-bit elements, an
       element >= 32 becomes an exponent symbol (mb8enc tree or adaptive gamma) and mantissa bits in a reversed bit string.
       The tree coders on 16-bit input and rcvzs32 keep 256 trees per chunk in the workspace (72 / 136 KiB): chunks of 16 KiB
       and more, as for TRC_RCC1.  Id 42 is not assigned. */
    , TRC_RCBV16 = 43,  TRC_RCBV32 = 44,    /* rcvsenc16/32   / rcvsdec16/32     tree, context prev >> 8 (16) / none (32)   (-e30) */
    TRC_RCBVZ16 = 45,   TRC_RCBVZ32 = 46,   /* rcvzsenc16/32  / rcvzsdec16/32    tree of zigzag deltas, prev >> 8 / >> 24  (-e33) */
    TRC_RCBVG16 = 47,   TRC_RCBVG32 = 48,   /* rcvgsenc16/32  / rcvgsdec16/32    gamma exponent                            (-e35) */
    TRC_RCBVGZ16 = 49,  TRC_RCBVGZ32 = 50   /* rcvgzsenc16/32 / rcvgzsdec16/32   gamma exponent of zigzag deltas           (-e36) */
    /* bitwise word coders, "s" predictor (rc_.c:60-138, 248-342; -e6/7/8): every byte of a 16 / 32-bit word coded with an
       mb8enc tree picked by the bytes above it (and, for -e7/-e8, the top bits of the previous word).  136.5 KiB .. 2.26 MiB of
       trees per chunk, held in at most TRC_WORD_MODEL_BUDGET bytes of slots that the chunks use in rounds.  Parity contract
       as for the integer coders (a final chunk shorter than one element is stored raw), plus one exception for rcsenc16,
       which has no OVERFLOW test: a chunk whose coded length would be >= its length is stored raw.  Id 51 is not assigned. */
    , TRC_RCW16 = 52,   /* rcsenc16   / rcsdec16     tree 0 for the high byte, 256 for the low byte          (-e6, 16-bit) */
    TRC_RCW32 = 53,     /* rcsenc32   / rcsdec32     order 0 over the bytes of the word                      (-e6, 32-bit) */
    TRC_RCCW32 = 54,    /* rccsenc32  / rccsdec32    as rcs32, the top byte's tree by (prev >> 25) & 127      (-e7) */
    TRC_RCC2W32 = 55    /* rcc2senc32 / rcc2sdec32   as rcs32, the top byte's tree by (prev >> 20) & 0x7ff    (-e8) */
    /* bitwise nibble and varint byte coders, "s" predictor (rc_.c:141-184, 442-462): one lane per chunk, the whole model in
       LDS, any chunk from TRC_CHUNK_MIN up.  The two nibble coders code in[i] & 15 and their decoders return in[i] & 15, as
       the reference does: feed them values 0..15 (harness gate m<16, turborc.c:493-494).  Ids 56 and 57 are not assigned. */
    , TRC_RC4 = 58,     /* rc4senc    / rc4sdec      adaptive 15-node nibble tree                             (-n -e41) */
    TRC_RC4C = 59,      /* rc4csenc   / rc4csdec     the same walk at probability 1/2: nothing adapts         (-n -e40) */
    TRC_RCU3 = 60       /* rcu3senc   / rcu3sdec     structured 3/5/8-bit varint of a byte, 3 flags + 3 trees  (-e17) */
    /* the byte-level bitwise coders on the dual-rate "ss" predictor (rc_ss.c; `turborc -pss -rNM`): two 16-bit counters per
       context, adapted with the shifts prm0 and prm1, a bit coded at their mean.  One lane per chunk, the whole model in LDS,
       any chunk from TRC_CHUNK_MIN up.  They take no CDF: `cdfnum` of the device and host calls carries TRC_SS_PRM(prm0, prm1),
       and so does the container header.  The id after TRC_RCU3 is not assigned. */
    , TRC_RCSS = 62,    /* rcssenc    / rcssdec      order-0 byte, one 255-node tree                          (-pss -e1) */
    TRC_RC4SS = 63,     /* rc4ssenc   / rc4ssdec     adaptive 15-node nibble tree                             (-pss -n -e41) */
    TRC_RC4CSS = 64,    /* rc4cssenc  / rc4cssdec    the same walk at probability 1/2: nothing adapts         (-pss -n -e40) */
    TRC_RCU3SS = 65     /* rcu3ssenc  / rcu3ssdec    structured 3/5/8-bit varint of a byte                    (-pss -e17) */
};

/* the two shift parameters of the "ss" coders as one `cdfnum` value: each in 1 .. 15 (0 would drive a probability to zero, and
 * the reference's file header has 4 bits per parameter); anything else is TRC_E_ARG */
#define TRC_SS_PRM(p0, p1) ((p0) | (p1) << 8)
#define TRC_SS_PRM_DEFAULT TRC_SS_PRM(5, 6)      /* the reference's defaults (turborc.c:91) */

#define TRC_MAGIC        0x31435254u   /* "TRC1" */
#define TRC_CHUNK_MIN    256u
#define TRC_CHUNK_MAX    65536u        /* chunk must be a multiple of 64 in [MIN, MAX] */
#define TRC_CHUNK_AUTO_MIN 512u        /* the parallel unit is the chunk: at 100 MB per GPU 4096 leaves 1.5 waves per CU (static rANS
                                          163 GB/s), 1024 six (449 GB/s), 512 twelve (590 GB/s); payload ratio on text 63.50 / 63.94 /
                                          64.52 %.  Gigabyte inputs fill the chip at 4096 too, so host-pointer calls pick the size from
                                          the input length (trc_auto_chunk) unless the caller fixes it. */
#define TRC_O1BIT_CHUNK_MIN 16384u     /* TRC_RCC1 / TRC_RCX1, TRC_RCBV16 / TRC_RCBVZ16 / TRC_RCBVZ32, TRC_RCW16 .. TRC_RCC2W32: the smallest chunk the automatic rules and the host-pointer calls use */
#define TRC_WORD_MODEL_BUDGET 4294967296ull  /* TRC_RCW16 .. TRC_RCC2W32: the most workspace one call spends on models.  A call
                                          holds min(chunks, budget / model bytes, in whole waves of 64) of them and codes its
                                          chunks in rounds of that many (profiles/word/word_notes.md) */
#define TRC_ANSB_CHUNK_MAX 8192u       /* TRC_ANSB only: one 8192-byte block of the reference per chunk */
#define TRC_PAD          256u          /* readable slack the device entry points need after every buffer */

typedef struct trc_container_hdr {
    uint32_t magic;      /* TRC_MAGIC */
    uint8_t  codec;      /* enum trc_codec */
    uint8_t  version;    /* 1 */
    uint16_t cdfnum;     /* static coders: alphabet size; ss coders: TRC_SS_PRM; else 0 */
    uint32_t chunk;      /* chunk size in bytes */
    uint32_t nchunks;    /* ceil(n / chunk) */
    uint64_t n;          /* original length */
    uint64_t payload;    /* total payload bytes (sum of clen[]) */
} trc_container_hdr;     /* 32 bytes, little endian */

/* error codes of the *_dev layer (0 = ok) */
enum { TRC_OK = 0, TRC_E_ARG = -1, TRC_E_HIP = -2, TRC_E_WORK = -3, TRC_E_CDF = -4, TRC_E_NODEV = -5 };

/* last error text of the calling thread's most recent failing call ("" if none) */
const char *trc_last_error(void);

/* number of visible HIP devices (0 if the runtime cannot initialise -- no CPU fallback exists) */
int trc_device_count(void);

/* chunk size of the host-pointer (reference-signature) calls, process-wide.  0 = automatic (the default): every call
 * takes trc_auto_chunk_codec(its coder, its input length) -- round 6: the LARGEST chunk of the ladder 512 .. 16 384 whose
 * one-wave time still hides behind the call's PCIe time (budget max(1.7 ms, 0.35 n / 50 GB/s)); what the caller of these
 * functions sees is the stored size and a PCIe-bound rate, and every chunk costs coder state, a directory entry and, for
 * the adaptive coders, a model that starts from scratch.  100 MB: 4096 for the static and the adaptive byte coders, 2048
 * for the bitwise ones; 1 GB: 16 384 (rccdfenc on drift: 26.9 % stored against 26.7 % for one whole-buffer call of the
 * reference; at chunk 512 it was 38.7 %).  Static coders stop at 4096, the bitwise rANS at one reference block (8192), the
 * order-1 rANS never goes below 4096, the bitwise order-1 coders (TRC_RCC1 / TRC_RCX1) never below TRC_O1BIT_CHUNK_MIN:
 * their model starts cold in every chunk, and below ~16 KiB they store more than the order-0 rcsenc.  trc_set_chunk(c) or TRC_CHUNK=c in the environment fix it; trc_set_chunk(0)
 * returns to automatic.  Decoders take the size from the container. */
int      trc_set_chunk(uint32_t chunk);
uint32_t trc_get_chunk(void);
uint32_t trc_auto_chunk(size_t n);                   /* = trc_auto_chunk_codec(TRC_ANS4S, n): the static coders' rule */
uint32_t trc_auto_chunk_codec(int codec, size_t n);
/* The devices of the host-pointer calls.  Default (ndev = 0, TRC_DEVICES unset): the caller's current device.  With a list --
 * trc_set_devices, or TRC_DEVICES="all" / "0,1,2,3" in the environment -- every call is cut into contiguous shards of whole
 * chunk groups, one per list entry, coded at the same time (one pipeline and one host thread per entry) and written straight
 * to their places in the caller's buffer: the result is byte-identical to the one-device container, and it is how a
 * single-threaded caller such as the reference harness (turborc.c:420-579) uses all GPUs of a node.  An entry may repeat (two
 * pipelines on one device: what the tests do on a one-GPU box).  trc_get_devices returns the list length. */
int trc_set_devices(const int *devs, int ndev);
int trc_get_devices(int *devs, int cap);
/* Diagnostic (needs no device): how a host-pointer call of n bytes would run on one pipeline.  chunk 0 = the automatic one; decode 0 / 1;
 * page_locked: the caller's input (encode) or output (decode) buffer is page-locked.  first_chunk[0 .. slices] <- the first chunk of every
 * slice (launch), the last entry = the number of chunks (at most `cap` entries are written); *part_bytes <- bytes of a chunk per pass when
 * the call is striped (encode) / streamed (decode), else 0.  Returns the number of slices, or a negative error code. */
int trc_host_plan(int codec, size_t n, uint32_t chunk, int decode, int page_locked, size_t *first_chunk, int cap, uint32_t *part_bytes);
/* the chunk for a DEVICE-RESIDENT call of n bytes (one launch over the whole input): the largest multiple of 64 <= 4096 that
 * makes the input a whole number of residency rounds of the coder's lanes, barely (a launch lasts rounds x one wave's time:
 * 100 MB of the model-per-lane coders at 1280 instead of 1536 is half the throughput).  What bench.py runs every coder at. */
uint32_t trc_round_chunk(int codec, size_t n);

/* ---- device-resident layer --------------------------------------------------------------------
 * All d_* pointers are device pointers on the current HIP device with TRC_PAD readable/writable
 * bytes of slack behind the stated size.  Alignment, as trc_encode_dev / trc_decode_dev check it:
 * d_in and d_out 16 bytes, d_work 256, d_total 8, d_clen 4, and d_payload 2 bytes only -- a
 * payload may sit at any even offset of a container, on the encode and on the decode side
 * (tests/test_gpu_sweep.py::test_payload_alignment).  `stream` is a hipStream_t (NULL = default
 * stream).  Calls only enqueue work; they never synchronise.                                    */

/* bytes of device workspace trc_encode_dev / trc_decode_dev need for (codec, n, chunk); 0 for an id that names no coder
 * (42, 51, 56, 57, 61, above 65, negative) or a chunk trc_encode_dev rejects.  codec 0: the 4096 bytes of trc_cdfini_dev. */
size_t trc_work_bytes(int codec, size_t n, uint32_t chunk);

/* cdfini on device (reference: rccdf.c:50-68): byte histogram of d_in[0..n) -> 15-bit CDF
 * d_cdf[0..cdfnum] (uint16).  d_status (int32, device) receives (int)n or -1 where the reference
 * would die().  d_work: >= trc_work_bytes(0, 0, 0) bytes.                                        */
int trc_cdfini_dev(const void *d_in, size_t n, uint16_t *d_cdf, unsigned cdfnum,
                   int32_t *d_status, void *d_work, void *stream);

/* The two halves of trc_cdfini_dev, for sharded inputs: every rank histograms its shard
 * (d_hist: uint64[256], zeroed by the call), the histograms are summed across ranks (one RCCL
 * all-reduce of 2 KiB), then every rank builds the same CDF from the global histogram. */
int trc_hist_dev(const void *d_in, size_t n, uint64_t *d_hist, void *stream);
int trc_cdf_from_hist_dev(const uint64_t *d_hist, size_t n_total, uint16_t *d_cdf, unsigned cdfnum,
                          int32_t *d_status, void *stream);

/* Static coders derive their symbol tables (44 KiB at the start of the workspace) from the CDF at every
 * trc_encode_dev / trc_decode_dev call.  A caller that codes many buffers against one CDF -- the reference harness
 * builds its CDF once, untimed, before the timed calls (turborc.c:429-433) -- can build them once with
 * trc_tables_dev and pass `codec | TRC_TABLES_READY` afterwards; the tables stay valid until the CDF or the
 * workspace changes. */
#define TRC_TABLES_READY 0x100
int trc_tables_dev(const uint16_t *d_cdf, unsigned cdfnum, void *d_work, size_t work_bytes, void *stream);

/* Encode n bytes at d_in with `codec`.
 *   d_cdf/cdfnum : static coders only (uint16[cdfnum+1], cdf[cdfnum] == 32768), else NULL/0; the "ss" coders (TRC_RCSS ..
 *                  TRC_RCU3SS) take NULL and cdfnum = TRC_SS_PRM(prm0, prm1), here and in every decode call below
 *   d_clen       : uint32[nchunks]  <- per-chunk compressed length (== chunk length: raw)
 *   d_payload    : >= n bytes       <- concatenated payloads
 *   d_total      : uint64           <- sum of clen[]
 *   d_work       : trc_work_bytes() bytes of scratch                                             */
int trc_encode_dev(int codec, const void *d_in, size_t n, uint32_t chunk,
                   const uint16_t *d_cdf, unsigned cdfnum,
                   uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                   void *d_work, size_t work_bytes, void *stream);

/* Decode: inverse of trc_encode_dev; d_out receives n bytes.
 * The decoders find a chunk's payload through per-group sums of d_clen, which a small kernel derives at every call.
 * trc_encode_dev leaves the very same sums in the workspace as a by-product, and so does every trc_decode_dev: a
 * caller that decodes the directory the workspace last saw -- encode followed by decode on one workspace, or the
 * same container decoded repeatedly, as the reference harness does -- may pass `codec | TRC_DIR_READY` to skip that
 * kernel (same (codec, n, chunk), d_clen contents unchanged since; not checked). */
#define TRC_DIR_READY 0x200
int trc_decode_dev(int codec, const uint32_t *d_clen, const void *d_payload, size_t n, uint32_t chunk,
                   const uint16_t *d_cdf, unsigned cdfnum,
                   void *d_out, void *d_work, size_t work_bytes, void *stream);

/* Random access: decode chunks [first_chunk, first_chunk + count) only.  d_clen, d_payload, n and chunk describe the WHOLE
 * container, exactly as for trc_decode_dev; d_out receives min(n, (first_chunk + count) * chunk) - first_chunk * chunk bytes,
 * the range's first byte at d_out[0], and nothing is written behind them.  first_chunk may be any chunk (no multiple of 64
 * needed).  Same alignment rules and error codes as trc_decode_dev; count == 0 returns TRC_OK and launches nothing,
 * first_chunk + count > nchunks is TRC_E_ARG.  Every coder id decodes ranges.
 * The workspace is one of its own kind, of trc_range_work_bytes(codec, n, chunk, count) bytes: what a decode of `count` chunks
 * needs plus 12 bytes per 64 chunks of the whole directory -- it grows with the range, not with n, and holds no encoder
 * scratch (always <= trc_work_bytes(codec, count * chunk, chunk) + 16 * ceil(nchunks / 64) + 4096).  0 for an id that names
 * no coder, a chunk trc_encode_dev rejects, count == 0 and count > nchunks; it never shrinks as count grows, so a workspace
 * sized for the largest range serves every smaller one.  Static coders keep their tables at its start: trc_tables_dev and
 * TRC_TABLES_READY work as above.
 * A call indexes the whole directory first (the per-group sums and their scan, O(nchunks)), then builds the range's own group
 * offsets from that index (O(count)).  `codec | TRC_DIR_READY` skips the first step.  The promise: the previous
 * trc_decode_range_dev on this workspace was for the same (n, chunk) and d_clen has not changed since -- ANY first_chunk and
 * ANY count, the index lies where (n, chunk) alone put it.  So the first range of a container costs O(nchunks), every later
 * one O(count).  The flag does not carry over between the two kinds of workspace: a trc_decode_dev / trc_encode_dev workspace
 * never serves trc_decode_range_dev and the other way round. */
size_t trc_range_work_bytes(int codec, size_t n, uint32_t chunk, size_t count);
int    trc_decode_range_dev(int codec, const uint32_t *d_clen, const void *d_payload, size_t n, uint32_t chunk,
                            size_t first_chunk, size_t count,
                            const uint16_t *d_cdf, unsigned cdfnum,
                            void *d_out, void *d_work, size_t work_bytes, void *stream);

/* ---- multi-GPU: the gather of results over RCCL (xGMI), plain C ------------------------------------------------
 * One process per GPU; every rank codes a contiguous range of whole chunks with the calls above (no data-path
 * collective).  Static coders first agree on one CDF: trc_hist_dev on the shard, trc_hist_allreduce_dev (256 x u64
 * summed in place), trc_cdf_from_hist_dev with the total length -- the gathered container then equals the single-GPU
 * container of the whole input bit for bit.
 * trc_exchange_dev gathers `nbatch` consecutive results at once, batch j onto rank j % world (nbatch = 1: the plain
 * gather onto rank 0; nbatch = world: every directed xGMI link carries one payload, all at the same time).  One
 * all-gather of the sizes, a host sync to read them, then ONE grouped ncclSend/ncclRecv call.
 *   nccl_comm   an ncclComm_t (passed as void*: RCCL is resolved at run time, this header needs no RCCL header)
 *   b[j]        batch j: this rank's result (d_clen[nchunks], d_payload, d_total as trc_encode_dev left them) and, on the
 *               batch's root, the receive buffers: d_clen_all (all ranks' directory slices in rank order) and
 *               d_payload_all (all ranks' payloads in rank order = the container's payload area)
 *   h_sizes     host, uint64[world * nbatch * 2] <- {payload bytes, chunks} of rank r, batch j at [(r*nbatch + j)*2]
 *   d_meta      device scratch, 16 * nbatch * (world + 1) bytes                                                    */
#define TRC_EXCHANGE_MAX_BATCH 64
typedef struct trc_batch {
    const uint32_t *d_clen; size_t nchunks; const void *d_payload; const uint64_t *d_total;
    uint32_t *d_clen_all; void *d_payload_all;
} trc_batch;
int trc_exchange_dev(void *nccl_comm, int nbatch, const trc_batch *b, uint64_t *h_sizes, void *d_meta, void *stream);
int trc_hist_allreduce_dev(void *nccl_comm, uint64_t *d_hist, void *stream);

/* Host-pointer encode that ALWAYS returns the TRC1 container, with an explicit chunk size -- for callers that repackage the
 * per-chunk payloads themselves (harness/trcfile.c writes the reference's file format from it) and therefore must not get
 * the reference convention "return == n means out is a raw copy" applied to the container as a whole.  out must hold
 * trc_container_bound(n, chunk) bytes (header + directory + n: every chunk stored raw).  Returns the container size, 0 on
 * error.  Decode with the reference-named decoder of the codec, or trc_decode_dev. */
size_t trc_container_bound(size_t n, uint32_t chunk);
size_t trc_encode_host(int codec, const void *in, size_t n, uint32_t chunk, void *out, size_t outcap,
                       const uint16_t *cdf, unsigned cdfnum);       /* "ss" coders: cdf = NULL, cdfnum = TRC_SS_PRM(prm0, prm1) */

/* Bounded decode for untrusted input: the reference-named decoders carry no input length, this one does -- the container is
 * validated against `inlen` (trc_container_check) before anything is read; inlen == outlen means "stored raw" and is copied.
 * cdf / cdfnum: static coders only (cdfnum 0: derived from the CDF's terminating 32768).  The "ss" coders take cdf = NULL and
 * cdfnum = 0 (the parameters are read from the header) or TRC_SS_PRM(..), which must then equal the header's: otherwise 0 is
 * returned.  Returns outlen, 0 on error. */
size_t trc_decode_host(int codec, const void *in, size_t inlen, void *out, size_t outlen,
                       const uint16_t *cdf, unsigned cdfnum);

/* Host-pointer calls and page-locked memory.  A pageable caller buffer travels through pinned staging slots (copy threads
 * + DMA: 38-40 GB/s per direction on the MI355X box); a page-locked one -- hipHostMalloc, or registered with the pair
 * below -- is read / written by DMA directly, detected per call with hipPointerGetAttributes.  Registration costs ~55 us
 * per MB, so it pays for buffers that are reused, as the reference harness reuses (in, out) for every timed repetition. */
int trc_host_pin(void *p, size_t len);
int trc_host_unpin(void *p);

/* Validate a TRC1 container held in buf[0..buflen) BEFORE handing it to a reference-named decoder: those prototypes
 * carry no input length, so a caller reading untrusted files must check that everything the decoder will touch lies
 * inside its buffer.  Checks header fields, codec (0 = any), the original length (outlen, (size_t)-1 = any), that the
 * directory fits, and that the directory's lengths add up to exactly the stated payload, which must end inside
 * buflen; a container of an "ss" coder must hold two parameters in 1 .. 15 in its cdfnum field.  Host-only (no GPU needed).
 * Returns TRC_OK or TRC_E_ARG (text in trc_last_error()). */
int trc_container_check(const void *buf, size_t buflen, int codec, size_t outlen);

/* Random access through host pointers.  trc_container_range (host only, no GPU needed) validates the container as
 * trc_container_check(buf, buflen, codec, (size_t)-1) does and plans bytes [offset, offset + len) of the original:
 *   first_chunk, nchunks     the chunks that cover them
 *   payload_off, payload_len where those chunks' payload lies, from the start of the payload area
 *                            (buf + 32 + 4 * hdr.nchunks), in bytes
 *   out_skip                 offset - first_chunk * chunk: the range's first byte within the covering chunks' output
 *   out_bytes                decoded size of the covering chunks
 * len == 0 or offset + len > n is TRC_E_ARG.  A caller with its own transport reads clen[first_chunk .. + nchunks) and
 * those payload_len bytes, nothing else: the two are a container of (out_bytes, chunk) for trc_decode_dev.
 * trc_decode_range_host does exactly that on the calling thread's current device (device lists are not used): it sends
 * the covering chunks' directory entries and payload, decodes them, and copies `len` bytes to out.  n is the original
 * length; inlen == n means "stored raw", as for trc_decode_host, and is a memcpy of the range.  cdf / cdfnum as for
 * trc_decode_host.  Returns len, 0 on error (text in trc_last_error(); without a device it says so). */
typedef struct trc_range { uint64_t first_chunk, nchunks, payload_off, payload_len, out_skip, out_bytes; } trc_range;
int    trc_container_range(const void *buf, size_t buflen, int codec, size_t offset, size_t len, trc_range *r);
size_t trc_decode_range_host(int codec, const void *in, size_t inlen, size_t n, size_t offset, size_t len, void *out,
                             const uint16_t *cdf, unsigned cdfnum);

/* ---- byte planes of 16 / 32 / 64-bit elements ---------------------------------------------------------------------
 * A byte coder run flat over bf16 / fp16 / fp32 / fp64 or wide-integer data mixes near-uniform mantissa bytes with highly
 * skewed sign / exponent bytes.  These calls code the BYTE PLANES separately, on the device, without touching the coders:
 *        esize in {2, 4, 8};   m = n / esize whole elements;   t = n % esize tail bytes;   plane k = the m bytes in[i * esize + k]
 * (the plain definition: the reference's tpenc, transpose_.c:110-123, gives exactly this where n % (32 esize) < esize and an
 * ISA-dependent layout elsewhere -- DESIGN.md).  Any other esize and m == 0 are TRC_E_ARG.
 *
 * The two kernels.  Planes lie `pitch` bytes apart: a multiple of 256, at least m; trc_planes_pitch(n, esize) = m + TRC_PAD
 * rounded up to 256 is the pitch of the coded calls below (0 for a bad esize or m == 0).  d_in / d_out 16-byte, d_planes 256-byte
 * aligned; d_tail: 8 bytes on the device that receive / supply the t tail bytes, may be NULL when t == 0.  Nothing is written
 * outside [0, m) of each plane, [0, t) of the tail and [0, n) of d_out; the calls only enqueue work. */
size_t trc_planes_pitch(size_t n, unsigned esize);
int trc_planes_split_dev(const void *d_in, size_t n, unsigned esize, void *d_planes, size_t pitch, void *d_tail, void *stream);
int trc_planes_join_dev(const void *d_planes, size_t pitch, const void *d_tail, size_t n, unsigned esize, void *d_out, void *stream);

/* Coded planes, device-resident: split into the workspace, then one trc_encode_dev(codec, plane k, m, chunk, ...) per plane on
 * the caller's stream -- plane k's (clen, payload, total) is exactly what trc_encode_dev returns for the m bytes of plane k.
 * With nc = ceil(m / chunk) and pitch = trc_planes_pitch(n, esize):
 *   d_clen    : uint32[esize * nc]      plane k's directory at d_clen + k * nc
 *   d_payload : esize * pitch bytes     plane k's payload at (char *)d_payload + k * pitch
 *   d_total   : uint64[esize]           plane k's payload bytes
 *   d_tail    : 8 bytes                 the t tail bytes (may be NULL when t == 0)
 * Static coders: every plane gets its OWN CDF, built over the plane as trc_cdfini_dev builds it, at d_cdf + k *
 * TRC_PLANES_CDF_STRIDE (uint16[esize * 264]; cdfnum = the alphabet size), its status at d_status[k] -- on encode d_cdf is an
 * OUTPUT, on decode an input.  Every other coder takes d_cdf = d_status = NULL; the "ss" coders pass cdfnum = TRC_SS_PRM(..)
 * through to every plane.  Decode and range decode run trc_decode_dev / trc_decode_range_dev per plane and join.  The range
 * call returns ELEMENTS [first_chunk * chunk, min(m, (first_chunk + count) * chunk)), esize times as many bytes, the first
 * element at d_out[0], never tail bytes.  Argument errors are those of the per-plane calls; TRC_TABLES_READY and TRC_DIR_READY
 * are TRC_E_ARG in all three (the planes share nothing a caller could promise about).
 * Workspace: trc_planes_work_bytes (encode and decode) / trc_planes_range_work_bytes bytes, 256-byte aligned: every plane has a
 * slice of its own, the plane buffer followed by what the per-plane call needs.  Both return 0 for what the calls reject.
 * The seven coders that keep only the low four bits of a byte (TRC_RCA4, TRC_RCAI4, TRC_ANSA4, TRC_RC4, TRC_RC4C, TRC_RC4SS,
 * TRC_RC4CSS) are refused by every coded planes call, filtered, host-pointer and container checks included: TRC_E_ARG / 0. */
#define TRC_PLANES_CDF_STRIDE 264
size_t trc_planes_work_bytes(int codec, size_t n, unsigned esize, uint32_t chunk);
int trc_encode_planes_dev(int codec, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                          uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                          uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                          void *d_work, size_t work_bytes, void *stream);
int trc_decode_planes_dev(int codec, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                          size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                          void *d_out, void *d_work, size_t work_bytes, void *stream);
size_t trc_planes_range_work_bytes(int codec, size_t n, unsigned esize, uint32_t chunk, size_t count);
int trc_decode_planes_range_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                const uint16_t *d_cdf, unsigned cdfnum,
                                void *d_out, void *d_work, size_t work_bytes, void *stream);

/* Coded planes through host pointers: the TRCP container, little endian.
 *   trc_planes_hdr (32 B) | uint64 off[esize] | section 0 .. esize - 1 | tail bytes
 *   off[k]     offset of section k from the container's start, a multiple of 8
 *   section k  static coders only: uint16 cdf[cdfnum + 1], zero-padded to a multiple of 8; then the TRC1 container of plane k,
 *              byte-identical to trc_encode_host(codec, plane k, m, chunk, ..) with the plane's own CDF -- so the
 *              reference-named decoders, trc_container_check and trc_container_range work on a section as they stand
 *   tail       `tail` bytes, the last bytes of the container
 * trc_encode_planes_host: chunk 0 = trc_auto_chunk_codec(codec, m); cdfnum = the alphabet size (static coders), TRC_SS_PRM (ss
 * coders), else 0; out must hold the container (trc_planes_bound is always enough; its chunk 0 = any chunk).  Decoders read
 * everything from the header.  trc_decode_planes_range_host returns bytes [offset, offset + len) of the original: it sends only
 * the covering chunks of every plane and takes tail bytes straight from the container.  All return the size, 0 on error (text
 * in trc_last_error()).  These calls are plain: the caller's current device, one copy each way, no device list, no striping.
 * trc_planes_check (host only, no GPU needed; outlen (size_t)-1 = any) validates magic, version, esize, tail == n % esize,
 * size <= buflen, the offsets (increasing, multiples of 8, inside size), every section with trc_container_check(section, its
 * extent, codec, m), a static coder's CDFs (strictly increasing, ending at 32768) and an ss coder's parameters; both decoders
 * call it before they read anything else. */
#define TRC_PLANES_MAGIC 0x50435254u   /* "TRCP" */
typedef struct trc_planes_hdr {
    uint32_t magic;      /* TRC_PLANES_MAGIC */
    uint8_t  codec;      /* enum trc_codec */
    uint8_t  version;    /* 1 */
    uint8_t  esize;      /* 2, 4 or 8 */
    uint8_t  tail;       /* n % esize */
    uint32_t chunk;      /* chunk size of every plane, in bytes */
    uint32_t cdfnum;     /* static coders: alphabet size; ss coders: TRC_SS_PRM; else 0 */
    uint64_t n;          /* original length */
    uint64_t size;       /* the whole container, bytes */
} trc_planes_hdr;        /* 32 bytes, little endian */
size_t trc_planes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum);
size_t trc_encode_planes_host(int codec, const void *in, size_t n, unsigned esize, uint32_t chunk,
                              void *out, size_t outcap, unsigned cdfnum);
size_t trc_decode_planes_host(const void *in, size_t inlen, void *out, size_t outlen);
size_t trc_decode_planes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out);
int    trc_planes_check(const void *buf, size_t buflen, size_t outlen);

/* ---- byte planes behind a predictor filter -----------------------------------------------------------------------------
 * The low byte planes of sorted ids, timestamps, offsets or sampled signals are near-uniform: their structure lies between
 * neighbouring elements.  A filter replaces every element by its difference to the one before it, ahead of the split:
 *        x[i] = the m elements as little-endian unsigned words of w = 8 * esize bits;   p[i] = 0 where i % seg == 0, else x[i - 1]
 *        TRC_FILTER_ZDELTA   d = x[i] - p[i] mod 2^w;   y[i] = (d << 1) ^ (0 - (d >> (w - 1)))      (zigzag of d read as signed)
 *                            inverse: d = (y >> 1) ^ (0 - (y & 1));   x[i] = p[i] + d mod 2^w
 *        TRC_FILTER_XOR      y[i] = x[i] ^ p[i];   inverse: x[i] = y[i] ^ p[i]
 * F(filter, seg, esize, in) = the y's followed by the t untouched tail bytes.  The predictor RESTARTS every seg elements (a multiple
 * of 64 in [TRC_CHUNK_MIN, TRC_CHUNK_MAX], the chunk rule; anything else is TRC_E_ARG), and the coded calls use seg = chunk, so a
 * restart segment is a coded chunk of every plane: the inverse is a scan within one segment, and a chunk range still decodes
 * from its own bytes alone.  A filter is an option, never a default: it helps integer columns and smooth series and does nothing
 * for weights.
 *
 * The whole contract:  fplanes(filter, ..., in)  ==  planes(..., F(filter, chunk, esize, in))  byte for byte -- directory, payload,
 * totals, per-plane CDFs, tail, the host container's body.  Every argument, alignment, flag and workspace rule is the one of the
 * unfiltered call (trc_planes_work_bytes / trc_planes_range_work_bytes serve unchanged: the filter lives inside split and join).
 * filter = TRC_FILTER_NONE makes a device call its unfiltered counterpart, launching the same kernels; any other value outside
 * {1, 2} is TRC_E_ARG before anything else is looked at.  The range call returns elements [first_chunk * chunk,
 * min(m, (first_chunk + count) * chunk)): its scan starts at a restart. */
enum { TRC_FILTER_NONE = 0, TRC_FILTER_ZDELTA = 1, TRC_FILTER_XOR = 2 };
int trc_planes_split_filter_dev(int filter, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                void *d_planes, size_t pitch, void *d_tail, void *stream);
int trc_planes_join_filter_dev(int filter, const void *d_planes, size_t pitch, const void *d_tail,
                               size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream);
int trc_encode_fplanes_dev(int codec, int filter, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                           uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                           uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                           void *d_work, size_t work_bytes, void *stream);
int trc_decode_fplanes_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                           size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                           void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_decode_fplanes_range_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload,
                                 size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                 const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_out, void *d_work, size_t work_bytes, void *stream);

/* Filtered planes through host pointers: the TRCF container = a 16-byte prefix in front of an ordinary TRCP container of
 * F(filter, chunk, esize, in).  Bytes [16, size) are byte-identical to trc_encode_planes_host(codec, F(in), ...) at the same
 * resolved chunk, so trc_planes_check, trc_container_check and trc_container_range work on the inner part as they stand.
 * trc_encode_fplanes_host takes filter 1 or 2 (TRC_FILTER_NONE returns 0: trc_encode_planes_host writes that content, one
 * container per content); out must hold trc_fplanes_bound = trc_planes_bound + 16 bytes.  The decoders read everything from the
 * two headers; the range decoder fetches the covering chunks of every plane, which are whole segments.  All return the size,
 * 0 on error (text in trc_last_error()).  trc_fplanes_check (host only, no GPU needed) validates magic, version 1, filter 1 or 2,
 * zero == 0, 16 < size <= buflen, then trc_planes_check(buf + 16, size - 16, outlen); both decoders call it first. */
#define TRC_FPLANES_MAGIC 0x46435254u   /* "TRCF" */
typedef struct trc_fplanes_hdr {
    uint32_t magic;      /* TRC_FPLANES_MAGIC */
    uint8_t  filter;     /* TRC_FILTER_ZDELTA or TRC_FILTER_XOR */
    uint8_t  version;    /* 1 */
    uint16_t zero;
    uint64_t size;       /* 16 + the inner TRCP container's size */
} trc_fplanes_hdr;       /* 16 bytes, little endian */
size_t trc_fplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum);
size_t trc_encode_fplanes_host(int codec, int filter, const void *in, size_t n, unsigned esize, uint32_t chunk,
                               void *out, size_t outcap, unsigned cdfnum);
size_t trc_decode_fplanes_host(const void *in, size_t inlen, void *out, size_t outlen);
size_t trc_decode_fplanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out);
int    trc_fplanes_check(const void *buf, size_t buflen, size_t outlen);

/* ---- the planes advisor: which filter for this buffer? -------------------------------------------------------------------
 * A filter is an option, never a default, so somebody has to choose; what decides the choice is the order-0 byte histogram of
 * every plane under every filter, and all of them come from ONE read of the input at about the cost of a split, writing nothing
 * but counters.
 *
 * trc_planes_hist_dev(filters, d_in, n, esize, seg, d_hist, stream): filters is a bit set, bit f requests filter id f (1 = none,
 * 2 = zigzag delta, 4 = xor; 1 .. 7, anything else is TRC_E_ARG).  d_hist[(f * esize + k) * 256 + b] = the number of the m =
 * n / esize elements whose byte k under filter f (restarted every seg elements) equals b.  The call zeroes all
 * trc_planes_hist_bytes(esize) = 3 * esize * 256 * 8 bytes first, on the stream: rows of filters not requested stay zero, nothing
 * behind them is written.  The tail bytes are in no plane and are not counted.  Arguments as for trc_planes_split_filter_dev
 * (esize 2, 4 or 8; n >= esize; seg by the chunk rule; d_in 16-byte aligned), d_hist 8-byte aligned.  Only enqueues work.
 * TRC_PLANES_GRID caps its grid as it does the split's; TRC_PLANES_HIST_ROUND_VECS (test aid) = vectors per thread between two
 * flushes of a workgroup's 32-bit counters.
 *
 * trc_planes_advise (host only, no GPU needed) turns such histograms into estimates and a choice:
 *     bits[f][k] = sum over b of c * log2(m / c), c = hist[(f * esize + k) * 256 + b]      (0 for rows not requested)
 *     total_bits[f] = sum over the planes
 *     filter = the requested filter with the smallest total, ties to the lower id -- but TRC_FILTER_NONE where it was requested
 *              and the winner saves less than 1/64 of TRC_FILTER_NONE's total.
 * The 1/64 is policy, not a measurement: on uniform data the three totals differ by noise only (0.01 - 0.03 % on 65 539 random
 * elements) and an argmin would pick a filter by coin toss; a filter has to earn its place.  Every requested row must sum to m:
 * a row that does not, esize outside {2, 4, 8}, filters outside 1 .. 7, m == 0 or a NULL pointer is TRC_E_ARG.
 *
 * trc_encode_aplanes_host: upload once, trc_planes_hist_dev(7, ..., seg = the resolved chunk), trc_planes_advise, then the coded
 * call on the bytes already on the device.  The output is byte for byte what the explicit call writes at the same resolved chunk:
 * trc_encode_planes_host (a TRCP container) where the choice is TRC_FILTER_NONE, trc_encode_fplanes_host(..., choice, ...) (a TRCF
 * container) otherwise; out must hold trc_fplanes_bound bytes; *advice (may be NULL) receives what decided.
 * trc_decode_xplanes_host reads either container: it looks at the magic and calls trc_decode_planes_host or
 * trc_decode_fplanes_host (or, for the TRCS container of the strided filters below, trc_decode_splanes_host); any other magic
 * returns 0 with the reason in trc_last_error(). */
typedef struct trc_planes_advice {
    int      filter;             /* the choice: TRC_FILTER_NONE, TRC_FILTER_ZDELTA or TRC_FILTER_XOR */
    unsigned esize, filters;     /* as given */
    uint64_t m;
    double   bits[3][8];         /* order-0 estimate of plane k under filter f, in bits */
    double   total_bits[3];      /* sum over the planes */
} trc_planes_advice;
size_t trc_planes_hist_bytes(unsigned esize);
int    trc_planes_hist_dev(unsigned filters, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                           uint64_t *d_hist, void *stream);
int    trc_planes_advise(const uint64_t *hist, unsigned filters, unsigned esize, size_t m, trc_planes_advice *a);
size_t trc_encode_aplanes_host(int codec, const void *in, size_t n, unsigned esize, uint32_t chunk,
                               void *out, size_t outcap, unsigned cdfnum, trc_planes_advice *advice);
size_t trc_decode_xplanes_host(const void *in, size_t inlen, void *out, size_t outlen);

/* ---- byte planes behind a STRIDED predictor filter: interleaved data -------------------------------------------------
 * Rows of K same-width fields, stereo / 5.1 / 7.1 PCM, xyz(w) points, complex pairs, RGB(A)16: the element in front belongs to
 * another series, and a filter that predicts from it is worse than none.  With a stride S in 1 .. TRC_STRIDE_MAX the predictor of
 * the filtered planes above reaches S elements back; everything not named here is as it is there:
 *        p[i] = 0 where i % seg < S, else x[i - S]
 *        y[i] = zigzag(x[i] - p[i] mod 2^w)  (TRC_FILTER_ZDELTA)      x[i] ^ p[i]  (TRC_FILTER_XOR)
 *        F_S(filter, seg, esize, in) = the y's followed by the t untouched tail bytes;   F_1 = F
 * The predictor still restarts every seg elements, whether or not S divides seg: a chunk range still decodes from its own bytes
 * alone and every per-chunk contract carries over.  The filter enum is untouched; the stride is an argument of calls of its own.
 *
 * The whole contract:  splanes(filter, S, ..., in)  ==  planes(..., F_S(filter, chunk, esize, in))  byte for byte -- directory,
 * payload, tail, totals, statuses and per-plane CDFs.  Arguments, alignment, flags and workspace (trc_planes_work_bytes /
 * trc_planes_range_work_bytes: the filter needs none) are those of the fplanes calls, with `int stride` behind `int filter`.
 * A stride outside 1 .. TRC_STRIDE_MAX is TRC_E_ARG, reported ahead of everything else, pointers included, so without a device.
 * With stride == 1 or filter == TRC_FILTER_NONE a device call IS the fplanes call and launches its kernels.
 *
 * trc_planes_hist_stride_dev has the layout and the rules of trc_planes_hist_dev, with the rows of filters 1 and 2 counted under
 * F_stride (the row of TRC_FILTER_NONE does not depend on it), so trc_planes_advise serves on its output as it stands; a caller
 * picks among strides by comparing total_bits of several calls.  The advisor does not search strides by itself.
 *
 * Host pointers: the TRCS container = trc_splanes_hdr (16 bytes: the TRCF prefix with the stride where that one has its reserved
 * field) in front of the TRCP container of F_S(filter, chunk, esize, in); bytes [16, size) are byte-identical to
 * trc_encode_planes_host(codec, F_S(in), ...) at the same resolved chunk.  trc_encode_splanes_host takes filter 1 or 2 and stride
 * 2 .. TRC_STRIDE_MAX: stride 1 returns 0 and names trc_encode_fplanes_host, TRC_FILTER_NONE names trc_encode_planes_host (one
 * layout per content); out must hold trc_splanes_bound = trc_planes_bound + 16 bytes.  The decoders read everything from the two
 * headers.  trc_splanes_check (host only, no GPU needed) validates magic, version 1, filter 1 or 2, stride 2 .. TRC_STRIDE_MAX,
 * 16 < size <= buflen, then trc_planes_check(buf + 16, size - 16, outlen); the decoders call it first.  trc_decode_xplanes_host
 * reads a TRCS container too. */
#define TRC_STRIDE_MAX 8
int trc_planes_split_sfilter_dev(int filter, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                 void *d_planes, size_t pitch, void *d_tail, void *stream);
int trc_planes_join_sfilter_dev(int filter, int stride, const void *d_planes, size_t pitch, const void *d_tail,
                                size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream);
int trc_encode_splanes_dev(int codec, int filter, int stride, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                           uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                           uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                           void *d_work, size_t work_bytes, void *stream);
int trc_decode_splanes_dev(int codec, int filter, int stride, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                           size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                           void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_decode_splanes_range_dev(int codec, int filter, int stride, const uint32_t *d_clen, const void *d_payload,
                                 size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                 const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_planes_hist_stride_dev(unsigned filters, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                               uint64_t *d_hist, void *stream);
#define TRC_SPLANES_MAGIC 0x53435254u   /* "TRCS" */
typedef struct trc_splanes_hdr {
    uint32_t magic;      /* TRC_SPLANES_MAGIC */
    uint8_t  filter;     /* TRC_FILTER_ZDELTA or TRC_FILTER_XOR */
    uint8_t  version;    /* 1 */
    uint16_t stride;     /* 2 .. TRC_STRIDE_MAX */
    uint64_t size;       /* 16 + the inner TRCP container's size */
} trc_splanes_hdr;       /* 16 bytes, little endian */
size_t trc_splanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum);
size_t trc_encode_splanes_host(int codec, int filter, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                               void *out, size_t outcap, unsigned cdfnum);
size_t trc_decode_splanes_host(const void *in, size_t inlen, void *out, size_t outlen);
size_t trc_decode_splanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out);
int    trc_splanes_check(const void *buf, size_t buflen, size_t outlen);

/* ---- byte planes behind a predictor of ORDER 2 or 3: smooth series ---------------------------------------------------
 * Sampled signals, PCM and sensor series are smooth, and the first difference of a smooth series is smooth again: the filters
 * above leave most of its structure in place.  The fixed polynomial predictors of the lossless audio coders take the difference
 * K times.  With the names above, S the stride in 1 .. TRC_STRIDE_MAX and K the order in 0 .. TRC_ORDER_MAX:
 *        D_S(a)[i] = a[i] where i % seg < S,  a[i] - a[i - S] mod 2^w elsewhere
 *        y[i]      = zigzag(D_S applied K times to x, at i)                               (zigzag once, at the end)
 *        O(K, S, seg, esize, in) = the y's followed by the t untouched tail bytes
 * or, with x taken as zero in front of its segment, D^K[i] = sum_j (-1)^j C(K, j) x[i - j S]:  x[i] - 2 x[i - S] + x[i - 2S]  for
 * K = 2,  x[i] - 3 x[i - S] + 3 x[i - 2S] - x[i - 3S]  for K = 3.  The inverse undoes the zigzag and runs K class-wise segmented
 * prefix sums mod 2^w from a zero state (a class = the place in the segment mod S).  K = 1 is F_S(TRC_FILTER_ZDELTA, ...), K = 0 is
 * no filter; there is no xor form.  The filter enum is untouched: the order is an argument of calls of its own, as the stride is.
 * An order is an option, never a default: on integer columns that the first difference already flattens, order 2 stores MORE.
 *
 * The whole contract:  oplanes(K, S, ..., in)  ==  planes(..., O(K, S, chunk, esize, in))  byte for byte -- directory, payload,
 * tail, totals, statuses and per-plane CDFs; a chunk range decodes from its own bytes alone.  Arguments, alignment, flags and
 * workspace are those of the planes calls (the filter needs no workspace), with `int order, int stride` where the splanes calls
 * have `int filter, int stride`.  An order outside 0 .. TRC_ORDER_MAX is TRC_E_ARG ahead of everything else, pointers included, so
 * without a device; the stride is looked at next; everything else as in the planes calls.  With order 0 a device call IS the
 * unfiltered call, with order 1 it IS the splanes call with TRC_FILTER_ZDELTA, and launches those kernels.
 *
 * trc_planes_hist_order_dev counts the planes under orders 0 .. 3 at one stride in one read of the input: orders is a bit set, bit
 * k = order k (1 .. 15, anything else is TRC_E_ARG, then the stride), d_hist[(k * esize + p) * 256 + b] as trc_planes_hist_dev has
 * it; the call zeroes all trc_planes_hist_order_bytes(esize) = 4 * esize * 256 * 8 bytes first, rows not requested stay zero,
 * nothing behind them is written.  Rows 0 and 1 are rows 0 and 1 of trc_planes_hist_stride_dev(3, stride, ...).
 * trc_planes_advise_order (host only) gives the estimates of trc_planes_advise and the requested order with the smallest total,
 * ties to the lower order -- but order 0 where it was requested and the winner saves less than 1/64 of its total (the same
 * policy).  Every requested row must sum to m; that, orders outside 1 .. 15, a bad esize, m == 0 or a NULL pointer is TRC_E_ARG.
 *
 * Host pointers: the TRCO container = trc_oplanes_hdr (16 bytes) in front of the TRCP container of O(K, S, chunk, esize, in);
 * bytes [16, size) are byte-identical to trc_encode_planes_host(codec, O(in), ...) at the same resolved chunk.
 * trc_encode_oplanes_host takes order 2 or 3: order 0 returns 0 and names trc_encode_planes_host, order 1 names
 * trc_encode_fplanes_host / trc_encode_splanes_host (one layout per content); out must hold trc_oplanes_bound = trc_planes_bound
 * + 16 bytes.  trc_oplanes_check (host only) validates magic, version 1, order 2 .. 3, stride 1 .. TRC_STRIDE_MAX, 16 < size <=
 * buflen, then trc_planes_check(buf + 16, size - 16, outlen); the decoders call it first.  trc_decode_xplanes_host reads a TRCO
 * container too.  trc_encode_aoplanes_host: upload once, trc_planes_hist_order_dev(15, stride, ..., seg = the resolved chunk),
 * trc_planes_advise_order, then the coded call on the bytes already on the device; the output is byte for byte what the explicit
 * call writes for that choice -- TRCP for order 0, TRCF for order 1 at stride 1, TRCS for order 1 at a stride above 1, TRCO for
 * order 2 or 3; out must hold trc_oplanes_bound bytes; *advice (may be NULL) receives what decided. */
#define TRC_ORDER_MAX 3
int trc_planes_split_ofilter_dev(int order, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                 void *d_planes, size_t pitch, void *d_tail, void *stream);
int trc_planes_join_ofilter_dev(int order, int stride, const void *d_planes, size_t pitch, const void *d_tail,
                                size_t n, unsigned esize, uint32_t seg, void *d_out, void *stream);
int trc_encode_oplanes_dev(int codec, int order, int stride, const void *d_in, size_t n, unsigned esize, uint32_t chunk,
                           uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                           uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                           void *d_work, size_t work_bytes, void *stream);
int trc_decode_oplanes_dev(int codec, int order, int stride, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                           size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                           void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_decode_oplanes_range_dev(int codec, int order, int stride, const uint32_t *d_clen, const void *d_payload,
                                 size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                 const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_out, void *d_work, size_t work_bytes, void *stream);
typedef struct trc_planes_order_advice {
    int      order;              /* the choice: 0 .. TRC_ORDER_MAX */
    unsigned esize, orders;      /* as given */
    uint64_t m;
    double   bits[4][8];         /* order-0 model estimate of plane p under predictor order k, in bits */
    double   total_bits[4];      /* sum over the planes */
} trc_planes_order_advice;
size_t trc_planes_hist_order_bytes(unsigned esize);
int    trc_planes_hist_order_dev(unsigned orders, int stride, const void *d_in, size_t n, unsigned esize, uint32_t seg,
                                 uint64_t *d_hist, void *stream);
int    trc_planes_advise_order(const uint64_t *hist, unsigned orders, unsigned esize, size_t m, trc_planes_order_advice *a);
#define TRC_OPLANES_MAGIC 0x4f435254u   /* "TRCO" */
typedef struct trc_oplanes_hdr {
    uint32_t magic;      /* TRC_OPLANES_MAGIC */
    uint8_t  order;      /* 2 .. TRC_ORDER_MAX */
    uint8_t  version;    /* 1 */
    uint16_t stride;     /* 1 .. TRC_STRIDE_MAX */
    uint64_t size;       /* 16 + the inner TRCP container's size */
} trc_oplanes_hdr;       /* 16 bytes, little endian */
size_t trc_oplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum);
size_t trc_encode_oplanes_host(int codec, int order, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                               void *out, size_t outcap, unsigned cdfnum);
size_t trc_decode_oplanes_host(const void *in, size_t inlen, void *out, size_t outlen);
size_t trc_decode_oplanes_range_host(const void *in, size_t inlen, size_t offset, size_t len, void *out);
int    trc_oplanes_check(const void *buf, size_t buflen, size_t outlen);
size_t trc_encode_aoplanes_host(int codec, int stride, const void *in, size_t n, unsigned esize, uint32_t chunk,
                                void *out, size_t outcap, unsigned cdfnum, trc_planes_order_advice *advice);

/* ---- byte planes relative to a BASE buffer: checkpoint and page deltas ------------------------------------------------
 * The filters above predict from inside the buffer.  A checkpoint, a fine-tuned model or an updated KV-cache page has a better
 * predictor: the same buffer one version earlier, already on the device.  With a base of the same element layout:
 *        x[i], b[i] = the m = n / esize elements of `in` and of `base`, little-endian unsigned words of w = 8 * esize bits
 *        TRC_FILTER_ZDELTA   d = x[i] - b[i] mod 2^w;   y[i] = zigzag(d)        inverse: x[i] = b[i] + unzigzag(y[i]) mod 2^w
 *        TRC_FILTER_XOR      y[i] = x[i] ^ b[i]                                  inverse: x[i] = y[i] ^ b[i]
 *        D(filter, esize, in, base) = the y's followed by the t = n % esize tail bytes of `in`, untouched
 * The filter enum is untouched; the base is an argument of calls of their own.  There is no restart and no `seg`: element i
 * depends on element i of the base only, so the inverse is elementwise.  The calls read bytes [0, m * esize) of the base and
 * nothing else: the base needs no TRC_PAD slack and no tail.
 *
 * The whole contract:  bplanes(filter, ..., in, base)  ==  planes(..., D(filter, esize, in, base))  byte for byte -- directory,
 * payload, totals, per-plane CDFs and statuses, tail, the host container's body.  Arguments, alignment, flags and workspace are
 * those of the unfiltered call (trc_planes_work_bytes / trc_planes_range_work_bytes serve unchanged).  A filter outside {0, 1, 2}
 * is TRC_E_ARG ahead of everything else.  With TRC_FILTER_NONE a device call IS its unfiltered counterpart, launches its kernels
 * and does not look at d_base (which may be NULL); with filter 1 or 2, d_base NULL or not 16-byte aligned is TRC_E_ARG.  The seven
 * low-nibble coders, TRC_TABLES_READY and TRC_DIR_READY are refused as everywhere in the family.
 *
 * Decoding IN PLACE is part of the contract: the d_out of the join and of the decoders may be exactly the address the call reads
 * the base from, which applies a delta to a resident base.  Any other overlap of [base, base + m * esize) with [d_out, d_out + n)
 * is TRC_E_ARG, before anything is enqueued.  trc_decode_bplanes_range_dev takes the WHOLE base and reads its elements
 * [first_chunk * chunk, ...) (that offset is a multiple of 128 bytes, so the alignment holds); d_out[0] is the range's first
 * element, and in place means d_out == (char *)d_base + first_chunk * chunk * esize.
 *
 * trc_planes_hist_base_dev has the layout and the rules of trc_planes_hist_dev (no seg), with the rows of filters 1 and 2 counted
 * under D and row 0 the unfiltered one, so trc_planes_advise serves on its output as it stands.  Without bit 1 or 2 in `filters`
 * it is trc_planes_hist_dev's unfiltered row and ignores d_base.
 *
 * The fingerprint lets a container name its base.  With W = ceil(nbytes / 8) little-endian u64 words w_j of the nbytes bytes,
 * zero-padded to 8:      fp = sum_j (2j + 1) * w_j + nbytes * 0x9E3779B97F4A7C15   mod 2^64
 * A change confined to one 8-byte word is always detected (the multiplier is odd), and so is another length of zeros.  It is an
 * IDENTITY check against mixing up files, not a cryptographic one: bases that collide are easy to construct.
 * trc_base_fingerprint_dev (d_base 16-byte aligned, read in [0, nbytes) only; d_fp 8-byte aligned, overwritten; only enqueues
 * work) and trc_base_fingerprint_host (host only, no GPU needed) give the same value. */
int trc_planes_split_base_dev(int filter, const void *d_in, const void *d_base, size_t n, unsigned esize,
                              void *d_planes, size_t pitch, void *d_tail, void *stream);
int trc_planes_join_base_dev(int filter, const void *d_planes, size_t pitch, const void *d_tail, const void *d_base,
                             size_t n, unsigned esize, void *d_out, void *stream);
int trc_encode_bplanes_dev(int codec, int filter, const void *d_in, const void *d_base, size_t n, unsigned esize, uint32_t chunk,
                           uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                           uint32_t *d_clen, void *d_payload, uint64_t *d_total, void *d_tail,
                           void *d_work, size_t work_bytes, void *stream);
int trc_decode_bplanes_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_tail,
                           const void *d_base, size_t n, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                           void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_decode_bplanes_range_dev(int codec, int filter, const uint32_t *d_clen, const void *d_payload, const void *d_base,
                                 size_t n, unsigned esize, uint32_t chunk, size_t first_chunk, size_t count,
                                 const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_out, void *d_work, size_t work_bytes, void *stream);
int trc_planes_hist_base_dev(unsigned filters, const void *d_in, const void *d_base, size_t n, unsigned esize,
                             uint64_t *d_hist, void *stream);
int      trc_base_fingerprint_dev(const void *d_base, size_t nbytes, uint64_t *d_fp, void *stream);
uint64_t trc_base_fingerprint_host(const void *base, size_t nbytes);

/* Planes against a base through host pointers: the TRCD container = a 32-byte prefix in front of an ordinary TRCP container of
 * D(filter, esize, in, base).  Bytes [32, size) are byte-identical to trc_encode_planes_host(codec, D(in, base), ...) at the same
 * resolved chunk, so trc_planes_check, trc_container_check and trc_container_range work on the inner part as they stand.
 * trc_encode_bplanes_host takes filter 1 or 2 (TRC_FILTER_NONE returns 0: trc_encode_planes_host writes that content, one layout
 * per content) and reads m * esize bytes of `base`; out must hold trc_bplanes_bound = trc_planes_bound + 32 bytes.  The base is
 * uploaded next to the input and fingerprinted on the device.  trc_decode_bplanes_host requires base_len >= base_bytes, uploads
 * and fingerprints base_bytes bytes of the base, and where the fingerprint differs from the header's returns 0 BEFORE decoding,
 * with "base fingerprint" and both values in trc_last_error().  trc_decode_bplanes_range_host uploads only the covering elements
 * of the base and the covering chunks, takes tail bytes from the container and does NOT verify the fingerprint: it never sees the
 * whole base; a caller who needs the check calls trc_base_fingerprint_host once.  All return the size, 0 on error.
 * trc_bplanes_check (host only, no GPU needed) validates, in this order, magic and version 1, filter 1 or 2, zero == 0,
 * 32 < size <= buflen, the inner container with trc_planes_check(buf + 32, size - 32, outlen), base_bytes == n - tail; both
 * decoders call it first.  trc_decode_xplanes_host returns 0 for this magic and names trc_decode_bplanes_host: it has no base. */
#define TRC_BPLANES_MAGIC 0x44435254u   /* "TRCD" */
typedef struct trc_bplanes_hdr {
    uint32_t magic;      /* TRC_BPLANES_MAGIC */
    uint8_t  filter;     /* TRC_FILTER_ZDELTA or TRC_FILTER_XOR */
    uint8_t  version;    /* 1 */
    uint16_t zero;
    uint64_t size;       /* 32 + the inner TRCP container's size */
    uint64_t base_bytes; /* m * esize: the bytes of the base the filter read */
    uint64_t base_fp;    /* the fingerprint of those bytes */
} trc_bplanes_hdr;       /* 32 bytes, little endian */
size_t trc_bplanes_bound(size_t n, unsigned esize, uint32_t chunk, unsigned cdfnum);
size_t trc_encode_bplanes_host(int codec, int filter, const void *in, const void *base, size_t n, unsigned esize, uint32_t chunk,
                               void *out, size_t outcap, unsigned cdfnum);
size_t trc_decode_bplanes_host(const void *in, size_t inlen, const void *base, size_t base_len, void *out, size_t outlen);
size_t trc_decode_bplanes_range_host(const void *in, size_t inlen, const void *base, size_t base_len,
                                     size_t offset, size_t len, void *out);
int    trc_bplanes_check(const void *buf, size_t buflen, size_t outlen);

/* ---- batched byte planes: many separate allocations in one coded call, any one of them decodable ------------------------
 * A checkpoint is hundreds of tensors of one dtype, a KV-cache a pool of pages, a table a set of columns: many allocations, each
 * too small to fill the device and too many to launch the planes calls once apiece.  A batch codes them as ONE planes call over
 * a VIRTUAL buffer that exists nowhere:
 *        esize in {2, 4, 8}; chunk by the chunk rule; `count` items, item i = n[i] bytes at d_ptr[i], n[i] >= esize, n[i] % esize == 0
 *        m[i] = n[i] / esize;   nc[i] = ceil(m[i] / chunk);   first[i] = nc[0] + .. + nc[i - 1];   NC = first[count]
 *        V(items, esize, chunk) = the items in order, every item BUT THE LAST followed by zero elements up to nc[i] * chunk elements
 *        M = (NC - nc[count - 1]) * chunk + m[count - 1] elements,  M * esize bytes  (a batch has whole elements only: no tail)
 * The whole contract:  encode_batch(codec, items, ...)  ==  trc_encode_planes_dev(codec, V, M * esize, esize, chunk, ...)  byte for
 * byte -- directory, payload, totals, per-plane CDFs and statuses -- in buffers of that call's shapes: d_clen[esize * NC], planes
 * trc_planes_pitch(M * esize, esize) apart, d_total[esize], d_cdf at TRC_PLANES_CDF_STRIDE.  Item i owns chunks [first[i], first[i]
 * + nc[i]) of every plane, so "decode item i alone" is a chunk range; a batch of one item is the plain call on that item.
 *
 * `items` is a HOST array the caller may free or reuse as soon as a call returns: the call copies what its kernels need (32 bytes
 * per item) to the table on the device before it returns, and that copy waits for the work enqueued on `stream` before it;
 * everything else only enqueues work.  Items lie anywhere on the device, 16-byte aligned, and -- unlike every other entry point --
 * need NO TRC_PAD of readable slack: the kernels read bytes [0, n[i]) of item i and nothing else, a tensor may end where its
 * allocation ends.  Writes: split [0, M) of every plane, the pad zeros included; join [0, n[i]) of every requested item; the
 * coded calls their coded buffers, as the planes calls do.
 *
 * TRC_E_ARG, before anything is enqueued: count == 0 or > TRC_PLANES_BATCH_MAX, n[i] < esize or n[i] % esize != 0 (any item), a
 * bad esize or chunk, NC > 0x7fffffff, a d_ptr that is NULL or not 16-byte aligned on an item the call touches, first_item +
 * item_count > count, TRC_TABLES_READY / TRC_DIR_READY, the seven low-nibble coders.  A workspace or table that is too small is
 * TRC_E_WORK.  The work-bytes functions return 0 for what the calls reject (and for item_count == 0, which needs none).
 *
 * trc_planes_batch_plan_host (host only, no GPU needed) validates sizes, esize and chunk -- it looks at no pointer, so that a
 * caller who will decode a few items may plan with the others NULL -- and returns the figures of the equivalent planes call;
 * first_chunk (may be NULL) receives first[0 .. count].
 * The two kernels on their own: trc_planes_split_batch_dev writes the planes of V (d_planes 256-byte aligned, pitch a multiple
 * of 256 and at least M); trc_planes_join_batch_dev scatters items [first_item, first_item + item_count) back from planes whose
 * element 0 is the first requested item's first element (64-byte aligned, so d_planes + first[first_item] * chunk of a whole
 * batch's planes serves; pitch at least the elements of the range), looking at no other item's pointer.  d_table: 256-byte
 * aligned, trc_planes_batch_table_bytes(items the call touches, their chunks) bytes.  TRC_PLANES_GRID caps their grids as it
 * does the unbatched kernels'.
 * The coded calls: the batched split into the workspace, then trc_cdfini_dev (static coders) + trc_encode_dev per plane exactly
 * as trc_encode_planes_dev; decode runs trc_decode_range_dev per plane over chunks [first[first_item], first[first_item +
 * item_count)) and the batched join over them into the items' own d_ptr.  Items outside the range are not looked at beyond their
 * n, and their d_ptr may be NULL; item_count == 0 is TRC_OK with nothing enqueued.  Workspace: 256-byte aligned,
 * trc_planes_batch_work_bytes (encode) / trc_planes_batch_range_work_bytes (decode: grows with the requested chunks, not with M). */
#define TRC_PLANES_BATCH_MAX 1048576u          /* items per call */
typedef struct trc_planes_item { void *d_ptr; uint64_t n; } trc_planes_item;     /* host array; const for encode */
typedef struct trc_planes_batch_plan {
    uint64_t m_total;       /* M */
    uint64_t n_virtual;     /* M * esize: the n of the equivalent planes call */
    uint64_t chunks;        /* NC */
    uint64_t pitch;         /* trc_planes_pitch(n_virtual, esize) */
    uint64_t pad_elems;     /* zero elements added */
} trc_planes_batch_plan;
int    trc_planes_batch_plan_host(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                  trc_planes_batch_plan *plan, uint64_t *first_chunk);
size_t trc_planes_batch_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk);
size_t trc_planes_batch_range_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                         size_t first_item, size_t item_count);
int trc_planes_split_batch_dev(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                               void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream);
int trc_planes_join_batch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, size_t count,
                              size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                              void *d_table, size_t table_bytes, void *stream);
size_t trc_planes_batch_table_bytes(size_t count, uint64_t chunks);
int trc_encode_planes_batch_dev(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                void *d_work, size_t work_bytes, void *stream);
int trc_decode_planes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                const trc_planes_item *items, size_t count, size_t first_item, size_t item_count,
                                unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                void *d_work, size_t work_bytes, void *stream);

/* ---- batched byte planes with a predictor filter PER ITEM ------------------------------------------------------------------
 * The columns of a table and the pages of a cache are where the structure lies between neighbouring elements, and a table mixes
 * natures at one element width: ids and timestamps want the zigzag delta, float columns want nothing.  So the filter of a batch is
 * chosen per item.  `filters` is a HOST array of `count` bytes, filters[i] one of TRC_FILTER_NONE / ZDELTA / XOR, with the lifetime
 * rule of `items`: free again when the call returns.
 *        G(i)  = item i                                        where filters[i] == TRC_FILTER_NONE
 *              = F(filters[i], seg = chunk, esize, item i)     otherwise          (the F of the filtered planes; items have no tail)
 *        VF(items, filters, esize, chunk) = V([G(0), .., G(count - 1)], esize, chunk)
 * Every item is filtered as if it stood alone, then the virtual buffer is built as before: the predictor restarts at every chunk and
 * items start on chunk boundaries, so an item never sees its neighbour, the pad behind an item stays ZERO bytes in every plane (VF is
 * V of the filtered items, not F of V), and plan, M, NC, first[] and pitch are those of the unfiltered batch.
 * The whole contract:  encode_fbatch(codec, items, filters, ...)  ==  trc_encode_planes_dev(codec, VF, M * esize, esize, chunk, ...)
 * byte for byte -- directory, payload, totals, per-plane CDFs and statuses -- in buffers of that call's shapes.  So:
 *   - filters == NULL or all TRC_FILTER_NONE IS the unfiltered batched call of the same name, launching its kernels;
 *   - a batch of one item with filter f is trc_encode_fplanes_dev(codec, f, item, ...) on that item;
 *   - item i is still chunks [first[i], first[i] + nc[i]) of every plane and its inverse scan is local to them: any item range
 *     decodes alone, as before.
 *
 * Every argument, alignment, workspace and table rule is the one of the unfiltered batched call with the same name, the no-slack
 * read rule included (the kernels read bytes [0, n[i]) of item i and nothing else); trc_planes_batch_work_bytes,
 * trc_planes_batch_range_work_bytes and trc_planes_batch_table_bytes serve unchanged: the filter needs no workspace and travels in
 * the item's 32-byte record.  The join and the decoder take the filters of the WHOLE batch (count entries) and validate all of them.
 * Errors: those of the unfiltered calls, and TRC_E_ARG with the item's index in trc_last_error() for a filter id outside {0, 1, 2}.
 * The order of the checks is the plan (sizes, esize, chunk: host only), then the filters, then pointers and buffers -- so a bad
 * filter is reported without a device.  The seven low-nibble coders, TRC_TABLES_READY and TRC_DIR_READY are refused as before.
 * Any batch with a filter other than NONE runs one filtered split (join) kernel in place of the unfiltered one. */
int trc_planes_split_fbatch_dev(const trc_planes_item *items, const uint8_t *filters, size_t count, unsigned esize, uint32_t chunk,
                                void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream);
int trc_planes_join_fbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, size_t count,
                               size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               void *d_table, size_t table_bytes, void *stream);
int trc_encode_fplanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, size_t count, unsigned esize, uint32_t chunk,
                                 uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                 uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_decode_fplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                 const trc_planes_item *items, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                 unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_work, size_t work_bytes, void *stream);

/* ---- batched byte planes against a base per item ------------------------------------------------------------------------------
 * A checkpoint against the previous one is hundreds of tensors, each with its own base.  `bases` and `filters` are HOST arrays of
 * `count` entries with the lifetime rule of `items`; in THESE calls a filter id always means "against bases[i]" (the predecessor
 * filters are not available here; mixing the two is out of scope):
 *        G(i)  = item i                                   where filters[i] == TRC_FILTER_NONE   (bases[i] is not looked at)
 *                D(filters[i], esize, item i, bases[i])   otherwise                             (the filters against a base, above)
 * The whole contract:  encode  ==  trc_encode_planes_dev(codec, V([G(0) .. G(count - 1)], esize, chunk), ...)  byte for byte; the pad
 * stays zero; plan, M, NC, first[] and pitch are the unfiltered batch's.  filters == NULL or all TRC_FILTER_NONE IS the unfiltered
 * batched call and launches its kernels.  For an item the call touches with filter 1 or 2, bases[i] must be non-NULL and 16-byte
 * aligned; the kernels read [0, n[i]) of it and nothing else (no slack needed; its last partial vector is moved element by
 * element).  On decode bases[i] == items[i].d_ptr is the in-place case and is allowed; any OTHER overlap of a base with an item is
 * not checked and gives undefined results.  Order of checks: the plan (host only), the filters (the item's index in the message),
 * then pointers and buffers.  The base pointers travel as a uint64 array behind the chunk map of the table:
 * trc_planes_bbatch_table_bytes = trc_planes_batch_table_bytes + 8 * count rounded up to 256, and the work-bytes functions are the
 * unfiltered batch's plus that.  The join is elementwise (no scan).  The TRCB container has no place for a base: the TRCE
 * container below carries these batches. */
int trc_planes_split_bbatch_dev(const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                unsigned esize, uint32_t chunk, void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream);
int trc_planes_join_bbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const void *const *bases,
                               const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                               unsigned esize, uint32_t chunk, void *d_table, size_t table_bytes, void *stream);
size_t trc_planes_bbatch_table_bytes(size_t count, uint64_t chunks);
size_t trc_planes_bbatch_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk);
size_t trc_planes_bbatch_range_work_bytes(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                          size_t first_item, size_t item_count);
int trc_encode_bplanes_batch_dev(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                 unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                 uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_decode_bplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload, const trc_planes_item *items,
                                 const void *const *bases, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                 unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_work, size_t work_bytes, void *stream);

/* ---- the batch advisor: which filter for which item? -------------------------------------------------------------------------
 * The planes advisor above reads one contiguous buffer with TRC_PAD behind it; the items of a batch are neither.  These calls are
 * that advisor over the batch's pointer table: ONE launch reads every item of an item range once and leaves the plane histograms
 * of every requested filter per item, and a host function turns them into one filter id per item by the same 1/64 rule.
 *
 * trc_planes_hist_batch_dev(filters, items, count, first_item, item_count, esize, chunk, d_hist, d_table, table_bytes, stream).
 * The whole contract: for j in [0, item_count) the 3 * esize * 256 counters at d_hist + j * 3 * esize * 256 equal, exactly, what
 *        trc_planes_hist_dev(filters, items[first_item + j].d_ptr, items[first_item + j].n, esize, seg = chunk, ...)
 * writes: the predictor restarts every `chunk` elements of the item (where the filtered batch calls restart it), the batch's pad
 * elements are counted nowhere, rows of filters not requested stay zero -- so every slice serves trc_planes_advise as it stands.
 * The call zeroes trc_planes_hist_batch_bytes(item_count, esize) = item_count * trc_planes_hist_bytes(esize) bytes on the stream
 * first and writes nothing behind them.  It keeps the batch's no-slack rule: it reads bytes [0, n[i]) of a requested item and
 * nothing else.  Items outside the range are looked at for their n only, and their d_ptr may be NULL; item_count == 0 is TRC_OK with
 * nothing enqueued.  Checks, in this order: the plan (sizes, esize, chunk: host only), filters in 1 .. 7, the range, the pointers
 * (the requested items' as in the other batched calls, d_hist 8-byte aligned), the table: 256-byte aligned,
 * trc_planes_batch_table_bytes(item_count, the chunks of the range) bytes, TRC_E_WORK where it is smaller.  `items` is free again
 * when the call returns, as in the other batched calls; apart from that upload the call only enqueues work.  TRC_PLANES_GRID and
 * TRC_PLANES_HIST_ROUND_VECS act as on trc_planes_hist_dev.
 *
 * trc_planes_advise_batch (host only, no GPU needed): entry i of filters_out (and of advice, count entries, may be NULL) is exactly
 * what trc_planes_advise(hist + i * 3 * esize * 256, filters, esize, n[i] / esize, &a) gives -- same estimates, same ties, same 1/64
 * rule.  It looks at no d_ptr.  Where an item fails (a row that does not sum to its elements, n[i] no whole number of elements) the
 * call returns TRC_E_ARG with that item's index in trc_last_error() and writes nothing to filters_out (entries of advice in front
 * of the failing item may have been written); count == 0, a bad esize or filters outside 1 .. 7 are TRC_E_ARG as well.
 *
 * trc_planes_advise_batch_dev does both and SYNCHRONISES: it is the one device call of this header that waits for `stream`, because
 * the choice is made on the host (the choice must be trc_planes_advise's bit for bit, and a device log2 would not promise that at
 * the 1/64 edge).  It walks the batch in slabs of consecutive items whose histograms fit TRC_PLANES_ADVISE_SLAB_BYTES: per slab
 * trc_planes_hist_batch_dev, a copy of the histograms to the host, trc_planes_advise_batch.  The result is what the three pieces
 * give when called by hand on the whole batch.  d_work: 256-byte aligned, trc_planes_advise_batch_work_bytes bytes = the slab's
 * histograms and the table of the largest slab; it does not grow with count beyond that (0 for what the call rejects).
 * TRC_PLANES_ADVISE_SLAB_ITEMS in the environment lowers the items per slab (test aid).  Every item's d_ptr is read.  On an error
 * nothing is written to filters_out. */
#define TRC_PLANES_ADVISE_SLAB_BYTES (8u << 20)
size_t trc_planes_hist_batch_bytes(size_t item_count, unsigned esize);   /* 0 for a bad esize / 0 items */
int    trc_planes_hist_batch_dev(unsigned filters, const trc_planes_item *items, size_t count,
                                 size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                                 uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);
int    trc_planes_advise_batch(const uint64_t *hist, unsigned filters, unsigned esize,
                               const trc_planes_item *items, size_t count,
                               uint8_t *filters_out, trc_planes_advice *advice /* count entries, may be NULL */);
size_t trc_planes_advise_batch_work_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk);
int    trc_planes_advise_batch_dev(unsigned filters, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                   uint8_t *filters_out, trc_planes_advice *advice,
                                   void *d_work, size_t work_bytes, void *stream);

/* ---- batched byte planes: the TRCB container, packed on the device -------------------------------------------------------------
 * A coded batch is loose device buffers (d_clen, payload planes `pitch` apart -- as large as the input --, d_total, CDFs) and a
 * caller who remembers codec, esize, chunk, cdfnum, every item's length and every item's filter.  The TRCB container is the same
 * batch in ONE compact, self-describing piece, little endian:
 *   trc_planes_batch_hdr (48 B) | uint64 n[count] | uint8 filter[count], zero-padded to a multiple of 8 | inner
 *   inner = the TRCP container of VF(items, filters, esize, chunk):  n = M * esize, tail = 0
 * The whole contract: bytes [inner, size) are byte for byte what trc_encode_planes_host(codec, VF, M * esize, esize, chunk, ...)
 * writes at the same chunk, with VF, M and first[] those of the batched calls above; unfiltered items are filter 0, and a batch
 * without filters stores `count` zero bytes (one layout).  So trc_planes_check, trc_container_check and trc_container_range work
 * on the inner part and its sections as they stand, and item i is chunks [first[i], first[i] + nc[i]) of every section.
 *
 * Host only, no GPU needed:
 *   trc_planes_batch_auto_chunk   what chunk 0 means: the chunk trc_encode_planes_host resolves for n = sum n[i] (trc_auto_chunk_codec
 *                                 on the element count, then the coder's floor and largest chunk); 0 for a bad batch or coder.
 *   trc_planes_batch_bound        48 + table + trc_planes_bound(M * esize, esize, chunk, cdfnum) + TRC_PAD: what d_out / out must
 *                                 hold (the container is always shorter); chunk 0 as above; 0 for what the calls reject.  It looks
 *                                 at no pointer.
 *   trc_planes_batch_layout_host  from the planes' payload sizes total[esize]: `inner`, off[k] = where the inner container's section
 *                                 k starts (from the TRCB start; a multiple of 8; a static coder's CDF, up8(2 (cdfnum + 1)) bytes,
 *                                 then the 32-byte TRC1 header, the directory, the payload) and `size`.  TRC_E_ARG where total[k] > M.
 *   trc_planes_batch_check        (count_expected (size_t)-1 = any) magic, version, both zero fields, esize, the chunk rule, count,
 *                                 inner == 48 + 8 count + up8(count), inner < size <= buflen, every n[i] a whole number (at least one)
 *                                 of elements, filters in {0, 1, 2}, zero filter padding, bytes == sum n[i], NC <= 0x7fffffff,
 *                                 trc_planes_check(buf + inner, size - inner, M * esize), and the inner header's esize and chunk
 *                                 equal to the outer ones, its tail 0, its size == size - inner.  A failure leaves the reason in
 *                                 trc_last_error(), prefixed "batch container:", naming the item where one is at fault.
 *   trc_planes_batch_info         the check, then the header and the first min(cap, count) table entries (n, filters: may be NULL):
 *                                 what a reader allocates by.
 *
 * trc_planes_batch_pack_dev writes the container in device memory from the outputs of trc_encode_(f)planes_batch_dev for these items
 * and filters (filters NULL = none), WITHOUT a host round trip: one kernel whose workgroups each re-derive the section offsets from
 * d_total and copy their share of directories, payloads and CDFs, write the headers and the zero bytes up to every multiple of 8.
 * When `stream` reaches the end of the call d_out[0, size) is the container and *d_size = size.  d_out 16-byte, d_size 8-byte aligned;
 * out_bytes >= trc_planes_batch_bound, else TRC_E_WORK; nothing at or behind d_out + size is written.  Checks: those of the batched
 * decode -- the plan, then the filters, then the buffers; no d_ptr is looked at.  The call only enqueues work, but for the upload of
 * the host-known front (header with `size` still open, n[], filters), which follows the lifetime rule of the batched calls' table:
 * items and filters are free again on return.  Where a static coder's d_status[k] < 0 or d_total[k] > M the kernel stores *d_size = 0
 * and d_out is undefined.  TRC_PLANES_GRID caps the grid as it does the other plane kernels'.
 *
 * trc_decode_planes_batch_packed_dev decodes items [first_item, first_item + item_count) straight from a container in device memory
 * (8-byte aligned, cont_bytes >= size, TRC_PAD readable bytes behind `size`: a buffer of trc_planes_batch_bound bytes has them):
 * plane k's directory, payload and CDF are read where they lie.  `total` is a HOST array of the planes' payload sizes (the payload
 * field of the sections' headers) from which trc_planes_batch_layout_host gives the offsets; layout.size > cont_bytes is TRC_E_ARG.
 * Otherwise the call is trc_decode_fplanes_batch_dev: same checks, workspace (trc_planes_batch_range_work_bytes), launches; it only
 * enqueues work and trusts d_cont as every _dev call trusts its buffers.
 *
 * Through host pointers (the caller's current device, no striping): `out` is host memory; items_on says where the ITEMS lie --
 * TRC_ITEMS_DEV: d_ptr are device addresses as in the batched calls; TRC_ITEMS_HOST: host addresses of any alignment, gathered
 * through a page-locked staging buffer so that thousands of small items do not pay a copy apiece.  Encode: the batched encode, the
 * pack kernel, one synchronise to read *d_size, one copy of `size` bytes; returns the size, 0 on error.  chunk 0 =
 * trc_planes_batch_auto_chunk; cdfnum as for trc_encode_planes_host.  trc_encode_aplanes_batch_host asks the batch advisor first
 * (trc_planes_advise_batch_dev, all three filters) and writes exactly what the explicit call writes for that list, which filters_out
 * (count bytes, may be NULL) receives.  The low-nibble coders and a bad filter id are refused before any device is needed.
 * trc_decode_planes_batch_host checks the container (trc_planes_batch_check with `count`), wants items[i].n == n[i] for ALL count
 * entries (d_ptr may be NULL outside the range), sends only the covering chunks of every section and joins into the items; returns
 * the bytes delivered, 0 on error.  trc_decode_xplanes_host does not take this container. */
#define TRC_PLANES_BATCH_MAGIC 0x42435254u   /* "TRCB" */
typedef struct trc_planes_batch_hdr {
    uint32_t magic;      /* TRC_PLANES_BATCH_MAGIC */
    uint8_t  version;    /* 1 */
    uint8_t  esize;      /* 2, 4 or 8 */
    uint16_t zero;
    uint32_t chunk;
    uint32_t zero2;
    uint64_t count;      /* items, 1 .. TRC_PLANES_BATCH_MAX */
    uint64_t inner;      /* offset of the TRCP container = 48 + 8 count + up8(count) */
    uint64_t size;       /* the whole container */
    uint64_t bytes;      /* sum of n[i] */
} trc_planes_batch_hdr;  /* 48 bytes, little endian */
typedef struct trc_planes_batch_layout {
    uint64_t inner;      /* offset of the inner TRCP container */
    uint64_t off[8];     /* section k of the inner container, from the TRCB start */
    uint64_t size;       /* the whole container */
} trc_planes_batch_layout;
enum { TRC_ITEMS_HOST = 0, TRC_ITEMS_DEV = 1 };
uint32_t trc_planes_batch_auto_chunk(int codec, const trc_planes_item *items, size_t count, unsigned esize);
size_t trc_planes_batch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum);
int    trc_planes_batch_layout_host(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                    unsigned cdfnum, const uint64_t *total, trc_planes_batch_layout *L);
int    trc_planes_batch_check(const void *buf, size_t buflen, size_t count_expected);
int    trc_planes_batch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, size_t cap);
int trc_planes_batch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, size_t count,
                              unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                              const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                              const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream);
int trc_decode_planes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                       const trc_planes_item *items, const uint8_t *filters, size_t count, size_t first_item, size_t item_count,
                                       unsigned esize, uint32_t chunk, unsigned cdfnum, const uint64_t *total /* host, esize entries */,
                                       void *d_work, size_t work_bytes, void *stream);
size_t trc_encode_planes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters /* NULL: none */,
                                    size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                    void *out, size_t outcap);
size_t trc_encode_aplanes_batch_host(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk,
                                     unsigned cdfnum, int items_on, void *out, size_t outcap, uint8_t *filters_out /* may be NULL */);
size_t trc_decode_planes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                    size_t first_item, size_t item_count, int items_on);

/* ---- batched byte planes with a filter AND A STRIDE per item: interleaved items in a batch ------------------------------------
 * A table handed over as a batch often has items that are row-major blocks of K same-width fields -- (id, t0, t1, counter) rows,
 * xyz(w) points, stereo or 5.1 PCM pages, complex pairs -- next to plain columns and float tensors.  For such an item the predictor
 * of the filtered batch, the element directly in front, is worse than none; the strided filter above predicts from the element K
 * back.  Here the stride is chosen per item, as the filter is.  `strides` is a HOST array of `count` bytes with the lifetime rule
 * of `items` and `filters`; every entry must be in 1 .. TRC_STRIDE_MAX.
 *        GS(i) = item i                                                  where filters[i] == TRC_FILTER_NONE   (strides[i] has no effect)
 *              = F_{strides[i]}(filters[i], seg = chunk, esize, item i)  otherwise     (the F_S of the strided planes; items have no tail)
 *        VS(items, filters, strides, esize, chunk) = V([GS(0) .. GS(count - 1)], esize, chunk)
 * Unchanged from the filtered batch: plan, M, NC, first[], pitch, table bytes and workspace; the pad behind an item, zero bytes in
 * every plane; the predictor restarting at every chunk of the item, whether or not S divides the chunk; item i being chunks
 * [first[i], first[i] + nc[i]) of every plane, any item range decoding alone; and items needing no readable slack: the kernels read
 * bytes [0, n[i]) of an item and nothing else.
 * The whole contract:  encode_sbatch(codec, items, filters, strides, ...)  ==  trc_encode_planes_dev(codec, VS, M * esize, esize,
 * chunk, ...) byte for byte -- directory, payload, totals, per-plane CDFs and statuses.  So:
 *   - strides == NULL, or 1 for every item whose filter is not NONE, IS the fplanes_batch call of the same kind and launches exactly
 *     its kernels (and says so in its messages);
 *   - a batch of one item with filter f and stride s is trc_encode_splanes_dev(codec, f, s, item, ...) on that item.
 * The arguments are those of the fbatch calls with `strides` behind `filters`; join and decode take the strides of the WHOLE batch.
 * Errors: those of the fbatch calls, and TRC_E_ARG with the item's index in trc_last_error() for a stride outside
 * 1 .. TRC_STRIDE_MAX.  The order of the checks is the plan, then the filters, then the strides, then pointers and buffers -- so a
 * bad stride is reported without a device.  The stride travels in the item's 32-byte record next to the filter.
 *
 * trc_planes_hist_sbatch_dev is trc_planes_hist_batch_dev under the items' strides: slice j is exactly what
 * trc_planes_hist_stride_dev(filters, strides[first_item + j], item, n, esize, seg = chunk, ...) writes for that item alone, so
 * trc_planes_advise_batch serves on it unchanged.  (`filters` is that call's bit set; the checks are the plan, the bit set, the
 * strides, the range, pointers, table.)  trc_planes_advise_sbatch_dev is trc_planes_advise_batch_dev over these histograms -- same
 * workspace function, same slabs, same synchronise: it picks the filter per item under the caller's strides and searches no strides.
 *
 * The TRCT container.  trc_planes_batch_check rejects other versions and non-zero reserved fields of TRCB, so the strides do not go
 * into it: as TRCS does for TRCF, a prefix carries them, little endian:
 *   trc_planes_sbatch_hdr (16 B) | uint8 stride[count], zero-padded to a multiple of 16 | the TRCB container of the batch
 * The TRCB front is as for (items, filters), the inner TRCP container is that of VS, and the TRCB header's `size` is the TRCB part's
 * own: the whole size is prefix + that, prefix = 16 + up16(count).  The stored stride of an item without a filter is 1.  One layout
 * per content: a batch in which no item with a filter has a stride above 1 is a TRCB container, and trc_encode_splanes_batch_host and
 * trc_planes_sbatch_pack_dev refuse it (TRC_E_ARG, naming trc_encode_planes_batch_host / trc_planes_batch_pack_dev).
 * Host only, no GPU needed:
 *   trc_planes_sbatch_bound   trc_planes_batch_bound + prefix; 0 for what the calls reject.
 *   trc_planes_sbatch_check   magic, version, the zero fields, count in 1 .. TRC_PLANES_BATCH_MAX (and == count_expected unless that is
 *                             (size_t)-1), the prefix within buflen, strides in 1 .. TRC_STRIDE_MAX, zero padding, then
 *                             trc_planes_batch_check on the rest, its count equal to the prefix's, and stride 1 wherever the filter is
 *                             NONE.  A failure leaves the reason in trc_last_error(), prefixed "strided batch container:".
 *   trc_planes_sbatch_info    trc_planes_batch_info (the TRCB header, n, filters) plus the strides: the first min(cap, count) entries
 *                             of each (n, filters, strides: may be NULL), nothing behind them.
 * trc_planes_sbatch_pack_dev uploads the host-known prefix and runs trc_planes_batch_pack_dev on d_out + prefix (a multiple of 16, so
 * that call's alignment holds); *d_size comes out as the WHOLE size (0 as there), on the stream, without a host round trip.
 * out_bytes >= trc_planes_sbatch_bound.  The checks are the plan, the filters, the strides, then those of that call.
 * trc_decode_splanes_batch_packed_dev is trc_decode_planes_batch_packed_dev on a TRCT container: d_cont is its start (16-byte
 * aligned), cont_bytes and TRC_PAD count from there; `strides` are the caller's, as `filters` are.
 * trc_encode_splanes_batch_host / trc_decode_splanes_batch_host mirror the TRCB pair, TRC_ITEMS_HOST / TRC_ITEMS_DEV included; the
 * decoder takes filters and strides from the container.  trc_decode_xplanes_host does not take this container either. */
#define TRC_PLANES_SBATCH_MAGIC 0x54435254u   /* "TRCT" */
typedef struct trc_planes_sbatch_hdr {
    uint32_t magic;      /* TRC_PLANES_SBATCH_MAGIC */
    uint8_t  version;    /* 1 */
    uint8_t  zero;
    uint16_t zero2;
    uint64_t count;      /* items: that of the TRCB container behind the strides */
} trc_planes_sbatch_hdr; /* 16 bytes, little endian */
size_t trc_planes_sbatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum);
int    trc_planes_sbatch_check(const void *buf, size_t buflen, size_t count_expected);
int    trc_planes_sbatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint8_t *strides, size_t cap);
int trc_planes_sbatch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                               unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                               const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                               const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream);
int trc_decode_splanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                        const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                        size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                        const uint64_t *total /* host, esize entries */, void *d_work, size_t work_bytes, void *stream);
size_t trc_encode_splanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                                     size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                     void *out, size_t outcap);
size_t trc_decode_splanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                     size_t first_item, size_t item_count, int items_on);
int trc_planes_split_sbatch_dev(const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count, unsigned esize,
                                uint32_t chunk, void *d_planes, size_t pitch, void *d_table, size_t table_bytes, void *stream);
int trc_planes_join_sbatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                               size_t count, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               void *d_table, size_t table_bytes, void *stream);
int trc_encode_splanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                 unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                 uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_decode_splanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                 const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, size_t count,
                                 size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_planes_hist_sbatch_dev(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count,
                               size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);
int trc_planes_advise_sbatch_dev(unsigned filters, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize,
                                 uint32_t chunk, uint8_t *filters_out, trc_planes_advice *advice,
                                 void *d_work, size_t work_bytes, void *stream);

/* ---- batched byte planes: a predictor ORDER per item -----------------------------------------------------------------------------
 * A batch mixes natures at one element width: sensor channels want order 2 or 3, sorted ids and timestamps want order 1 and store more
 * at order 2, float tensors want no filter.  Here the order of the oplanes calls is chosen per item, as filter and stride are.
 * `orders` is a HOST array of `count` bytes with the lifetime rule of `items`, `filters` and `strides`; every entry must be in
 * 1 .. TRC_ORDER_MAX.  An entry has an effect only where filters[i] == TRC_FILTER_ZDELTA: xor has no order, the filter enum is untouched.
 *        GO(i) = item i                                                         where filters[i] == TRC_FILTER_NONE
 *              = F_{strides[i]}(TRC_FILTER_XOR, seg = chunk, esize, item i)     where filters[i] == TRC_FILTER_XOR
 *              = O(orders[i], strides[i], seg = chunk, esize, item i)           where filters[i] == TRC_FILTER_ZDELTA
 *                                                                               (the O of the oplanes section; items have no tail)
 *        VO(items, filters, strides, orders, esize, chunk) = V([GO(0) .. GO(count - 1)], esize, chunk)
 * Unchanged from the strided batch: plan, M, NC, first[], pitch, table bytes and workspace; the pad behind an item, zero bytes in
 * every plane; the predictor restarting at every chunk of the item, whether or not S divides the chunk; item i being chunks
 * [first[i], first[i] + nc[i]) of every plane, any item range decoding alone; and items needing no readable slack: the kernels read
 * bytes [0, n[i]) of an item and nothing else.
 * The whole contract:  encode_obatch(codec, items, filters, strides, orders, ...)  ==  trc_encode_planes_dev(codec, VO, M * esize,
 * esize, chunk, ...) byte for byte -- directory, payload, totals, per-plane CDFs and statuses.  So:
 *   - orders == NULL, or 1 for every ZDELTA item, IS the sbatch call of the same kind (which is the fbatch or plain batch call where
 *     that section says so), launches exactly those kernels and names itself so in its messages;
 *   - the order travels in the item's 32-byte record next to filter and stride (order - 1 in bits 59 .. 60 of v0): a record of
 *     order 1 is the sbatch record bit for bit;
 *   - a batch of one item with filter ZDELTA, order k and stride s is trc_encode_oplanes_dev(codec, k, s, item, ...) on that item.
 * The arguments are those of the sbatch calls with `orders` behind `strides`; join and decode take the orders of the WHOLE batch.
 * Errors: those of the sbatch calls, and TRC_E_ARG with the item's index in trc_last_error() for an order outside
 * 1 .. TRC_ORDER_MAX.  The order of the checks is the plan, the filters, the strides, the orders, then pointers and buffers -- so a
 * bad order is reported without a device.
 *
 * trc_planes_hist_obatch_dev counts every item of an item range under the orders of the bit set `orders_set` (bit k = order k,
 * 1 .. 15) at the item's stride: slice j is exactly what trc_planes_hist_order_dev(orders_set, strides[first_item + j], item, n,
 * esize, seg = chunk, ...) writes for that item alone, trc_planes_hist_order_bytes(esize) bytes; trc_planes_hist_obatch_bytes(item_count,
 * esize) is the size (0 for a bad esize or no items).  Checks, zeroing, range rules and table: those of trc_planes_hist_sbatch_dev.
 * trc_planes_advise_obatch (host only) gives per item exactly trc_planes_advise_order's choice on the item's slice, as
 * filters_out[i] (NONE for order 0, else ZDELTA) and orders_out[i] (the order; 1 where the filter is NONE); advice: NULL or `count`
 * entries.  It fails as trc_planes_advise_batch does, and on an error nothing is written to filters_out, orders_out or advice.
 * trc_planes_advise_obatch_dev is the slab walk of trc_planes_advise_batch_dev over these histograms: the same
 * TRC_PLANES_ADVISE_SLAB_BYTES, the same TRC_PLANES_ADVISE_SLAB_ITEMS aid, the same synchronise; a workspace function of its own
 * (a slice is 4/3 of a filter slice, so a slab holds 3/4 of the items).  It searches orders under the caller's strides (NULL: 1); it
 * searches no strides and no xor.
 *
 * The TRCU container: the prefix of TRCT with the orders behind the strides, little endian:
 *   trc_planes_obatch_hdr (16 B) | uint8 stride[count], zero-padded to a multiple of 16 | uint8 order[count], likewise
 *   | the TRCB container of (items, filters), whose inner TRCP container is that of VO
 * prefix = 16 + 2 * up16(count).  The stored stride of an item without a filter is 1, the stored order of an item whose filter is
 * not ZDELTA is 1.  One layout per content: a batch in which no ZDELTA item has an order above 1 is a TRCT or TRCB container, and
 * trc_planes_obatch_pack_dev and trc_encode_oplanes_batch_host refuse it (TRC_E_ARG, naming the calls that take it).
 * Host only, no GPU needed:
 *   trc_planes_obatch_bound   trc_planes_batch_bound + prefix; 0 for what the calls reject.
 *   trc_planes_obatch_check   magic, version, the zero fields, count (and == count_expected unless that is (size_t)-1), the prefix
 *                             within buflen, strides in 1 .. TRC_STRIDE_MAX, orders in 1 .. TRC_ORDER_MAX, zero padding, then
 *                             trc_planes_batch_check on the rest, its count equal to the prefix's, stride 1 wherever the filter is
 *                             NONE, order 1 wherever it is not ZDELTA, and at least one order above 1.  A failure leaves the reason
 *                             in trc_last_error(), prefixed "ordered batch container:".
 *   trc_planes_obatch_info    trc_planes_sbatch_info plus the orders.
 * trc_planes_obatch_pack_dev, trc_decode_oplanes_batch_packed_dev, trc_encode_oplanes_batch_host and trc_decode_oplanes_batch_host
 * are the TRCT calls with the orders; the decoder takes filters, strides and orders from the container.
 * trc_encode_aoplanes_batch_host: the order advisor (all four orders) under the caller's strides (NULL: 1), then the coded call; the
 * output is byte for byte what the explicit call for that choice writes -- TRCB, TRCT or TRCU; out must hold
 * trc_planes_obatch_bound bytes; filters_out / orders_out (may be NULL) receive the choice.
 * trc_decode_xplanes_host does not take this container either. */
#define TRC_PLANES_OBATCH_MAGIC 0x55435254u   /* "TRCU" */
typedef struct trc_planes_obatch_hdr {
    uint32_t magic;      /* TRC_PLANES_OBATCH_MAGIC */
    uint8_t  version;    /* 1 */
    uint8_t  zero;
    uint16_t zero2;
    uint64_t count;      /* items: that of the TRCB container behind the strides and orders */
} trc_planes_obatch_hdr; /* 16 bytes, little endian */
size_t trc_planes_obatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum);
int    trc_planes_obatch_check(const void *buf, size_t buflen, size_t count_expected);
int    trc_planes_obatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint8_t *strides,
                              uint8_t *orders, size_t cap);
int trc_planes_obatch_pack_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                               size_t count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                               const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                               const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size, void *stream);
int trc_decode_oplanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                        const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                        size_t count, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                        const uint64_t *total /* host, esize entries */, void *d_work, size_t work_bytes, void *stream);
size_t trc_encode_oplanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                                     const uint8_t *orders, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                     void *out, size_t outcap);
size_t trc_decode_oplanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, size_t count,
                                     size_t first_item, size_t item_count, int items_on);
size_t trc_encode_aoplanes_batch_host(int codec, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize,
                                      uint32_t chunk, unsigned cdfnum, int items_on, void *out, size_t outcap,
                                      uint8_t *filters_out, uint8_t *orders_out);
int trc_planes_split_obatch_dev(const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                size_t count, unsigned esize, uint32_t chunk, void *d_planes, size_t pitch,
                                void *d_table, size_t table_bytes, void *stream);
int trc_planes_join_obatch_dev(const void *d_planes, size_t pitch, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides,
                               const uint8_t *orders, size_t count, size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               void *d_table, size_t table_bytes, void *stream);
int trc_encode_oplanes_batch_dev(int codec, const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders,
                                 size_t count, unsigned esize, uint32_t chunk, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status,
                                 uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_decode_oplanes_batch_dev(int codec, const uint32_t *d_clen, const void *d_payload,
                                 const trc_planes_item *items, const uint8_t *filters, const uint8_t *strides, const uint8_t *orders, size_t count,
                                 size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                                 void *d_work, size_t work_bytes, void *stream);
size_t trc_planes_hist_obatch_bytes(size_t item_count, unsigned esize);
int trc_planes_hist_obatch_dev(unsigned orders_set, const trc_planes_item *items, const uint8_t *strides, size_t count,
                               size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);
int trc_planes_advise_obatch(const uint64_t *hist, unsigned orders_set, unsigned esize, const trc_planes_item *items, size_t count,
                             uint8_t *filters_out, uint8_t *orders_out, trc_planes_order_advice *advice);
size_t trc_planes_advise_obatch_work_bytes(const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk);
int trc_planes_advise_obatch_dev(unsigned orders_set, const trc_planes_item *items, const uint8_t *strides, size_t count, unsigned esize,
                                 uint32_t chunk, uint8_t *filters_out, uint8_t *orders_out, trc_planes_order_advice *advice,
                                 void *d_work, size_t work_bytes, void *stream);

/* ---- batched byte planes against a base per item: fingerprints per base, the TRCE container --------------------------------------
 * A batch coded against bases decodes silently wrong against any other base, and in place it destroys that base.  So a container of
 * such a batch names every base by its fingerprint (trc_base_fingerprint_host, above), and the fingerprints of a whole batch come
 * from ONE launch.
 *
 * trc_base_fingerprint_batch_dev: for j in [0, item_count), i = first_item + j:
 *        d_fp[j] = trc_base_fingerprint_host(bases[i], items[i].n)   where filters[i] != TRC_FILTER_NONE
 *                = 0                                                 otherwise (bases[i] is not looked at and may be NULL)
 * exactly: the sum wraps mod 2^64, so every order of addition gives the same value.  The call zeroes d_fp[0, item_count) on the
 * stream first.  It reads bytes [0, n[i]) of a requested base and nothing else (whole 16-byte words, the bytes behind them one by
 * one: no slack needed); no d_ptr is looked at.  The work is cut by bytes, not by items: a 200 MB base is shared by many workgroups,
 * thousands of 4 KiB bases share a few.  Checks, in this order: the items (1 .. TRC_PLANES_BATCH_MAX of them, none empty), the
 * filters, the range, the pointers (a requested base non-NULL and 16-byte aligned, d_fp 8-byte aligned), the table: 256-byte
 * aligned, trc_base_fingerprint_batch_table_bytes(item_count) bytes (32 per item for the records and 8 per item that
 * trc_base_verify_batch_dev uses, each rounded up to 256; 0 for 0 or too many items), TRC_E_WORK where it is smaller.
 * item_count == 0 is TRC_OK with nothing enqueued.  `items`, `bases` and `filters` are free again when the call returns; apart from
 * that upload the call only enqueues work.  TRC_PLANES_GRID caps the grid as it does the other plane kernels'.
 *
 * The TRCE container, little endian, mirrors TRCT -- a prefix in front of an unchanged TRCB container:
 *   trc_planes_bbatch_hdr (16 B) | uint64 base_fp[count], zero-padded so that the prefix is a multiple of 16 | the TRCB container
 * The TRCB part is that of (items, filters) with the inner TRCP container of V([G(0) .. G(count - 1)]), G as above: byte for byte
 * what trc_planes_batch_pack_dev writes for the outputs of trc_encode_bplanes_batch_dev, its header's `size` its own -- so
 * trc_planes_batch_check, trc_planes_batch_info and trc_planes_check work on that part as they stand.  base_fp[i] is the
 * fingerprint of bases[i] over n[i] bytes (a base's length is its item's and is not stored), 0 for an item without a filter.  One
 * layout per content: a batch in which every filter is NONE is a TRCB container, and trc_planes_bbatch_pack_dev refuses it
 * (TRC_E_ARG, naming trc_planes_batch_pack_dev).
 * Host only, no GPU needed:
 *   trc_planes_bbatch_bound   trc_planes_batch_bound + prefix, prefix = 16 + up16(8 count); 0 for what the calls reject.
 *   trc_planes_bbatch_check   in this order: magic, version, the zero fields, count in 1 .. TRC_PLANES_BATCH_MAX (and == count_expected
 *                             unless that is (size_t)-1), the prefix within buflen, zero padding, trc_planes_batch_check on the rest,
 *                             its count equal to the prefix's, base_fp[i] == 0 wherever filter[i] is NONE, at least one filter set.
 *                             A failure leaves the reason in trc_last_error(), prefixed "based batch container:", naming the item.
 *   trc_planes_bbatch_info    trc_planes_batch_info (the TRCB header, n, filters) plus the first min(cap, count) fingerprints
 *                             (n, filters, base_fp: may be NULL), nothing behind them.
 * trc_planes_bbatch_pack_dev writes the container in device memory without a host round trip: the 16-byte header (an upload), the
 * zero padding, trc_base_fingerprint_batch_dev with d_fp = d_out + 16, trc_planes_batch_pack_dev on d_out + prefix (a multiple of
 * 16, so that call's alignment holds); *d_size comes out as the WHOLE size (0 as there).  out_bytes >= trc_planes_bbatch_bound, the
 * table that of the fingerprint call for `count` items; nothing at or behind d_out + size is written.  Checks: the plan, the
 * filters, the all-NONE refusal, the bases, the table, then those of trc_planes_batch_pack_dev; nothing is enqueued unless all pass.
 * trc_decode_bplanes_batch_packed_dev is trc_decode_planes_batch_packed_dev on a TRCE container: d_cont is its start (16-byte
 * aligned), cont_bytes and TRC_PAD count from there, `bases` stand next to `filters` (bases[i] == items[i].d_ptr: in place), the
 * workspace is trc_planes_bbatch_range_work_bytes.  It trusts its buffers as every _dev call does and does NOT verify the bases.
 * trc_base_verify_batch_dev fingerprints the bases of items [first_item, first_item + item_count) (the call above, into the
 * table's second part) and a small kernel writes *d_bad (8-byte aligned, device): the lowest item index whose fingerprint differs
 * from the base_fp of the container at d_cont (device, 8-byte aligned; only its prefix is read), or -1.  A batch range holds whole items, so every requested base is seen whole.  It only enqueues
 * work (but for the table upload): the caller decides whether to wait for *d_bad before a decode in place.  The decode does not
 * gate on it because that would put a flag read into every join kernel, or a host round trip into a call that only enqueues: the
 * join kernels stay as they are, and a caller who cannot afford a wrong base reads *d_bad first.
 *
 * Through host pointers (TRC_ITEMS_HOST / TRC_ITEMS_DEV as for TRCB; the BASES lie where the items lie): trc_encode_bplanes_batch_host
 * is the batched encode against the bases and trc_planes_bbatch_pack_dev, one synchronise to read the size, one copy; it returns the
 * size, 0 on error, and refuses an all-NONE batch (naming trc_encode_planes_batch_host), a bad filter id and the low-nibble coders
 * before any device is needed.  trc_decode_bplanes_batch_host checks the container, wants items[i].n == n[i] for ALL entries, uploads
 * (or uses) only the requested items' bases and compares their fingerprints with the container's BEFORE anything is decoded: on a
 * mismatch it returns 0 with "base fingerprint", the item's index and both values in trc_last_error(), and no output is touched.  A
 * wrong base outside the range is not looked at.  bases[i] == items[i].d_ptr is the in-place case.  It also reads a plain TRCB
 * container (no item has a base: `bases` is ignored and may be NULL).
 *
 * The advisor against bases, per item.  trc_planes_hist_bbatch_dev is trc_planes_hist_batch_dev with item i predicted from
 * bases[i]: slice j is exactly what trc_planes_hist_base_dev(filters, item, base, n, esize, ...) writes for item first_item + j
 * alone -- no restart, no seg (`chunk` shapes the plan and the walk only), pad elements counted nowhere.  An item whose base is NULL
 * (or bases == NULL) gets the unfiltered row alone: rows 1 and 2 of its slice stay zero.  A base is 16-byte aligned, and bytes
 * [0, n[i]) of it are read, nothing else.  Same d_hist, table (trc_planes_batch_table_bytes: the base's address travels in the
 * item's record), checks and order as trc_planes_hist_batch_dev.  trc_planes_advise_bbatch (host only) gives per item what
 * trc_planes_advise gives on the item's slice under the bit set filters & (bases[i] ? 7 : 1) -- same estimates, ties and 1/64 rule --
 * so an item with no base is never given a filter (and is TRC_E_ARG, naming the item, where `filters` lacks the unfiltered row).
 * trc_planes_advise_bbatch_dev does both, with the slabs, the workspace function (trc_planes_advise_batch_work_bytes) and the single
 * synchronise per slab of trc_planes_advise_batch_dev.  trc_encode_abplanes_batch_host asks it first (all three filters) and writes
 * exactly the container the explicit call writes for the chosen list, which filters_out (count bytes, may be NULL) receives: TRCE,
 * or TRCB where no filter was chosen anywhere. */
#define TRC_PLANES_BBATCH_MAGIC 0x45435254u   /* "TRCE" */
typedef struct trc_planes_bbatch_hdr {
    uint32_t magic;      /* TRC_PLANES_BBATCH_MAGIC */
    uint8_t  version;    /* 1 */
    uint8_t  zero;
    uint16_t zero2;
    uint64_t count;      /* items: that of the TRCB container behind the fingerprints */
} trc_planes_bbatch_hdr; /* 16 bytes, little endian */
size_t trc_base_fingerprint_batch_table_bytes(size_t item_count);
int    trc_base_fingerprint_batch_dev(const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                      size_t first_item, size_t item_count, uint64_t *d_fp,
                                      void *d_table, size_t table_bytes, void *stream);
size_t trc_planes_bbatch_bound(int codec, const trc_planes_item *items, size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum);
int    trc_planes_bbatch_check(const void *buf, size_t buflen, size_t count_expected);
int    trc_planes_bbatch_info(const void *buf, size_t buflen, trc_planes_batch_hdr *h, uint64_t *n, uint8_t *filters, uint64_t *base_fp, size_t cap);
int trc_planes_bbatch_pack_dev(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                               unsigned esize, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum,
                               const int32_t *d_status, const uint32_t *d_clen, const void *d_payload,
                               const uint64_t *d_total, void *d_out, size_t out_bytes, uint64_t *d_size,
                               void *d_table, size_t table_bytes, void *stream);
int trc_decode_bplanes_batch_packed_dev(int codec, const void *d_cont, size_t cont_bytes,
                                        const trc_planes_item *items, const void *const *bases, const uint8_t *filters, size_t count,
                                        size_t first_item, size_t item_count, unsigned esize, uint32_t chunk, unsigned cdfnum,
                                        const uint64_t *total /* host, esize entries */, void *d_work, size_t work_bytes, void *stream);
size_t trc_encode_bplanes_batch_host(int codec, const trc_planes_item *items, const void *const *bases, const uint8_t *filters,
                                     size_t count, unsigned esize, uint32_t chunk, unsigned cdfnum, int items_on,
                                     void *out, size_t outcap);
size_t trc_encode_abplanes_batch_host(int codec, const trc_planes_item *items, const void *const *bases, size_t count, unsigned esize,
                                      uint32_t chunk, unsigned cdfnum, int items_on, void *out, size_t outcap,
                                      uint8_t *filters_out /* may be NULL */);
size_t trc_decode_bplanes_batch_host(const void *in, size_t inlen, const trc_planes_item *items, const void *const *bases, size_t count,
                                     size_t first_item, size_t item_count, int items_on);
int trc_planes_hist_bbatch_dev(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t count,
                               size_t first_item, size_t item_count, unsigned esize, uint32_t chunk,
                               uint64_t *d_hist, void *d_table, size_t table_bytes, void *stream);
int trc_planes_advise_bbatch(const uint64_t *hist, unsigned filters, unsigned esize, const trc_planes_item *items,
                             const void *const *bases, size_t count, uint8_t *filters_out, trc_planes_advice *advice /* may be NULL */);
int trc_planes_advise_bbatch_dev(unsigned filters, const trc_planes_item *items, const void *const *bases, size_t count, unsigned esize,
                                 uint32_t chunk, uint8_t *filters_out, trc_planes_advice *advice,
                                 void *d_work, size_t work_bytes, void *stream);
int trc_base_verify_batch_dev(const void *d_cont, const trc_planes_item *items, const void *const *bases, const uint8_t *filters,
                              size_t count, size_t first_item, size_t item_count, int64_t *d_bad,
                              void *d_table, size_t table_bytes, void *stream);

/* Optional timing of the coder kernels: every coder launch of a call carries a HIP event pair (hipExtLaunchKernel
 * start/stop events on the caller's stream), so the durations are the kernels' own -- BOTH passes of the two-pass
 * rANS encoders and the order-1 model fill included (the directory/gather kernels are not coder kernels).
 * enable(1) resets the counters; read() waits for the recorded events and returns the summed duration and the
 * number of encode (decode) CALLS measured: total_ms / launches = coder-kernel time of one call (at most 4096
 * kernel launches per direction between two enable() calls).  `decode` = 2 reads the third class: the encode path's own
 * directory work (group scan on large inputs, payload gather), so that (N + C) / (coder + gather) is a measured quantity.
 * Thread-safe. */
int trc_timing_enable(int on);
int trc_timing_pause(int paused);   /* suspend (1) / resume (0) the event pairs without resetting what was collected: time a SAMPLE of the calls */
int trc_timing_read(int decode, double *total_ms, int *launches);

/* name of the dominant kernel the last encode/decode of `codec` launched (for rocprof lookups) */
const char *trc_kernel_name(int codec, int decode);

#ifdef __cplusplus
}
#endif
#endif
