// trc_launch.h -- host-side launch entry points of the kernel translation units (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

// Optional timing of the coder kernels of a call: while the API layer has timing armed for the calling thread, every
// coder launch of the call (both passes of the two-pass rANS encoders, the order-1 model fill) carries its own event
// pair (hipExtLaunchKernelGGL: timestamps of the dispatch itself, no extra barrier packets in the queue -- separate
// hipEventRecord calls around a launch cost ~6 us of queue time each); otherwise it is a plain launch.  `kern` goes in
// parentheses when it is a template instance.
bool trc_tm_next(hipEvent_t *start, hipEvent_t *stop);      // trc_api.hip: hands out the next pair, false = not timing
#define TRC_LAUNCH_TIMED(kern, grid, block, lds, stream, ...)                                                      \
    do {                                                                                                         \
        hipEvent_t tm_a_, tm_b_;                                                                                 \
        if (trc_tm_next(&tm_a_, &tm_b_)) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)(lds), stream, tm_a_, tm_b_, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                    \
    } while (0)

// Kernels that need more than 64 KiB of dynamic LDS raise their limit once per DEVICE (the attribute is per device:
// a process that moves to another GPU must set it there too).
bool trc_first_use_on_device(unsigned long long *mask);
#define TRC_RAISE_LDS_ONCE(kern, bytes)                                                                            \
    do {                                                                                                         \
        static unsigned long long seen_ = 0;                                                                     \
        if (trc_first_use_on_device(&seen_))                                                                     \
            (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
    } while (0)

// a dynamic-LDS request above half of a CU's 160 KiB: at most one such workgroup per CU (the large workgroups whose waves keep each
// other's pace, TrcPace: their waves are meant to be the only ones on their SIMDs)
#define TRC_LDS_ONE_PER_CU (82u * 1024u)
// the nibble coders (48-byte model rows: many waves per CU) take the large workgroup shape when the launch is one residency round of
// twelve waves per CU (TRC_NIB_WPG, trc_dev.h); TRC_NIB_BIG=0 / 1 forces the shape (tuning aid, tests)
static inline bool trc_nib_big(uint32_t ngroups)
{
    static const int env = getenv("TRC_NIB_BIG") ? atoi(getenv("TRC_NIB_BIG")) : -1;
    return env >= 0 ? env != 0 : (ngroups >= 2048u && ngroups <= 12u * 256u);
}

// The arrival gate of the NEXT encode launched by this thread (trc_io.h, WaveChunks::gate): set by the host layer around its
// trc_encode_dev call, read by the launchers of the encoders that honour it (trc_gate_ok), null otherwise.
struct TrcGate { const uint32_t *flag; uint32_t part; };
extern thread_local TrcGate trc_gate_tls;
struct TrcProg { uint32_t *counters; uint32_t *host_flags; uint32_t part; };  // ... and the progress counters of the next DECODE (WaveChunks::prog)
extern thread_local TrcProg trc_prog_tls;
bool trc_prog_ok(int codec);                                   // the decoder of `codec` reports its progress (trc_api.hip)
bool trc_gate_ok(int codec);                                   // the encoder of `codec` waits at the gate (trc_api.hip)

// Workspace carve-up shared by encode and decode (all offsets 256-byte aligned).
struct TrcWork {
    uint8_t  *tables;    // per-call coder tables derived from the CDF (static coders)
    uint32_t *gsum;      // per-group (64 chunks) payload bytes
    uint64_t *goff;      // exclusive prefix of gsum (ngroups+1 entries) when the scan kernel runs; NULL = kernels sum gsum themselves
    uint64_t *goff_area; // where that prefix lives in the workspace, always.  Round 4: the gather of an encode leaves every group's base
                         // there (it has just computed it), and a decode of that very directory (TRC_DIR_READY) reads it instead of
                         // having each of its waves add up the group sums below its own
    uint8_t  *scratch;   // encode only: per-chunk private output regions
    uint32_t  stride;    // bytes per scratch region
    uint8_t  *scratch2;  // second region array (RCS2: stream 1)
    uint32_t  stride2;
    uint32_t  nchunks, ngroups;
    uint8_t  *model;     // models in HBM (TrcCodec::model_area): ANSO1, RCC1, RCX1 one order-1 model per chunk (136 / 136 / 64 KiB); trees
                         // of the 32-bit Rice, Turbo-VLC context and word coders
    uint32_t *aux;       // Turbo-VLC coders: two u32 per chunk (length of the first payload piece; mantissa bits)
    uint32_t  ss_prm;    // "ss" predictor coders: the call's two shift parameters, prm0 | prm1 << 8 (TRC_SS_PRM), else 0
};
#define TRC_O1_MODEL_BYTES (256u * 17u * 32u)

// table area layout (bytes from TrcWork::tables)
#define TRC_TAB_ENC   0          // uint4[256]   encoder symbol table
#define TRC_TAB_DEC   4096       // u32[256]     decoder symbol table
#define TRC_TAB_LUT   8192       // u8[32768]    slot -> symbol
#define TRC_TAB_CDF   40960      // u16[260]     sanitised CDF copy
#define TRC_TAB_BYTES 45056      // (the bytes from 41984 are unused; the size callers see stays)

// static-table prep (ANS4S / RCS1 / RCS2)
void trc_launch_static_prep(const uint16_t *d_cdf, unsigned cdfnum, uint8_t *tables, hipStream_t s);

// How the payload gather finds a chunk's payload in the scratch (one value per coder: TrcCodec::gather).  Raw chunks (clen ==
// chunk length) are copied from the input instead.
enum TrcGather {
    TRC_GATHER_START = 0,      // at the START of the chunk's scratch region
    TRC_GATHER_END = 1,        // at the END of it
    TRC_GATHER_TWO = 2,        // [4 + len0 bytes at the start of region A][rest at the start of region B] (two streams), len0 = u32 at region A
    TRC_GATHER_AUX = 3,        // [la bytes at the start of the region][rest at its END], la = aux[2c] (Turbo-VLC)
    TRC_GATHER_VLA = 4,        // [la bytes at the END of region A][rest at the END of region B] (Turbo-VLC over rANS)
};

// directory scan + payload gather
void trc_launch_group_sums(const uint32_t *d_clen, uint32_t nchunks, size_t n, uint32_t chunk, uint32_t *gsum, hipStream_t s);
void trc_launch_scan_groups(const uint32_t *gsum, uint32_t ngroups, uint64_t *goff, uint64_t *d_total, hipStream_t s);
// the directory of chunks [first, first + count): goff_sub[0 .. ceil(count / 64)] and gsum_sub[] from the full directory's goff
void trc_launch_range_dir(const uint32_t *d_clen, uint32_t nchunks, size_t n, uint32_t chunk, const uint64_t *goff_full,
                          uint32_t first, uint32_t count, uint32_t *gsum_sub, uint64_t *goff_sub, hipStream_t s);
void trc_launch_gather(const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, TrcGather mode,
                       const uint32_t *d_clen, uint8_t *d_payload, uint64_t *d_total, hipStream_t s);

// Every coder family has one encode and one decode launcher of these two shapes; the coder's row (trc_api.hip) names them and
// carries the family's own parameters, which the launcher reads from it.
struct TrcCodec;
typedef void TrcEncFn(const TrcCodec &c, const uint8_t *d_in, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s);
typedef void TrcDecFn(const TrcCodec &c, const uint8_t *d_payload, const uint32_t *d_clen, size_t n, uint32_t chunk,
                      const TrcWork &w, uint8_t *d_out, hipStream_t s);

// One row per coder id: how it is launched, and every per-coder decision of the API and the host layer.
struct TrcCodec {
    int id;
    TrcEncFn *enc;             // null: the id is not assigned
    TrcDecFn *dec;
    // the family's parameters
    int8_t k;                  // index within the family (integer, Turbo-VLC bitwise, word, nibble / varint coders); the order-1 bitwise context (0 rccs, 1 rcxs)
    int8_t streams;            // static / adaptive / vnibble range coders: 1 or 2 streams; -1: rccdfsm
    int8_t nibble;             // adaptive coders on values 0..15
    bool low4;                 // codes in[i] & 15 and decodes to it, never stores raw (the seven `turborc -n` coders): the byte-plane calls refuse it
    int8_t variant;            // Turbo-VLC: 0 u, 1 v, 2 vz (over rANS: 0 u, 1 v)
    int8_t zz;                 // Turbo-VLC over rANS: zigzag-delta form
    int8_t elem;               // Turbo-VLC: element bytes (2 or 4)
    TrcGather gather;
    bool cdf;                  // static coder: needs a CDF, derives its tables from it
    bool ss;                   // "ss" predictor coder: no CDF, `cdfnum` carries the two shift parameters (TRC_SS_PRM)
    bool aux;                  // two u32 per chunk in the workspace (TrcWork::aux)
    bool gate;                 // the encoder waits at the arrival gate (WaveChunks::gate)
    bool prog;                 // the decoder reports its progress (WaveChunks::prog)
    uint16_t wave_ns;          // one wave's time per byte of its chunk, ns, the slower of encode and decode
    uint32_t round_lanes;      // chunks coded at once in one residency round of the chip
    uint32_t auto_max;         // the largest chunk trc_auto_chunk_codec picks
    uint32_t floor;            // the smallest chunk the automatic rules and the host-pointer calls use (0: TRC_CHUNK_AUTO_MIN for the
                               // automatic ones, none for the host calls); trc_round_chunk takes exactly this one
    uint32_t chunk_max;        // the largest chunk the kernels take
    uint16_t pad;              // scratch bytes per chunk beyond its length
    uint8_t s2_mul;            // second scratch array: s2_mul x chunk + s2_add bytes per chunk ...
    uint16_t s2_add;
    bool s2_lanes;             // ... per LANE, dead lanes of the last wave included (rows of 64)
    size_t (*model_area)(const TrcCodec &c, size_t nchunks);   // bytes of TrcWork::model (null: none)
    size_t (*slice_model)(const TrcCodec &c);                   // model bytes per chunk that cap a host-pointer call's slices (null: no cap)
    const char *kernel_enc, *kernel_dec;                         // the dominant kernels (trc_kernel_name)
};

// ANS4S: static-CDF rANS (anscdf4senc / anscdf4sdec)
TrcEncFn trc_launch_ans4s_enc;  TrcDecFn trc_launch_ans4s_dec;
// RCS1 / RCS2: static-CDF range coder, 1 or 2 streams (rccdfsenc / rccdfs2enc and their decoders);
// streams == -1: RCSM, one stream with the 32-bit range / 16-bit I/O geometry (rccdfsmenc / rccdfsm*dec)
TrcEncFn trc_launch_rcs_enc;    TrcDecFn trc_launch_rcs_dec;
// RCB: bitwise order-0 range coder (rcsenc / rcsdec)
TrcEncFn trc_launch_rcb_enc;    TrcDecFn trc_launch_rcb_dec;
// RCC1 / RCX1: bitwise order-1 range coders (rccsenc / rccsdec: k = 0; rcxsenc / rcxsdec: k = 1), models in w.model
TrcEncFn trc_launch_o1bit_enc;  TrcDecFn trc_launch_o1bit_dec;
// RCG8 .. RCRZ32: gamma / Rice integer coders (k = codec - TRC_RCG8); models in LDS, the 32-bit Rice ones in w.model
TrcEncFn trc_launch_int_enc;    TrcDecFn trc_launch_int_dec;
size_t trc_int_model_bytes(int k, size_t ngroups);   // workspace bytes of w.model for ngroups waves (0: the model is in LDS)
// RCBV16 .. RCBVGZ32: Turbo-VLC coders on the bitwise range coder (k = codec - TRC_RCBV16); aux[2c] = length of the
// range-coder piece (TRC_GATHER_AUX); the context-model coders (k = 0, 2, 3) keep 256 trees per chunk in w.model
TrcEncFn trc_launch_bvlc_enc;   TrcDecFn trc_launch_bvlc_dec;
size_t trc_bvlc_model_bytes(int k, size_t nchunks);   // workspace bytes of w.model for nchunks chunks (0: the model is in LDS)
// RCW16 .. RCC2W32: bitwise word coders (k = codec - TRC_RCW16); w.model holds trc_word_slots(k, nchunks) models of
// trc_word_model_bytes(k), used by the chunks in rounds
TrcEncFn trc_launch_word_enc;   TrcDecFn trc_launch_word_dec;
size_t trc_word_model_bytes(int k);
size_t trc_word_slots(int k, size_t nchunks);
// RC4 / RC4C / RCU3: bitwise nibble and varint byte coders (k = codec - TRC_RC4: rc4s, rc4cs, rcu3s); models in LDS, none for rc4cs
TrcEncFn trc_launch_nibbit_enc; TrcDecFn trc_launch_nibbit_dec;
// RC4SS / RC4CSS / RCU3SS / RCSS: the byte-level bitwise coders on the dual-rate "ss" predictor (k = 0 rc4ss, 1 rc4css, 2 rcu3ss,
// 3 rcss); models in LDS, none for rc4css; the two shift parameters in w.ss_prm
TrcEncFn trc_launch_ssbit_enc;  TrcDecFn trc_launch_ssbit_dec;
void trc_o1bit_fill(uint8_t *model, size_t bytes, hipStream_t s);   // set `bytes` (a multiple of 16) of tree nodes to 0x4000
// RCA / RCAI: adaptive-CDF byte range coder, 1 stream (rccdfenc / rccdfdec) or hi/lo nibbles on 2 streams (rccdfienc / rccdfidec);
// nibble != 0: the `turborc -n` coders on values 0..15 (rccdf4enc/dec, rccdf4ienc/idec)
TrcEncFn trc_launch_rca_enc;    TrcDecFn trc_launch_rca_dec;
// RCV8 / RCVI8: "vnibble" adaptive-CDF range coders, 1 or 2 streams (rccdfenc8 / rccdfienc8 and their decoders)
TrcEncFn trc_launch_rcv_enc;    TrcDecFn trc_launch_rcv_dec;
// ANSA: adaptive-CDF byte rANS (anscdfenc / anscdfdec); scratch2 holds the 8 B/byte record stack
// nibble != 0: anscdf4enc / anscdf4dec on values 0..15 (2 states, 4 B/byte record stack)
TrcEncFn trc_launch_ansa_enc;   TrcDecFn trc_launch_ansa_dec;
void trc_launch_ansa_code(int nibble, size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s);   // pass 2 alone
void trc_launch_ansa_code_planar(size_t n, uint32_t chunk, const TrcWork &w, uint32_t *d_clen, hipStream_t s);   // pass 2 over the planar record space (four lanes per chunk)
// ANSO1: order-1 adaptive-CDF byte rANS (anscdf1enc / anscdf1dec): pass 1 with the models in HBM (w.model), then pass 2 of ANSA
// (plain or planar); scratch2 holds the same 8 B/byte record stack as ANSA
TrcEncFn trc_launch_anso1_enc;  TrcDecFn trc_launch_anso1_dec;
// ANSB: bitwise order-0 rANS (ansbc / ansbd); chunks of at most 8192 bytes (one reference block); scratch2 holds the
// 16 B/byte record stack
TrcEncFn trc_launch_ansb_enc;   TrcDecFn trc_launch_ansb_dec;
// Turbo-VLC integer coders (rccdf{u,v,vz}{enc,dec}{16,32}): variant 0 = u, 1 = v, 2 = vz; elem = 2 or 4 bytes;
// aux[2c] = length of the range-coder piece (TRC_GATHER_AUX)
TrcEncFn trc_launch_vlc_enc;    TrcDecFn trc_launch_vlc_dec;
// ... over the adaptive CDF rANS (anscdf{u,uz,v,vz}{enc,dec}{16,32}): variant 0 = u, 1 = v; zz = zigzag-delta form;
// scratch2 holds, per chunk, the record stack (8 B per element) and, at the end of the slot, the mantissa bytes
TrcEncFn trc_launch_vla_enc;    TrcDecFn trc_launch_vla_dec;

// cdfini on device
void trc_launch_hist(const uint8_t *d_in, size_t n, uint64_t *d_hist, hipStream_t s);
void trc_launch_cdf_build(const uint64_t *d_hist, size_t n_total, uint16_t *d_cdf, unsigned cdfnum, int32_t *d_status, hipStream_t s);
void trc_launch_cdfini(const uint8_t *d_in, size_t n, uint16_t *d_cdf, unsigned cdfnum,
                       int32_t *d_status, uint64_t *d_hist /*256 u64*/, hipStream_t s);
