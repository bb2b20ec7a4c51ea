// trc_api.hip -- the C-ABI of libturborc_hip.so (include/trc_hip.h, include/anscdf.h, include/turborc.h).
//
// Layer 2 (*_dev): enqueue-only, caller-owned device buffers and stream.
// Layer 1 (reference prototypes): host pointers; stage through a process-wide device context,
// run layer 2, wrap the result in the TRC1 container.  There is NO CPU coding path in this
// library: if HIP is unavailable every call fails loudly (stderr + trc_last_error, return 0).
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/trc_hip.h"
#include "trc_launch.h"

typedef unsigned short cdf_t;
static const unsigned TRC_PROB_ONE_HOST = 32768u;

// ------------------------------------------------------------------------------------ errors ---
static thread_local char g_err[512];
static int fail(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    fprintf(stderr, "turborc_hip: ERROR: %s\n", g_err);
    return code;
}
// the same for the other translation units of the library (trc_rccl.hip)
int trc_fail(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    fprintf(stderr, "turborc_hip: ERROR: %s\n", g_err);
    return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(TRC_E_HIP, "%s -> %s", #x, hipGetErrorString(e_)); } while (0)

extern "C" const char *trc_last_error(void) { return g_err; }

extern "C" int trc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------ coders ---
// One row per assigned coder id: its launchers and the family's parameters, and every per-coder decision below (workspace,
// chunk rules, gather, host-pointer calls).  A new coder is a new row; ids without a row are rejected everywhere.
//
// wave_ns: one wave's time per byte of its chunk, ns, the slower of encode and decode.  Byte coders: profiles/r05_all_codecs.txt,
// kernel time at chunk 4096 with the chip a third full / 4096.  Order-1 bitwise coders: one lane per chunk, models in HBM, chunk
// 16384, markov (profiles/o1bit_notes.md).  Integer coders: one lane per chunk, 100 MB with the chip less than one round full,
// rcgs / rcrs at chunk 16384, the zigzag coders at 4096 (profiles/intbit/intbit_notes.md).  Turbo-VLC on the bitwise coder: 100 MB,
// about one round, the context coders at chunk 16384, the others at 1536 (profiles/bvlc/bvlc_bench.jsonl).  Word coders: trees in
// HBM, 100 MB of `walk` at chunk 16384 (profiles/word/word_notes.md).
//
// round_lanes: chunks per residency round of the chip (trc_round_chunk).  Static coders 12 waves per CU (196 608 chunks; the
// two-lanes-per-chunk `-e45` coder 98 304), a model per lane in LDS 4 waves per CU (256 CUs x 4 waves x 64 lanes = 65 536), the
// small-model coders (nibble, vnibble, Turbo-VLC) ~20 (327 680).  Integer coders: the 8-bit models (9-13 KiB of LDS per wave)
// leave room for more resident lanes than the 16/32-bit ones (100 MB: chunk 1024 against 1536, rcgs8 1.9 against 2.6 ms --
// profiles/intbit/intbit_notes.md).  Turbo-VLC on the bitwise coder (9 / 34 KiB of LDS per wave): 100 MB in one round at 1536 is
// the sweep's best for every coder not held at the floor (profiles/bvlc/bvlc_bench.jsonl).
//
// floor: the order-1 rANS never goes below 4096; the bitwise order-1 coders stay at TRC_O1BIT_CHUNK_MIN, the ratio floor
// (DESIGN.md): every larger chunk only waits longer -- and so do the Turbo-VLC coders with 256 trees per chunk (their workspace
// is 4.5 / 8.5 bytes per input byte at 16384, four times that at 4096, for 0.4 points of ratio: profiles/bvlc/bvlc_notes.md) and
// the word coders (one lane per chunk, trees in HBM).
//
// pad: payload + one period of look-ahead, moved in whole 64-B segments (trc_io.h); the integer coders add up to 107 coded bits
// (~134 B) with one element after the last raw test, the bitwise Turbo-VLC ones ~7 words and 4 mantissa bytes, the word coders
// 16 words (rcs16 stops once its output reaches the chunk).
//
// second scratch array: the second stream (same stride as the first, look-ahead included), the adaptive rANS record stacks (8 B per
// byte, the nibble form 4, the bitwise rANS 16), the bitwise encoder's deepest tree level (128 nodes x u16 per chunk,
// trc_rc_bit.hip; its rows are indexed by LANE), and for Turbo-VLC over rANS the record stack (8 B per element) with room for the
// mantissa bytes at the slot's end: 8 x chunk / elem + chunk + 64 (exact: a chunk is a multiple of 64).
#define TRC_MODEL_ROUND_CHUNKS 65536u
#define TRC_AUTO_CHUNK_MAX 16384u
// models in the workspace (w.model): an order-1 model per chunk of the call (anscdf1 and rccs 136 KiB, rcxs 64 KiB), the integer
// coders' per-wave blocks (trc_rc_int.hip), the Turbo-VLC context coders' 256 trees per chunk (trc_rc_bvlc.hip), the word coders'
// slots that the chunks use in rounds (trc_rc_word.hip), at most TRC_WORD_MODEL_BUDGET bytes
static size_t o1_model(const TrcCodec &) { return TRC_O1_MODEL_BYTES; }
static size_t o1x_model(const TrcCodec &) { return 512u * 64u * 2u; }
static size_t per_chunk_area(const TrcCodec &c, size_t nchunks) { return nchunks * c.slice_model(c); }
static size_t int_area(const TrcCodec &c, size_t nchunks) { return trc_int_model_bytes(c.k, (nchunks + 63) / 64); }
static size_t bvlc_area(const TrcCodec &c, size_t nchunks) { return trc_bvlc_model_bytes(c.k, nchunks); }
static size_t word_model(const TrcCodec &c) { return trc_word_model_bytes(c.k); }
static size_t word_area(const TrcCodec &c, size_t nchunks) { return trc_word_slots(c.k, nchunks) * trc_word_model_bytes(c.k); }

#define LAUNCH(f) .enc = trc_launch_##f##_enc, .dec = trc_launch_##f##_dec
#define KERNELS(e, d) .kernel_enc = e, .kernel_dec = d
#define STATIC(i, f, st, g, ns, lanes, s2mul, s2add, ke, kd) \
    { .id = i, LAUNCH(f), .streams = st, .gather = g, .cdf = true, .wave_ns = ns, .round_lanes = lanes, .auto_max = 4096u, \
      .chunk_max = TRC_CHUNK_MAX, .pad = 128, .s2_mul = s2mul, .s2_add = s2add, KERNELS(ke, kd) }
#define ADAPTIVE(i, f, st, nib, g, stream, ns, lanes, s2mul, s2add, ke, kd) \
    { .id = i, LAUNCH(f), .streams = st, .nibble = nib, .low4 = nib != 0, .gather = g, .gate = stream, .prog = stream, .wave_ns = ns, .round_lanes = lanes, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, .s2_mul = s2mul, .s2_add = s2add, KERNELS(ke, kd) }
#define VLC(i, ns) \
    { .id = i, LAUNCH(vlc), .variant = (i - TRC_VLCU16) >> 1, .elem = ((i - TRC_VLCU16) & 1) ? 4 : 2, .gather = TRC_GATHER_AUX, .aux = true, \
      .wave_ns = ns, .round_lanes = 327680u, .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, \
      KERNELS("trc_vlc_enc_kernel", "trc_vlc_dec_kernel") }
#define VLA(i, var, z, el, ns) \
    { .id = i, LAUNCH(vla), .variant = var, .zz = z, .elem = el, .gather = TRC_GATHER_VLA, .aux = true, .wave_ns = ns, .round_lanes = 327680u, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, .s2_mul = 8 / el + 1, .s2_add = 64, \
      KERNELS("trc_vla_model_kernel", "trc_vla_dec_kernel") }
#define O1BIT(i, ctx, ns, model) \
    { .id = i, LAUNCH(o1bit), .k = ctx, .gather = TRC_GATHER_START, .wave_ns = ns, .round_lanes = 327680u, .auto_max = TRC_AUTO_CHUNK_MAX, \
      .floor = TRC_O1BIT_CHUNK_MIN, .chunk_max = TRC_CHUNK_MAX, .pad = 128, .model_area = per_chunk_area, .slice_model = model, \
      KERNELS("trc_rc_o1bit_enc_kernel", "trc_rc_o1bit_dec_kernel") }
#define INT(i, ns) \
    { .id = i, LAUNCH(int), .k = i - TRC_RCG8, .gather = TRC_GATHER_START, .wave_ns = ns, \
      .round_lanes = (i - TRC_RCG8) % 3 == 0 ? 98304u : TRC_MODEL_ROUND_CHUNKS, .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, \
      .pad = 256, .model_area = int_area, KERNELS("trc_rc_int_enc_kernel", "trc_rc_int_dec_kernel") }
// (the context coders keep 256 trees per chunk in w.model, but have no slice_model: a host-pointer call does not cap their slices)
#define BVLC(i, ctx, ns) \
    { .id = i, LAUNCH(bvlc), .k = i - TRC_RCBV16, .gather = TRC_GATHER_AUX, .aux = true, .wave_ns = ns, .round_lanes = TRC_MODEL_ROUND_CHUNKS, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .floor = ctx ? TRC_O1BIT_CHUNK_MIN : 0u, .chunk_max = TRC_CHUNK_MAX, .pad = 256, .model_area = bvlc_area, \
      KERNELS("trc_rc_bvlc_enc_kernel", "trc_rc_bvlc_dec_kernel") }
#define WORD(i, ns) \
    { .id = i, LAUNCH(word), .k = i - TRC_RCW16, .gather = TRC_GATHER_START, .wave_ns = ns, .round_lanes = 327680u, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .floor = TRC_O1BIT_CHUNK_MIN, .chunk_max = TRC_CHUNK_MAX, .pad = 256, .model_area = word_area, \
      .slice_model = word_model, KERNELS("trc_rc_word_enc_kernel", "trc_rc_word_dec_kernel") }
// one lane per chunk, the whole model in LDS (rc4s 2 KiB per wave, rcu3s 37.4 KiB, rc4cs none): no floor, any chunk from 256 up.
// wave_ns from the chunk-16384 runs of the 100 MB sweep in profiles/nibbit/nibbit_notes.md (chip a tenth full); round_lanes from
// the sweep's best chunk: rc4s 512 (256 is no faster), rc4cs 1024, rcu3s 1536 (four waves per CU, as its LDS allows)
#define NIBBIT(i, ns, lanes) \
    { .id = i, LAUNCH(nibbit), .k = i - TRC_RC4, .low4 = i - TRC_RC4 < 2, .gather = TRC_GATHER_START, .wave_ns = ns, .round_lanes = lanes, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, KERNELS("trc_rc_nib_enc_kernel", "trc_rc_nib_dec_kernel") }
// the same shape on the dual-rate "ss" predictor (trc_rc_ss.hip: rc4ss 4 KiB of LDS per wave, rcss 64 KiB, rcu3ss 74.75 KiB, rc4css
// none); the call's two shift parameters travel in `cdfnum` (TRC_SS_PRM).  wave_ns and round_lanes are those of the "s" counterparts (rcs, rc4s, rc4cs, rcu3s) until the sweep of
// profiles/ssbit/ssbit_notes.md has been run: not measured
#define SSBIT(i, kk, ns, lanes) \
    { .id = i, LAUNCH(ssbit), .k = kk, .low4 = kk < 2, .gather = TRC_GATHER_START, .ss = true, .wave_ns = ns, .round_lanes = lanes, \
      .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, KERNELS("trc_rc_ss_enc_kernel", "trc_rc_ss_dec_kernel") }
// what an id without a coder answers to trc_auto_chunk_codec / trc_round_chunk
#define NONE(i) { .id = i, .wave_ns = 400, .round_lanes = 327680u, .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, KERNELS("", "") }

static constexpr TrcCodec g_codecs[] = {
    NONE(0),
    STATIC(TRC_ANS4S, ans4s, 0, TRC_GATHER_END, 67, 196608u, 0, 0, "trc_ans4s_enc_kernel", "trc_ans4s_dec_kernel"),
    STATIC(TRC_RCS1, rcs, 1, TRC_GATHER_START, 184, 196608u, 0, 0, "trc_rcs_enc_kernel", "trc_rcs_dec_kernel"),
    STATIC(TRC_RCS2, rcs, 2, TRC_GATHER_TWO, 112, 98304u, 1, 128, "trc_rcs2p_enc_kernel", "trc_rcs2p_dec_kernel"),
    ADAPTIVE(TRC_RCA, rca, 1, 0, TRC_GATHER_START, true, 406, TRC_MODEL_ROUND_CHUNKS, 0, 0, "trc_rca_enc_mc_kernel", "trc_rca_dec_kernel"),
    ADAPTIVE(TRC_ANSA, ansa, 0, 0, TRC_GATHER_END, true, 336, TRC_MODEL_ROUND_CHUNKS, 8, 0, "trc_ansa_model2_kernel", "trc_ansa_dec_kernel"),
    { .id = TRC_RCB, LAUNCH(rcb), .gather = TRC_GATHER_START, .gate = true, .prog = true, .wave_ns = 592, .round_lanes = TRC_MODEL_ROUND_CHUNKS,
      .auto_max = TRC_AUTO_CHUNK_MAX, .chunk_max = TRC_CHUNK_MAX, .pad = 128, .s2_mul = 0, .s2_add = 256, .s2_lanes = true,
      KERNELS("trc_rcb_enc_mc_kernel", "trc_rcb_dec_kernel") },
    ADAPTIVE(TRC_RCAI, rca, 2, 0, TRC_GATHER_TWO, true, 397, TRC_MODEL_ROUND_CHUNKS, 1, 128, "trc_rca_enc_mc_kernel", "trc_rca_dec_kernel"),
    ADAPTIVE(TRC_RCA4, rca, 1, 1, TRC_GATHER_START, false, 245, 327680u, 0, 0, "trc_rca_enc_kernel", "trc_rca_dec_kernel"),
    ADAPTIVE(TRC_RCAI4, rca, 2, 1, TRC_GATHER_TWO, false, 260, 327680u, 1, 128, "trc_rca_enc_kernel", "trc_rca_dec_kernel"),
    ADAPTIVE(TRC_ANSA4, ansa, 0, 1, TRC_GATHER_END, false, 255, 327680u, 4, 0, "trc_ansa_model_kernel", "trc_ansa_dec_kernel"),
    STATIC(TRC_RCSM, rcs, -1, TRC_GATHER_START, 230, 196608u, 0, 0, "trc_rcs_enc_kernel", "trc_rcs_dec_kernel"),
    { .id = TRC_ANSO1, LAUNCH(anso1), .gather = TRC_GATHER_END, .wave_ns = 884, .round_lanes = 327680u, .auto_max = TRC_AUTO_CHUNK_MAX,
      .floor = 4096u, .chunk_max = TRC_CHUNK_MAX, .pad = 128, .s2_mul = 8, .s2_add = 0, .model_area = per_chunk_area, .slice_model = o1_model,
      KERNELS("trc_o1_sort_kernel", "trc_o1_dec_rowsn_kernel") },
    { .id = TRC_ANSB, LAUNCH(ansb), .gather = TRC_GATHER_END, .wave_ns = 635, .round_lanes = TRC_MODEL_ROUND_CHUNKS, .auto_max = TRC_ANSB_CHUNK_MAX,
      .chunk_max = TRC_ANSB_CHUNK_MAX, .pad = 128, .s2_mul = 16, .s2_add = 0, KERNELS("trc_ansb_model_kernel", "trc_ansb_dec_kernel") },
    VLC(TRC_VLCU16, 391), VLC(TRC_VLCU32, 214), VLC(TRC_VLCV16, 391), VLC(TRC_VLCV32, 214), VLC(TRC_VLCVZ16, 391), VLC(TRC_VLCVZ32, 214),
    VLA(TRC_VLAU16, 0, 0, 2, 370), VLA(TRC_VLAUZ16, 0, 1, 2, 260), VLA(TRC_VLAV16, 1, 0, 2, 370), VLA(TRC_VLAVZ16, 1, 1, 2, 370),
    VLA(TRC_VLAV32, 1, 0, 4, 201), VLA(TRC_VLAVZ32, 1, 1, 4, 201),
    ADAPTIVE(TRC_RCV8, rcv, 1, 0, TRC_GATHER_START, false, 746, 327680u, 0, 0, "trc_rcv_enc_kernel", "trc_rcv_dec_kernel"),
    ADAPTIVE(TRC_RCVI8, rcv, 2, 0, TRC_GATHER_TWO, false, 797, 327680u, 1, 128, "trc_rcv_enc_kernel", "trc_rcv_dec_kernel"),
    O1BIT(TRC_RCC1, 0, 2830, o1_model), O1BIT(TRC_RCX1, 1, 3310, o1x_model),
    INT(TRC_RCG8, 1580), INT(TRC_RCG16, 1490), INT(TRC_RCG32, 1160), INT(TRC_RCGZ8, 1980), INT(TRC_RCGZ16, 650), INT(TRC_RCGZ32, 310),
    INT(TRC_RCR8, 2690), INT(TRC_RCR16, 1810), INT(TRC_RCR32, 3110), INT(TRC_RCRZ8, 1850), INT(TRC_RCRZ16, 640), INT(TRC_RCRZ32, 770),
    NONE(42),
    BVLC(TRC_RCBV16, 1, 884), BVLC(TRC_RCBV32, 0, 392), BVLC(TRC_RCBVZ16, 1, 831), BVLC(TRC_RCBVZ32, 1, 461),
    BVLC(TRC_RCBVG16, 0, 1352), BVLC(TRC_RCBVG32, 0, 728), BVLC(TRC_RCBVGZ16, 0, 1383), BVLC(TRC_RCBVGZ32, 0, 781),
    NONE(51),
    WORD(TRC_RCW16, 1340), WORD(TRC_RCW32, 1430), WORD(TRC_RCCW32, 1460), WORD(TRC_RCC2W32, 1440),
    NONE(56), NONE(57),
    NIBBIT(TRC_RC4, 570, 196608u), NIBBIT(TRC_RC4C, 320, 98304u), NIBBIT(TRC_RCU3, 1500, TRC_MODEL_ROUND_CHUNKS),
    NONE(61),
    SSBIT(TRC_RCSS, 3, 592, TRC_MODEL_ROUND_CHUNKS), SSBIT(TRC_RC4SS, 0, 570, 196608u), SSBIT(TRC_RC4CSS, 1, 320, 98304u),
    SSBIT(TRC_RCU3SS, 2, 1500, TRC_MODEL_ROUND_CHUNKS),
};
#undef LAUNCH
#undef KERNELS
#undef STATIC
#undef ADAPTIVE
#undef VLC
#undef VLA
#undef O1BIT
#undef INT
#undef BVLC
#undef WORD
#undef NIBBIT
#undef SSBIT
#undef NONE
static constexpr int TRC_NCODECS = (int)(sizeof g_codecs / sizeof g_codecs[0]);
static constexpr bool rows_in_id_order()
{
    for (int i = 0; i < TRC_NCODECS; i++) if (g_codecs[i].id != i) return false;
    return true;
}
static_assert(rows_in_id_order(), "g_codecs[i] must be the row of id i");
// the row of an id; ids without a coder get a row without launchers
static const TrcCodec &codec_row(int codec) { return g_codecs[codec > 0 && codec < TRC_NCODECS ? codec : 0]; }
static bool codec_ok(int codec) { return codec_row(codec).enc != nullptr; }
// the two shift parameters of an "ss" coder as `cdfnum` carries them (TRC_SS_PRM): each in 1 .. 15, nothing above them
static bool ss_prm_ok(unsigned v) { return !(v & ~0x0f0fu) && (v & 0x0fu) && (v & 0x0f00u); }

// ------------------------------------------------------------------------------------ config ---
// The chunk is the parallel unit AND the price of the format: every chunk costs 8 bytes of coder state and 4 bytes of
// directory, and an adaptive model learns its statistics anew in every chunk (20 MB of `drift` through rccdfenc: 38.7 % stored
// at chunk 512, 30.6 % at 1536, 28.0 % at 4096, 26.9 % at 16 384; one whole-buffer call of the reference 26.7 %).
// Rounds 3-5 picked the chunk of a host-pointer call for the KERNELS (512 below 1 GB: the chip full of short waves) -- on a path
// whose pace is set by PCIe, not by the kernels (the policy optimised the one quantity the caller cannot see and
// gave away the one it can).  Round 6: unless the caller fixes the size (trc_set_chunk, TRC_CHUNK), a host-pointer call takes the
// LARGEST chunk whose one-wave time still hides behind the call's transfer time:
//     wave time(chunk) = wave_ns x chunk                    (a launch lasts one wave's time however few chunks it has, and the
//                                                           slices of a call are coded concurrently: trc_host.inc)
//     budget           = max(1.7 ms, 0.35 x n / 50 GB/s)    (a third of what the link needs for the call: the last slice to arrive
//                                                           still has a wave's time to go, so a call lasts link time + wave time;
//                                                           the floor is what 100 MB are given: rccdf at 4096, 28.0 % stored)
// from the ladder 512 .. 16 384, between the coder's floor and its auto_max: static coders stop at 4096 (text100m: 63.50 % of
// payload against 63.35 % whole-buffer -- nothing left to gain), the bitwise rANS at one reference block (8192).
// 100 MB: rccdf / rccdfi / anscdf 4096, rcs 2048, static 4096; 1 GB: rccdf / anscdf 16 384, rcs 8192.
static uint32_t g_chunk = 0;                                  // 0: not read yet;  ~0u: automatic
static bool chunk_ok(uint32_t c) { return c >= TRC_CHUNK_MIN && c <= TRC_CHUNK_MAX && (c % 64u) == 0; }
extern "C" uint32_t trc_auto_chunk_codec(int codec, size_t n)
{
    static const uint32_t ladder[] = { 16384u, 12288u, 8192u, 6144u, 4096u, 3072u, 2048u, 1536u, 1024u, 768u, 512u };
    const TrcCodec &r = codec_row(codec);
    const double link_ns = 0.35 * (double)n / 50.0;               // 50 GB/s = 50 bytes per ns
    const double budget_ns = link_ns > 1.7e6 ? link_ns : 1.7e6;
    const uint32_t lo = r.floor ? r.floor : TRC_CHUNK_AUTO_MIN;
    for (uint32_t c : ladder)
        if (c <= r.auto_max && (c <= lo || (double)r.wave_ns * c <= budget_ns)) return c;
    return lo;
}
extern "C" uint32_t trc_auto_chunk(size_t n) { return trc_auto_chunk_codec(TRC_ANS4S, n); }      // the static coders' rule
// The chunk for a DEVICE-RESIDENT call of n bytes (one launch over the whole input: trc_encode_dev, bench.py).  A launch lasts
// (residency rounds) x (one wave's time, proportional to its chunk), so the input should be a whole number of rounds of the
// coder's resident lanes (round_lanes), barely: the LARGEST chunk (multiple of 64) with ceil(n / chunk) <= k rounds for the
// smallest k that allows it.  100 MB: 512 / 1024 / 1536 / 512 as measured best in round 3 (profiles/r03_notes.md section 7: 1280
// instead of 1536 is a factor 1.9); 70 / 120 / 150 / 333 MB: tests/test_gpu_chunk_policy.py.
// Round 5: the cap is TRC_ROUND_CHUNK_MAX = 16 384 bytes, not 4096.  Rounds pack (profiles/r04_notes.md 1): k rounds of chunk c
// cost what ONE round of chunk k c costs -- and the larger chunk pays the model's learning phase and the coder's flush bytes k
// times less often.  1 GB of `rccdf` took four rounds of chunk 3840 (28.0 % stored; one whole-buffer call of the reference:
// 26.7 %); it now takes one round of chunk 15 296.  The kernels take chunks up to 65 536; above 16 KiB the
// ratio has nothing left to gain.  (The bitwise rANS stays within one reference block; a coder with a floor takes its floor:
// one lane per chunk, the launch's time is one chunk's.)
#define TRC_ROUND_CHUNK_MAX 16384u
extern "C" uint32_t trc_round_chunk(int codec, size_t n)
{
    const TrcCodec &r = codec_row(codec);
    if (r.floor) return r.floor;
    const size_t rc = r.round_lanes;
    const size_t cap = r.chunk_max < TRC_ROUND_CHUNK_MAX ? r.chunk_max : TRC_ROUND_CHUNK_MAX;
    for (size_t k = 1;; k++) {
        size_t c = (n + rc * k - 1) / (rc * k);               // ceil(n / c) <= rc * k
        c = (c + 63u) & ~(size_t)63u;
        if (c <= cap) return c < TRC_CHUNK_AUTO_MIN ? TRC_CHUNK_AUTO_MIN : (uint32_t)c;
    }
}
extern "C" uint32_t trc_get_chunk(void)
{
    if (!g_chunk) {
        const char *e = getenv("TRC_CHUNK");
        uint32_t c = e ? (uint32_t)strtoul(e, 0, 10) : 0;
        g_chunk = chunk_ok(c) ? c : ~0u;
    }
    return g_chunk == ~0u ? 0u : g_chunk;
}
extern "C" int trc_set_chunk(uint32_t chunk)
{
    if (chunk == 0) { g_chunk = ~0u; return TRC_OK; }         // back to automatic
    if (!chunk_ok(chunk)) return fail(TRC_E_ARG, "chunk %u: must be 0 (automatic) or a multiple of 64 in [%u,%u]", chunk, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    g_chunk = chunk;
    return TRC_OK;
}

// ------------------------------------------------------------------------------ workspace map ---
// up to this many groups every consumer wave sums the per-group byte counts itself (one scan kernel less
// per call); beyond it a single-workgroup scan kernel runs
#define TRC_INKERNEL_SCAN_MAX 8192u
static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// bytes of the second scratch array (rows per chunk or per lane) and of the coder's model area
static inline size_t scratch2_bytes(const TrcCodec &r, size_t nchunks, uint32_t chunk)
{
    const size_t rows = r.s2_lanes ? ((nchunks + 63) & ~(size_t)63) : nchunks;
    return up256(rows * ((size_t)r.s2_mul * chunk + r.s2_add) + 256);
}
static inline size_t model_area_bytes(const TrcCodec &r, size_t nchunks) { return r.model_area ? up256(r.model_area(r, nchunks)) : 0; }

extern "C" size_t trc_work_bytes(int codec, size_t n, uint32_t chunk)
{
    if (!codec) return 4096;           // cdfini: histogram bins
    const TrcCodec &r = codec_row(codec);
    if (!r.enc || !chunk_ok(chunk)) return 0;
    const size_t nchunks = (n + chunk - 1) / chunk, ngroups = (nchunks + 63) / 64;
    return up256(TRC_TAB_BYTES) + up256(4 * ngroups) + up256(8 * (ngroups + 1)) +
           up256(nchunks * ((size_t)chunk + r.pad)) + scratch2_bytes(r, nchunks, chunk) + model_area_bytes(r, nchunks) +
           (r.aux ? up256(nchunks * 8) : 0) + 4096;
}

static int carve(const TrcCodec &r, size_t n, uint32_t chunk, void *d_work, size_t work_bytes, TrcWork &w)
{
    const size_t need = trc_work_bytes(r.id, n, chunk);
    if (!need || work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    if (((uintptr_t)d_work) & 255) return fail(TRC_E_ARG, "workspace must be 256-byte aligned");
    const size_t nchunks = (n + chunk - 1) / chunk, ngroups = (nchunks + 63) / 64;
    uint8_t *p = (uint8_t *)d_work;
    w.tables = p;               p += up256(TRC_TAB_BYTES);
    w.gsum = (uint32_t *)p;     p += up256(4 * ngroups);
    static const uint32_t scan_max = getenv("TRC_SCAN_MAX") ? (uint32_t)atoi(getenv("TRC_SCAN_MAX")) : TRC_INKERNEL_SCAN_MAX;   // tuning aid
    w.goff_area = (uint64_t *)p;
    w.goff = ngroups > scan_max ? (uint64_t *)p : nullptr;     p += up256(8 * (ngroups + 1));
    w.scratch = p;
    w.stride = chunk + r.pad;
    w.stride2 = r.s2_mul * chunk + r.s2_add;
    w.scratch2 = p + up256(nchunks * (size_t)w.stride);
    w.model = w.scratch2 + scratch2_bytes(r, nchunks, chunk);
    w.aux = (uint32_t *)(w.model + model_area_bytes(r, nchunks));
    w.nchunks = (uint32_t)nchunks; w.ngroups = (uint32_t)ngroups;
    return TRC_OK;
}

static int check_common(int codec, size_t n, uint32_t chunk, const uint16_t *d_cdf, unsigned cdfnum)
{
    const TrcCodec &r = codec_row(codec);
    if (!r.enc) return fail(TRC_E_ARG, "codec %d not available", codec);
    if (!chunk_ok(chunk)) return fail(TRC_E_ARG, "chunk %u: must be a multiple of 64 in [%u,%u]", chunk, TRC_CHUNK_MIN, TRC_CHUNK_MAX);
    if ((n + chunk - 1) / chunk > 0x7fffffffu) return fail(TRC_E_ARG, "too many chunks");
    if (chunk > r.chunk_max) return fail(TRC_E_ARG, "codec %d: chunk %u exceeds %u", r.id, chunk, r.chunk_max);
    if (r.cdf && (!d_cdf || cdfnum < 1 || cdfnum > 256)) return fail(TRC_E_CDF, "static coder needs a CDF with 1..256 symbols");
    if (r.ss && (d_cdf || !ss_prm_ok(cdfnum)))
        return fail(TRC_E_ARG, "codec %d takes no CDF and cdfnum = TRC_SS_PRM(prm0, prm1) with both in 1..15 (got %s, 0x%x)", r.id, d_cdf ? "a CDF" : "none", cdfnum);
    return TRC_OK;
}

// ------------------------------------------------------------------ coder-kernel timing (opt-in) ---
// Event pairs ride on every coder launch of a call made while timing is on (TRC_LAUNCH_TIMED, trc_launch.h): two-pass
// encoders contribute both passes.  The pool is process-wide and guarded by a mutex; which direction a launch belongs
// to is a per-thread flag set around the launches of one trc_encode_dev / trc_decode_dev call.
#define TRC_TM_MAX 4096
static struct TmState {
    std::mutex mu;
    bool on = false;
    int calls[3] = { 0, 0, 0 }, pairs[3] = { 0, 0, 0 };       // 0 encode coder kernels, 1 decode coder kernels, 2 the encode path's scan + gather
    hipEvent_t ev[3][TRC_TM_MAX][2];
    bool made[3][TRC_TM_MAX] = {};
    bool paused = false;
} g_tm;
static thread_local int tm_dir = -1;                            // direction of the call in progress on this thread, -1 = not timing
extern "C" int trc_timing_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_tm.mu);
    g_tm.on = on != 0; g_tm.paused = false;
    for (int d = 0; d < 3; d++) g_tm.calls[d] = g_tm.pairs[d] = 0;
    return TRC_OK;
}
// suspend / resume without touching what has been collected (a caller that times a sample of its calls)
extern "C" int trc_timing_pause(int paused)
{
    std::lock_guard<std::mutex> lk(g_tm.mu);
    g_tm.paused = paused != 0;
    return TRC_OK;
}
bool trc_tm_next(hipEvent_t *start, hipEvent_t *stop)
{
    if (tm_dir < 0) return false;
    std::lock_guard<std::mutex> lk(g_tm.mu);
    const int d = tm_dir, i = g_tm.pairs[d];
    if (!g_tm.on || i >= TRC_TM_MAX) return false;
    if (!g_tm.made[d][i]) {
        if (hipEventCreate(&g_tm.ev[d][i][0]) != hipSuccess || hipEventCreate(&g_tm.ev[d][i][1]) != hipSuccess) return false;
        g_tm.made[d][i] = true;
    }
    *start = g_tm.ev[d][i][0]; *stop = g_tm.ev[d][i][1];
    g_tm.pairs[d] = i + 1;
    return true;
}
static inline void tm_begin(int dec)
{
    std::lock_guard<std::mutex> lk(g_tm.mu);
    tm_dir = (g_tm.on && !g_tm.paused) ? dec : -1;
}
static inline void tm_end(int dec)
{
    if (tm_dir < 0) return;
    tm_dir = -1;
    std::lock_guard<std::mutex> lk(g_tm.mu);
    g_tm.calls[dec]++;
}
// decode = 2: the encode path's own directory work, the group scan (large inputs) and the payload gather.
// total_ms = summed duration of every coder kernel launched by the calls of that direction since enable(1);
// launches = number of CALLS (so total_ms / launches is the coder-kernel time of one encode or decode, all passes)
extern "C" int trc_timing_read(int decode, double *total_ms, int *launches)
{
    const int d = decode == 2 ? 2 : decode ? 1 : 0;
    int np, nc;
    { std::lock_guard<std::mutex> lk(g_tm.mu); np = g_tm.pairs[d]; nc = g_tm.calls[d]; }
    double sum = 0;
    for (int i = 0; i < np; i++) {
        float ms = 0;
        HIPCHK(hipEventSynchronize(g_tm.ev[d][i][1]));
        HIPCHK(hipEventElapsedTime(&ms, g_tm.ev[d][i][0], g_tm.ev[d][i][1]));
        sum += ms;
    }
    if (total_ms) *total_ms = sum;
    if (launches) *launches = nc;
    return TRC_OK;
}
thread_local TrcGate trc_gate_tls = { nullptr, 0 };
bool trc_gate_ok(int codec)
{
    static const bool off = getenv("TRC_HOST_NO_GATE") != nullptr;       // tuning aid / tests: the slice pipeline for every coder
    return !off && codec_row(codec).gate;
}
thread_local TrcProg trc_prog_tls = { nullptr, nullptr, 0 };
bool trc_prog_ok(int codec)
{
    static const bool off = getenv("TRC_HOST_NO_GATE") != nullptr;
    return !off && codec_row(codec).prog;
}
bool trc_first_use_on_device(unsigned long long *mask)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    const unsigned long long bit = 1ull << dev;
    if (*mask & bit) return false;
    *mask |= bit;
    return true;
}

// ------------------------------------------------------------------------------ layer 2: *_dev ---
extern "C" int trc_cdfini_dev(const void *d_in, size_t n, uint16_t *d_cdf, unsigned cdfnum,
                              int32_t *d_status, void *d_work, void *stream)
{
    if (!n || cdfnum < 1 || cdfnum > 256) return fail(TRC_E_ARG, "cdfini: n=%zu cdfnum=%u", n, cdfnum);
    trc_launch_cdfini((const uint8_t *)d_in, n, d_cdf, cdfnum, d_status, (uint64_t *)d_work, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

extern "C" int trc_hist_dev(const void *d_in, size_t n, uint64_t *d_hist, void *stream)
{
    if (!d_hist) return fail(TRC_E_ARG, "hist: null histogram");
    if (n) trc_launch_hist((const uint8_t *)d_in, n, d_hist, (hipStream_t)stream);
    else HIPCHK(hipMemsetAsync(d_hist, 0, 256 * sizeof(uint64_t), (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return TRC_OK;
}
extern "C" int trc_cdf_from_hist_dev(const uint64_t *d_hist, size_t n_total, uint16_t *d_cdf, unsigned cdfnum,
                                     int32_t *d_status, void *stream)
{
    if (!n_total || cdfnum < 1 || cdfnum > 256) return fail(TRC_E_ARG, "cdf_from_hist: n=%zu cdfnum=%u", n_total, cdfnum);
    trc_launch_cdf_build(d_hist, n_total, d_cdf, cdfnum, d_status, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

extern "C" int trc_tables_dev(const uint16_t *d_cdf, unsigned cdfnum, void *d_work, size_t work_bytes, void *stream)
{
    if (!d_cdf || cdfnum < 1 || cdfnum > 256) return fail(TRC_E_CDF, "tables: need a CDF with 1..256 symbols");
    if (!d_work || work_bytes < up256(TRC_TAB_BYTES) || (((uintptr_t)d_work) & 255)) return fail(TRC_E_WORK, "tables: workspace too small or misaligned");
    trc_launch_static_prep(d_cdf, cdfnum, (uint8_t *)d_work, (hipStream_t)stream);   // the table area opens the workspace (carve)
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

extern "C" int trc_encode_dev(int codec, const void *d_in, size_t n, uint32_t chunk,
                              const uint16_t *d_cdf, unsigned cdfnum,
                              uint32_t *d_clen, void *d_payload, uint64_t *d_total,
                              void *d_work, size_t work_bytes, void *stream)
{
    const bool tables_ready = codec & TRC_TABLES_READY;
    codec &= ~TRC_TABLES_READY;
    int rc = check_common(codec, n, chunk, d_cdf, cdfnum);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_payload & 1) || ((uintptr_t)d_total & 7))
        return fail(TRC_E_ARG, "encode: d_in must be 16-byte, d_clen 4-byte, d_payload 2-byte, d_total 8-byte aligned");
    if (n == 0) { HIPCHK(hipMemsetAsync(d_total, 0, 8, s)); return TRC_OK; }
    const TrcCodec &r = codec_row(codec);
    TrcWork w;
    if ((rc = carve(r, n, chunk, d_work, work_bytes, w))) return rc;
    w.ss_prm = r.ss ? cdfnum : 0u;
    if (r.cdf && !tables_ready) trc_launch_static_prep(d_cdf, cdfnum, w.tables, s);
    tm_begin(0);
    r.enc(r, (const uint8_t *)d_in, n, chunk, w, d_clen, s);
    tm_end(0);
    tm_begin(2);
    if (w.goff) trc_launch_scan_groups(w.gsum, w.ngroups, w.goff, d_total, s);
    trc_launch_gather((const uint8_t *)d_in, n, chunk, w, r.gather, d_clen, (uint8_t *)d_payload, d_total, s);
    tm_end(2);
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

extern "C" int trc_decode_dev(int codec, const uint32_t *d_clen, const void *d_payload, size_t n, uint32_t chunk,
                              const uint16_t *d_cdf, unsigned cdfnum,
                              void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const bool tables_ready = codec & TRC_TABLES_READY, dir_ready = codec & TRC_DIR_READY;
    codec &= ~(TRC_TABLES_READY | TRC_DIR_READY);
    int rc = check_common(codec, n, chunk, d_cdf, cdfnum);
    if (rc) return rc;
    if (n == 0) return TRC_OK;
    if (((uintptr_t)d_out & 15) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_payload & 1))
        return fail(TRC_E_ARG, "decode: d_out must be 16-byte, d_clen 4-byte, d_payload 2-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const TrcCodec &r = codec_row(codec);
    TrcWork w;
    if ((rc = carve(r, n, chunk, d_work, work_bytes, w))) return rc;
    w.ss_prm = r.ss ? cdfnum : 0u;
    if (r.cdf && !tables_ready) trc_launch_static_prep(d_cdf, cdfnum, w.tables, s);
    // TRC_DIR_READY promises that the last encode OR DECODE on this workspace was of this directory (include/trc_hip.h), so both must
    // leave every group's base in goff_area: an encode's gather does (trc_launch.h); a decode derives the sums from clen[] and scans
    // them into the same place.  (Round 4 read goff_area after a decode that had never written it -- a workspace that only ever
    // decoded fed its second decode whatever the memory held: ADVICE r4.)
    if (!dir_ready) {
        trc_launch_group_sums(d_clen, w.nchunks, n, chunk, w.gsum, s);
        trc_launch_scan_groups(w.gsum, w.ngroups, w.goff_area, nullptr, s);
    }
    w.goff = w.goff_area;
    tm_begin(1);
    r.dec(r, (const uint8_t *)d_payload, d_clen, n, chunk, w, (uint8_t *)d_out, s);
    tm_end(1);
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

// ---- decode of a chunk range ------------------------------------------------------------------------------------
// Chunks [first_chunk, first_chunk + count) of a container are a container of their own -- the same payload area, the directory
// from entry first_chunk on -- once their groups' offsets are known: the decoders take ABSOLUTE group offsets (w.goff above).  The
// range workspace holds the index of the FULL directory (per-group sums and their scan: 12 bytes per 64 chunks, placed by (n, chunk)
// alone, so that TRC_DIR_READY finds it whatever the last range was), the range's own group sums and offsets
// (trc_range_dir_kernel, trc_dir.hip), and what a decoder of `count` chunks uses: the tables and the models.  No scratch regions,
// no record stacks, no aux words: those serve the encoders and the gather only (every TrcDecFn reads w.tables, w.goff, w.gsum,
// w.model, w.nchunks, w.ngroups and nothing else), and their pointers are null here.
//   tables | gsum of the full directory | goff of the full directory | gsum of the range | goff of the range | models
static inline size_t dir_index_bytes(size_t ngroups) { return up256(4 * ngroups) + up256(8 * (ngroups + 1)); }
extern "C" size_t trc_range_work_bytes(int codec, size_t n, uint32_t chunk, size_t count)
{
    const TrcCodec &r = codec_row(codec);
    if (!r.enc || !chunk_ok(chunk) || chunk > r.chunk_max) return 0;
    const size_t nchunks = (n + chunk - 1) / chunk;
    if (!count || count > nchunks || nchunks > 0x7fffffffu) return 0;
    return up256(TRC_TAB_BYTES) + dir_index_bytes((nchunks + 63) / 64) + dir_index_bytes((count + 63) / 64) + model_area_bytes(r, count);
}

extern "C" int trc_decode_range_dev(int codec, const uint32_t *d_clen, const void *d_payload, size_t n, uint32_t chunk,
                                    size_t first_chunk, size_t count,
                                    const uint16_t *d_cdf, unsigned cdfnum,
                                    void *d_out, void *d_work, size_t work_bytes, void *stream)
{
    const bool tables_ready = codec & TRC_TABLES_READY, dir_ready = codec & TRC_DIR_READY;
    codec &= ~(TRC_TABLES_READY | TRC_DIR_READY);
    int rc = check_common(codec, n, chunk, d_cdf, cdfnum);
    if (rc) return rc;
    const size_t nchunks = (n + chunk - 1) / chunk, ngroups = (nchunks + 63) / 64;
    if (first_chunk > nchunks || count > nchunks - first_chunk)
        return fail(TRC_E_ARG, "decode_range: chunks [%zu, %zu + %zu) of %zu", first_chunk, first_chunk, count, nchunks);
    if (count == 0) return TRC_OK;
    if (((uintptr_t)d_out & 15) || ((uintptr_t)d_clen & 3) || ((uintptr_t)d_payload & 1))
        return fail(TRC_E_ARG, "decode_range: d_out must be 16-byte, d_clen 4-byte, d_payload 2-byte aligned");
    const TrcCodec &r = codec_row(codec);
    const size_t need = trc_range_work_bytes(codec, n, chunk, count);
    if (!need || work_bytes < need) return fail(TRC_E_WORK, "workspace %zu B < required %zu B", work_bytes, need);
    if (((uintptr_t)d_work) & 255) return fail(TRC_E_ARG, "workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t ngroups_sub = (count + 63) / 64;
    uint8_t *p = (uint8_t *)d_work;
    TrcWork w = {};
    w.tables = p;                        p += up256(TRC_TAB_BYTES);
    uint32_t *gsum_full = (uint32_t *)p; p += up256(4 * ngroups);
    uint64_t *goff_full = (uint64_t *)p; p += up256(8 * (ngroups + 1));
    w.gsum = (uint32_t *)p;              p += up256(4 * ngroups_sub);
    w.goff = w.goff_area = (uint64_t *)p; p += up256(8 * (ngroups_sub + 1));
    w.model = p;
    w.stride = chunk + r.pad;
    w.stride2 = r.s2_mul * chunk + r.s2_add;
    w.nchunks = (uint32_t)count; w.ngroups = (uint32_t)ngroups_sub;
    w.ss_prm = r.ss ? cdfnum : 0u;
    if (r.cdf && !tables_ready) trc_launch_static_prep(d_cdf, cdfnum, w.tables, s);
    if (!dir_ready) {                    // O(nchunks), once per container and workspace; everything below is O(count)
        trc_launch_group_sums(d_clen, (uint32_t)nchunks, n, chunk, gsum_full, s);
        trc_launch_scan_groups(gsum_full, (uint32_t)ngroups, goff_full, nullptr, s);
    }
    trc_launch_range_dir(d_clen, (uint32_t)nchunks, n, chunk, goff_full, (uint32_t)first_chunk, (uint32_t)count, w.gsum, w.goff, s);
    const size_t b0 = first_chunk * (size_t)chunk, b1 = (first_chunk + count) * (size_t)chunk;
    tm_begin(1);
    r.dec(r, (const uint8_t *)d_payload, d_clen + first_chunk, (b1 < n ? b1 : n) - b0, chunk, w, (uint8_t *)d_out, s);
    tm_end(1);
    HIPCHK(hipGetLastError());
    return TRC_OK;
}

// The kernel that takes the longest in the DEFAULT dispatch of the coder at the bench configurations (100 MB, the library's chunk):
// what a rocprofv3 --kernel-trace of bench.py lists first for that direction.  Two-pass encoders launch more than one kernel (the
// timing pairs sum them); forms at other sizes (the order-1 coder's eight-lane decoder and position-order passes) have
// other names.  Descriptive: nothing is dispatched by this string.
extern "C" const char *trc_kernel_name(int codec, int decode)
{
    const TrcCodec &r = codec_row(codec);
    return decode ? r.kernel_dec : r.kernel_enc;
}

// --------------------------------------------------- layer 1: reference prototypes (host pointers) ---
#include "trc_host.inc"

// Page-lock a caller's buffer for the host-pointer calls (hipHostRegister / hipHostUnregister behind plain C: a harness needs
// no HIP header).  Registration costs ~55 us per MB: once per buffer, not per call.
extern "C" int trc_host_pin(void *p, size_t len)
{
    if (!p || !len) return fail(TRC_E_ARG, "host_pin: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(TRC_E_NODEV, "no HIP device");
    HIPCHK(hipHostRegister(p, len, hipHostRegisterDefault));
    return TRC_OK;
}
extern "C" int trc_host_unpin(void *p)
{
    if (!p) return fail(TRC_E_ARG, "host_unpin: bad arguments");
    HIPCHK(hipHostUnregister(p));
    return TRC_OK;
}

extern "C" size_t trc_container_bound(size_t n, uint32_t chunk)
{
    if (!chunk_ok(chunk)) return 0;
    return sizeof(trc_container_hdr) + 4 * ((n + chunk - 1) / chunk) + n;
}
extern "C" size_t trc_encode_host(int codec, const void *in, size_t n, uint32_t chunk, void *out, size_t outcap,
                                  const uint16_t *cdf, unsigned cdfnum)
{
    if (!codec_ok(codec)) { fail(TRC_E_ARG, "codec %d not available", codec); return 0; }
    if (!outcap) { fail(TRC_E_ARG, "encode_host: outcap must be given"); return 0; }
    return host_encode(codec, (const unsigned char *)in, n, (unsigned char *)out, (const cdf_t *)cdf, (int)cdfnum, chunk, outcap);
}

static int container_verdict(const void *buf, size_t buflen, int codec, size_t outlen, char *why, size_t whysz);
// The bounded decoder: like the reference-named decoder of `codec`, but the caller states how many bytes `in` really holds and the
// container is validated against THAT before anything is read (the reference prototypes carry no input length, so through them a
// forged header can make a decoder read past a short buffer).  Raw streams (inlen == outlen) are copied.  Returns outlen, 0 on error.
extern "C" size_t trc_decode_host(int codec, const void *in, size_t inlen, void *out, size_t outlen,
                                  const uint16_t *cdf, unsigned cdfnum)
{
    if (!codec_ok(codec)) { fail(TRC_E_ARG, "codec %d not available", codec); return 0; }
    if (!in || !out) { fail(TRC_E_ARG, "decode_host: bad arguments"); return 0; }
    if (outlen == 0) return 0;
    // inlen == outlen is the reference's "stored raw" convention -- but trc_encode_host with a stated capacity returns the
    // container whatever its size, so a container of exactly outlen bytes is possible (nearly incompressible input): what
    // validates as a container of this coder and this length is decoded, anything else of that size is the raw copy.
    char why[200];
    if (inlen == outlen && container_verdict(in, inlen, codec, outlen, why, sizeof why)) { memcpy(out, in, outlen); return outlen; }   // raw: not an error, nothing reported
    if (inlen != outlen && trc_container_check(in, inlen, codec, outlen)) return 0;
    return host_decode(codec, (const unsigned char *)in, outlen, (unsigned char *)out, (const cdf_t *)cdf, (int)cdfnum);
}

// ---- container validation for untrusted input (the reference prototypes carry no input length) ------
// Everything a decoder will read from buf is checked against buflen: header fields, the directory, and that the
// directory's (clamped) lengths add up to exactly the stated payload, which must end inside the buffer.
// quiet form: the verdict and, on failure, its reason in `why` -- nothing printed, trc_last_error() untouched (the raw-or-container
// probe of trc_decode_host is not an error)
static int container_verdict(const void *buf, size_t buflen, int codec, size_t outlen, char *why, size_t whysz)
{
#define BAD(...) do { snprintf(why, whysz, __VA_ARGS__); return TRC_E_ARG; } while (0)
    trc_container_hdr h;
    if (!buf || buflen < sizeof h) BAD("container: %zu bytes is shorter than the header", buflen);
    memcpy(&h, buf, sizeof h);
    if (h.magic != TRC_MAGIC || h.version != 1) BAD("container: bad magic/version");
    if (!codec_ok(h.codec) || (codec && h.codec != codec)) BAD("container: codec %u (expected %d)", h.codec, codec);
    if (codec_row(h.codec).ss && !ss_prm_ok(h.cdfnum)) BAD("container: codec %u with parameters 0x%x (each must be 1..15)", h.codec, h.cdfnum);
    if (!chunk_ok(h.chunk)) BAD("container: chunk %u", h.chunk);
    if (outlen != (size_t)-1 && h.n != outlen) BAD("container: holds %llu bytes, caller expects %zu", (unsigned long long)h.n, outlen);
    if (h.n == 0 || (h.n + h.chunk - 1) / h.chunk != h.nchunks) BAD("container: nchunks %u does not match n/chunk", h.nchunks);
    const size_t dir = 4 * (size_t)h.nchunks;
    if (dir > buflen - sizeof h) BAD("container: directory (%zu B) runs past the buffer", dir);
    if (h.payload > h.n || h.payload > buflen - sizeof h - dir) BAD("container: payload (%llu B) runs past the buffer", (unsigned long long)h.payload);
    const uint8_t *d = (const uint8_t *)buf + sizeof h;
    uint64_t sum = 0;
    for (uint32_t c = 0; c < h.nchunks; c++) {
        uint32_t l; memcpy(&l, d + 4 * (size_t)c, 4);
        const uint64_t len = (c + 1 == h.nchunks) ? h.n - (uint64_t)c * h.chunk : h.chunk;
        sum += l < len ? l : len;                               // the decoders read an entry above the chunk length as "raw"
    }
    if (sum != h.payload) BAD("container: directory sums to %llu, header says %llu", (unsigned long long)sum, (unsigned long long)h.payload);
    return TRC_OK;
#undef BAD
}
extern "C" int trc_container_check(const void *buf, size_t buflen, int codec, size_t outlen)
{
    char why[200];
    return container_verdict(buf, buflen, codec, outlen, why, sizeof why) ? fail(TRC_E_ARG, "%s", why) : TRC_OK;
}

// ---- a byte range of a container: trc_container_range, trc_decode_range_host ------------------------------------
#include "trc_range.inc"

// ---- byte planes of 16 / 32 / 64-bit elements: device wrappers, the TRCP container, its host calls ----------------
#include "trc_planes.inc"
#include "trc_splanes.inc"
#include "trc_oplanes.inc"
#include "trc_bplanes.inc"
#include "trc_planes_batch.inc"
#include "trc_planes_container.inc"
#include "trc_planes_bcontainer.inc"
#include "trc_planes_ocontainer.inc"

// ---- exports with the reference's names (include/turborc.h:500, include/anscdf.h:40-96) ----------
static bool ss_args_ok(const char *who, unsigned prm0, unsigned prm1)
{
    if (prm0 >= 1 && prm0 <= 15 && prm1 >= 1 && prm1 <= 15) return true;
    fail(TRC_E_ARG, "%s: parameters (%u, %u) must both be in 1..15", who, prm0, prm1);
    return false;
}
extern "C" {

// cdfini: reference rccdf.c:50-68.  Returns (int)inlen; -1 where the reference would die().
int cdfini(unsigned char *in, size_t inlen, cdf_t *cdf, unsigned cdfnum)
{
    if (!inlen || cdfnum < 1 || cdfnum > 256) { fail(TRC_E_ARG, "cdfini: inlen=%zu cdfnum=%u", inlen, cdfnum); return -1; }
#define ICHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail(TRC_E_HIP, "%s -> %s", #x, hipGetErrorString(e_)); return -1; } } while (0)
    const std::vector<int> devs = devs_get();
    if (devs.size() > 1) {
        // over the device list: every pipeline counts the bytes of its share (trc_hist_dev), the counts are summed on the host -- exact, so the
        // CDF is the one-device CDF bit for bit -- and the first pipeline turns the sum into the CDF (trc_cdf_from_hist_dev)
        const int nd = (int)devs.size();
        std::vector<uint64_t> hist((size_t)nd * 256, 0);
        std::vector<std::string> errs((size_t)nd);
        int prev = 0;
        (void)hipGetDevice(&prev);
        auto one = [&](int s) {
            HostCtx &c = g_mctxs[s];
            std::lock_guard<std::mutex> lk(c.mu);
            const size_t o = inlen / nd * s, l = s + 1 == nd ? inlen - o : inlen / nd;
            if (!l) return;
            uint64_t *d_hist = nullptr;
            if (hipSetDevice(devs[s]) != hipSuccess || ctx_init(c, devs[s]) || grow(&c.d_in, &c.cap_in, l)) { errs[s] = "device setup failed"; return; }
            d_hist = (uint64_t *)(c.d_small + 40960);
            if (hipMemcpyAsync(c.d_in, in + o, l, hipMemcpyHostToDevice, c.s_k[0]) != hipSuccess || trc_hist_dev(c.d_in, l, d_hist, c.s_k[0]) ||
                hipMemcpyAsync(&hist[(size_t)s * 256], d_hist, 2048, hipMemcpyDeviceToHost, c.s_k[0]) != hipSuccess ||
                hipStreamSynchronize(c.s_k[0]) != hipSuccess) errs[s] = "histogram failed";
        };
        std::vector<std::thread> th;
        for (int s = 1; s < nd; s++) th.emplace_back(one, s);
        one(0);
        for (auto &x : th) x.join();
        for (int s = 0; s < nd; s++) if (!errs[s].empty()) { (void)hipSetDevice(prev); fail(TRC_E_HIP, "cdfini over the device list: %s", errs[s].c_str()); return -1; }
        for (int s = 1; s < nd; s++) for (int k = 0; k < 256; k++) hist[k] += hist[(size_t)s * 256 + k];
        HostCtx &c = g_mctxs[0];
        std::lock_guard<std::mutex> lk(c.mu);
        int32_t st = -1;
        uint64_t *d_hist = (uint64_t *)(c.d_small + 40960);
        uint16_t *d_cdf = (uint16_t *)c.d_small;
        int32_t *d_status = (int32_t *)(c.d_small + 32768);
        const bool ok = hipSetDevice(devs[0]) == hipSuccess &&
                        hipMemcpyAsync(d_hist, hist.data(), 2048, hipMemcpyHostToDevice, c.s_k[0]) == hipSuccess &&
                        trc_cdf_from_hist_dev(d_hist, inlen, d_cdf, cdfnum, d_status, c.s_k[0]) == TRC_OK &&
                        hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, c.s_k[0]) == hipSuccess &&
                        hipMemcpyAsync(cdf, d_cdf, (cdfnum + 1) * sizeof(cdf_t), hipMemcpyDeviceToHost, c.s_k[0]) == hipSuccess &&
                        hipStreamSynchronize(c.s_k[0]) == hipSuccess;
        (void)hipSetDevice(prev);
        if (!ok) { fail(TRC_E_HIP, "cdfini over the device list: building the CDF failed"); return -1; }
        if (st < 0) { fail(TRC_E_CDF, "cdfini: distribution cannot be normalised to a strictly increasing 15-bit CDF"); return -1; }
        return (int)inlen;
    }
    HostCtx *cp = nullptr;
    int dev = 0;
    if (devs.size() == 1) { cp = &g_mctxs[0]; dev = devs[0]; }
    else { if (ctx_get(cp)) return -1; if (hipGetDevice(&dev) != hipSuccess) return -1; }
    HostCtx &c = *cp;
    std::lock_guard<std::mutex> lk(c.mu);
    int prev = dev;
    (void)hipGetDevice(&prev);
    if (prev != dev) ICHK(hipSetDevice(dev));
    struct Back { int p, d; ~Back() { if (p != d) (void)hipSetDevice(p); } } back = { prev, dev };
    if (ctx_init(c, dev)) return -1;
    if (grow(&c.d_in, &c.cap_in, inlen) || grow(&c.d_work[0], &c.cap_work[0], 4096)) return -1;
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    int32_t *d_status = (int32_t *)(c.d_small + 32768);
    ICHK(hipMemcpyAsync(c.d_in, in, inlen, hipMemcpyHostToDevice, c.s_k[0]));
    if (trc_cdfini_dev(c.d_in, inlen, d_cdf, cdfnum, d_status, c.d_work[0], c.s_k[0])) return -1;
    int32_t st = -1;
    ICHK(hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, c.s_k[0]));
    ICHK(hipMemcpyAsync(cdf, d_cdf, (cdfnum + 1) * sizeof(cdf_t), hipMemcpyDeviceToHost, c.s_k[0]));
    ICHK(hipStreamSynchronize(c.s_k[0]));
    if (st < 0) { fail(TRC_E_CDF, "cdfini: distribution cannot be normalised to a strictly increasing 15-bit CDF"); return -1; }
    return (int)inlen;
}

void anscdfini(unsigned id) { (void)id; }   // reference: CPU ISA dispatch (anscdf.c:759-808); nothing to select here

#define TRC_EXPORT_ANS4S(sfx) \
    size_t anscdf4senc##sfx(unsigned char *in, size_t inlen, unsigned char *out, cdf_t *cdf) { return host_encode(TRC_ANS4S, in, inlen, out, cdf, 0); } \
    size_t anscdf4sdec##sfx(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf) { return host_decode(TRC_ANS4S, in, outlen, out, cdf, 0); }
TRC_EXPORT_ANS4S()
TRC_EXPORT_ANS4S(0)
TRC_EXPORT_ANS4S(s)
TRC_EXPORT_ANS4S(x)

// static-CDF range coder: rccdfsenc + the four equivalent decoders, rccdfs2enc + its two decoders
size_t rccdfsenc(unsigned char *in, size_t inlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_encode(TRC_RCS1, in, inlen, out, cdf, (int)cdfnum); }
#define TRC_EXPORT_RCS1DEC(name) size_t name(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_decode(TRC_RCS1, in, outlen, out, cdf, (int)cdfnum); }
TRC_EXPORT_RCS1DEC(rccdfsldec)
TRC_EXPORT_RCS1DEC(rccdfsbdec)
TRC_EXPORT_RCS1DEC(rccdfsvldec)
TRC_EXPORT_RCS1DEC(rccdfsvbdec)
// one stream, 32-bit range / 16-bit I/O (reference rccdf.c:648-694; turborc -e44) -- SURVEY 8f rank 1
size_t rccdfsmenc(unsigned char *in, size_t inlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_encode(TRC_RCSM, in, inlen, out, cdf, (int)cdfnum); }
size_t rccdfsmbdec(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_decode(TRC_RCSM, in, outlen, out, cdf, (int)cdfnum); }
size_t rccdfsmldec(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_decode(TRC_RCSM, in, outlen, out, cdf, (int)cdfnum); }
size_t rccdfs2enc(unsigned char *in, size_t inlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_encode(TRC_RCS2, in, inlen, out, cdf, (int)cdfnum); }
size_t rccdfsl2dec(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_decode(TRC_RCS2, in, outlen, out, cdf, (int)cdfnum); }
size_t rccdfsb2dec(unsigned char *in, size_t outlen, unsigned char *out, cdf_t *cdf, unsigned cdfnum) { return host_decode(TRC_RCS2, in, outlen, out, cdf, (int)cdfnum); }

// the coders without a CDF: one encoder and one decoder name per id; TRC_HOST4 adds the names with the reference's 0 / s / x
// ISA suffixes, which all run the same coder here
#define TRC_HOST(enc, dec, id) \
    size_t enc(unsigned char *in, size_t inlen, unsigned char *out) { return host_encode(id, in, inlen, out, nullptr, 0); } \
    size_t dec(unsigned char *in, size_t outlen, unsigned char *out) { return host_decode(id, in, outlen, out, nullptr, 0); }
#define TRC_HOST4(enc, dec, id) TRC_HOST(enc, dec, id) TRC_HOST(enc##0, dec##0, id) TRC_HOST(enc##s, dec##s, id) TRC_HOST(enc##x, dec##x, id)

// bitwise order-0 range coder, "s" predictor (reference rc_.c:37-58; turborc -e1 / file codec 1)
TRC_HOST(rcsenc, rcsdec, TRC_RCB)

// bitwise order-1 range coders, "s" predictor (reference rc_.c:186-209 and :372-400; turborc -e2 / -e4, file codecs 2 / 4)
TRC_HOST(rccsenc, rccsdec, TRC_RCC1)              TRC_HOST(rcxsenc, rcxsdec, TRC_RCX1)

// gamma / Rice integer coders (reference rc_.c:464-842; turborc -e26 .. -e29)
TRC_HOST(rcgsenc8, rcgsdec8, TRC_RCG8)        TRC_HOST(rcgsenc16, rcgsdec16, TRC_RCG16)     TRC_HOST(rcgsenc32, rcgsdec32, TRC_RCG32)
TRC_HOST(rcgzsenc8, rcgzsdec8, TRC_RCGZ8)     TRC_HOST(rcgzsenc16, rcgzsdec16, TRC_RCGZ16)  TRC_HOST(rcgzsenc32, rcgzsdec32, TRC_RCGZ32)
TRC_HOST(rcrsenc8, rcrsdec8, TRC_RCR8)        TRC_HOST(rcrsenc16, rcrsdec16, TRC_RCR16)     TRC_HOST(rcrsenc32, rcrsdec32, TRC_RCR32)
TRC_HOST(rcrzsenc8, rcrzsdec8, TRC_RCRZ8)     TRC_HOST(rcrzsenc16, rcrzsdec16, TRC_RCRZ16)  TRC_HOST(rcrzsenc32, rcrzsdec32, TRC_RCRZ32)

// Turbo-VLC coders on the bitwise range coder (reference rc_.c:1012-1336; turborc -e30 / -e33 / -e35 / -e36)
TRC_HOST(rcvsenc16, rcvsdec16, TRC_RCBV16)       TRC_HOST(rcvsenc32, rcvsdec32, TRC_RCBV32)
TRC_HOST(rcvzsenc16, rcvzsdec16, TRC_RCBVZ16)    TRC_HOST(rcvzsenc32, rcvzsdec32, TRC_RCBVZ32)
TRC_HOST(rcvgsenc16, rcvgsdec16, TRC_RCBVG16)    TRC_HOST(rcvgsenc32, rcvgsdec32, TRC_RCBVG32)
TRC_HOST(rcvgzsenc16, rcvgzsdec16, TRC_RCBVGZ16) TRC_HOST(rcvgzsenc32, rcvgzsdec32, TRC_RCBVGZ32)

// bitwise word coders (reference rc_.c:60-138, 248-342; turborc -e6 / -e7 / -e8)
TRC_HOST(rcsenc16, rcsdec16, TRC_RCW16)      TRC_HOST(rcsenc32, rcsdec32, TRC_RCW32)
TRC_HOST(rccsenc32, rccsdec32, TRC_RCCW32)   TRC_HOST(rcc2senc32, rcc2sdec32, TRC_RCC2W32)

// bitwise nibble coders, adaptive and static (reference rc_.c:141-184; turborc -n -e41 / -e40), and the structured 3/5/8-bit
// varint byte coder (rc_.c:442-462; turborc -e17)
TRC_HOST(rc4senc, rc4sdec, TRC_RC4)          TRC_HOST(rc4csenc, rc4csdec, TRC_RC4C)       TRC_HOST(rcu3senc, rcu3sdec, TRC_RCU3)

// the same byte-level coders on the dual-rate "ss" predictor (reference rc_ss.c; turborc -pss -rNM): the two shift parameters
// are arguments; a decoder uses its own and fails where the container's header holds other ones
#define TRC_HOST_SS(enc, dec, id) \
    size_t enc(unsigned char *in, size_t inlen, unsigned char *out, unsigned prm0, unsigned prm1) \
    { return ss_args_ok(#enc, prm0, prm1) ? host_encode(id, in, inlen, out, nullptr, (int)TRC_SS_PRM(prm0, prm1)) : 0; } \
    size_t dec(unsigned char *in, size_t outlen, unsigned char *out, unsigned prm0, unsigned prm1) \
    { return ss_args_ok(#dec, prm0, prm1) ? host_decode(id, in, outlen, out, nullptr, (int)TRC_SS_PRM(prm0, prm1)) : 0; }
TRC_HOST_SS(rcssenc, rcssdec, TRC_RCSS)          TRC_HOST_SS(rc4ssenc, rc4ssdec, TRC_RC4SS)
TRC_HOST_SS(rc4cssenc, rc4cssdec, TRC_RC4CSS)    TRC_HOST_SS(rcu3ssenc, rcu3ssdec, TRC_RCU3SS)
#undef TRC_HOST_SS

// adaptive-CDF byte range coder (reference rccdf.c:187-211; turborc -e46)
TRC_HOST(rccdfenc, rccdfdec, TRC_RCA)
// interleaved adaptive-CDF byte range coder (reference rccdf.c:213-249; turborc -e47) -- SURVEY 8f rank 1
TRC_HOST(rccdfienc, rccdfidec, TRC_RCAI)
// "vnibble" adaptive-CDF range coders (reference rccdf.c:326-390; turborc -e48 / -e49)
TRC_HOST(rccdfenc8, rccdfdec8, TRC_RCV8)         TRC_HOST(rccdfienc8, rccdfidec8, TRC_RCVI8)
// adaptive-CDF byte rANS (reference anscdf.c:567-605, dispatch :816-817; turborc -e56 / -e57 / -e58)
TRC_HOST4(anscdfenc, anscdfdec, TRC_ANSA)
// the `turborc -n` coders on values 0..15 -- SURVEY 8f rank 1
// adaptive-CDF nibble range coder, one stream (reference rccdf.c:250-275) and interleaved (rccdf.c:277-323)
TRC_HOST(rccdf4enc, rccdf4dec, TRC_RCA4)         TRC_HOST(rccdf4ienc, rccdf4idec, TRC_RCAI4)
// adaptive-CDF nibble rANS (reference anscdf.c:87-133, dispatch :814-815)
TRC_HOST4(anscdf4enc, anscdf4dec, TRC_ANSA4)
// order-1 adaptive-CDF byte rANS (reference anscdf.c:607-645, dispatch :818-819; turborc -e64) -- SURVEY 8f rank 2
TRC_HOST4(anscdf1enc, anscdf1dec, TRC_ANSO1)
// bitwise order-0 rANS (reference anscdf.c:672-731; turborc -e66) -- SURVEY 8f rank 2.  Chunks above one reference
// block (8192 bytes) are not supported by the kernels: the call uses min(configured chunk, 8192).
TRC_HOST(ansbc, ansbd, TRC_ANSB)

// Turbo-VLC integer coders over the adaptive CDF range coder (reference rccdf.c:391-632; turborc -e50/52/53 with 16- or
// 32-bit input) -- SURVEY 8f rank 3.  Lengths are byte counts, as in the reference.
TRC_HOST(rccdfuenc16, rccdfudec16, TRC_VLCU16)   TRC_HOST(rccdfuenc32, rccdfudec32, TRC_VLCU32)
TRC_HOST(rccdfvenc16, rccdfvdec16, TRC_VLCV16)   TRC_HOST(rccdfvenc32, rccdfvdec32, TRC_VLCV32)
TRC_HOST(rccdfvzenc16, rccdfvzdec16, TRC_VLCVZ16) TRC_HOST(rccdfvzenc32, rccdfvzdec32, TRC_VLCVZ32)
// ... and over the adaptive CDF rANS (reference anscdf.c:139-483, dispatch :820-833; turborc -e60..63)
TRC_HOST4(anscdfuenc16, anscdfudec16, TRC_VLAU16)    TRC_HOST4(anscdfuzenc16, anscdfuzdec16, TRC_VLAUZ16)
TRC_HOST4(anscdfvenc16, anscdfvdec16, TRC_VLAV16)    TRC_HOST4(anscdfvzenc16, anscdfvzdec16, TRC_VLAVZ16)
TRC_HOST4(anscdfvenc32, anscdfvdec32, TRC_VLAV32)    TRC_HOST4(anscdfvzenc32, anscdfvzdec32, TRC_VLAVZ32)
#undef TRC_HOST4
#undef TRC_HOST

typedef size_t (*fanscdfenc)(unsigned char *in, size_t inlen, unsigned char *out);
typedef size_t (*fanscdfdec)(unsigned char *in, size_t inlen, unsigned char *out);
fanscdfenc _anscdfenc = anscdfenc;      // the reference's dispatch globals (include/anscdf.h:32-35)
fanscdfdec _anscdfdec = anscdfdec;
fanscdfenc _anscdf4enc = anscdf4enc;
fanscdfdec _anscdf4dec = anscdf4dec;

}  // extern "C"
