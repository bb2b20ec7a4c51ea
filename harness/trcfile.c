/* trcfile.c -- minimal file compressor on top of the drop-in headers ("makes the chunked format a
 * usable file compressor").  Plain C, links only against libturborc_hip.so.
 *
 *   trcfile c <id> <in> <out>     compress   (id: TurboRC -e numbers 1, 42, 44, 45, 46, 47, 56, 64, 65, 66)
 *   trcfile c <id> <in> <out> [-r NM]   id 62 .. 65 with -r or without: the library's "ss" predictor coders TRC_RCSS, TRC_RC4SS,
 *                                 TRC_RC4CSS, TRC_RCU3SS (trc_hip.h) with the parameters N and M (two digits 1..9, default 56);
 *                                 the container's header records them, so d and x take no option.  Without -r, 64 and 65 are
 *                                 the TurboRC numbers above
 *   trcfile p <id> <esize> <in> <out>   compress the BYTE PLANES of esize-byte elements (2, 4 or 8: bf16 / fp16, fp32, fp64 and wide
 *                                 integers), each plane with coder <id>: the file is the library's TRCP container (trc_hip.h), which
 *                                 records everything d and x need; static coders (42, 44, 45, 65) get a CDF per plane
 *   trcfile f <id> <esize> <z|x> <in> <out>   as p, with a filter ahead of the planes: z = zigzag delta, x = xor against the
 *                                 previous element, restarted at every chunk -- for integer columns and smooth series (sorted ids,
 *                                 timestamps, sampled signals).  The file is the library's filtered planes container: 16 bytes
 *                                 "TRCF" | u8 filter | u8 1 | u16 0 | u64 size, then the TRCP container of the filtered data
 *   trcfile s <id> <esize> <z|x> <stride> <in> <out>   as f for INTERLEAVED data (rows of K fields, stereo / 5.1 PCM, xyz points, complex
 *                                 pairs): the filter predicts from the element <stride> back, 2 .. 8.  The file is the library's
 *                                 strided planes container: 16 bytes "TRCS" | u8 filter | u8 1 | u16 stride | u64 size, then the TRCP
 *                                 container of the filtered data
 *   trcfile o <id> <esize> <order> <stride> <in> <out>   as s for SMOOTH series (sampled signals, PCM, sensor readings): the zigzag delta
 *                                 taken <order> times, 2 or 3 (the fixed polynomial predictors of the lossless audio coders), against
 *                                 the element <stride> back, 1 .. 8.  The file is the library's order planes container: 16 bytes "TRCO"
 *                                 | u8 order | u8 1 | u16 stride | u64 size, then the TRCP container of the filtered data
 *   trcfile O <id> <esize> <stride> <in> <out>   as p, f, s or o, whichever the library's order advisor chooses from the order-0
 *                                 histograms of the planes under orders 0 .. 3 at <stride> (trc_encode_aoplanes_host): the file is
 *                                 what that command would have written; prints the four estimates and the chosen order
 *   trcfile r <id> <esize> <z|x> <base> <in> <out>   as f, with the filter RELATIVE TO A BASE FILE: z = zigzag delta, x = xor of every
 *                                 element against the element at the same place in <base> (the previous checkpoint, the base model of
 *                                 a fine-tune, a page before its update), which holds at least the whole elements of <in>.  The file
 *                                 is the library's TRCD container: 32 bytes "TRCD" | u8 filter | u8 1 | u16 0 | u64 size | u64 base
 *                                 bytes | u64 base fingerprint, then the TRCP container of the filtered data
 *   trcfile R <in> <base> <out>   decompress a file of r against its base; a base with another fingerprint is refused.  d and x do
 *                                 not read such a file: they have no base to give
 *   trcfile a <id> <esize> <in> <out>   as p or f, whichever the library's planes advisor chooses from the order-0 histograms of the
 *                                 planes under no filter, z and x (trc_encode_aplanes_host): the file is what p or f would have
 *                                 written; prints the three estimates and the choice (n, z or x)
 *   trcfile b <id> <esize> <chunk|0> <n|z|x|a> <out> <in>...   compress a BATCH: every input file is one item (a tensor, a page, a
 *                                 column) of esize-byte elements, all of them in one coded call; one filter letter for all items (n =
 *                                 none), a = the library's batch advisor chooses per item and every choice is printed, or o = the
 *                                 library's order advisor chooses a predictor order 0 .. 3 per item at stride 1 (a TRCU file where an
 *                                 order above 1 is chosen; l lists it with a stride and an order per item, B decodes from it).  The file is
 *                                 the library's TRCB container (trc_hip.h), which records every item's length and filter
 *   trcfile B <in> <first> <count> <out>   items [first, first + count) of a file of b, their bytes concatenated: only the chunks
 *                                 that cover them are sent to the GPU
 *   trcfile l <in>                list a file of b: count, esize, chunk, coder and every item's bytes and filter (needs no GPU).  B and l
 *                                 also read the library's TRCT container (a TRCB container behind a stride per item, which this
 *                                 tool does not write); l then adds a stride column
 *   trcfile e <id> <esize> <chunk|0> <z|x|a> <out> <in> <base|-> [<in> <base|-> ...]   compress a BATCH AGAINST BASES: every input file is
 *                                 one item and is followed by its base file (the same tensor of the previous checkpoint; at least the
 *                                 item's bytes), or by - for an item without one, which is coded unfiltered.  z / x: that filter for
 *                                 every item with a base; a = the library's advisor against the bases chooses per item
 *                                 (trc_encode_abplanes_batch_host) and every choice is printed.  The file is the library's TRCE
 *                                 container: a fingerprint per base in front of a TRCB container -- or, where no item ends up with a
 *                                 filter, a plain TRCB container, which B reads
 *   trcfile E <in> <item> <base|-> <out>   item <item> of a file of e against its base file (- where it has no filter): only the chunks
 *                                 that cover it are sent to the GPU; a base with another fingerprint is refused.  l lists such a file
 *                                 with every item's base fingerprint (needs no GPU); B does not read it: it has no bases to give
 *   trcfile d <in> <out>          decompress (files of c, p, f, s, o, a and O)
 *   trcfile x <in> <offset> <len> <out>   extract bytes [offset, offset + len) of a file written by `trcfile c`, p, f, s or o: only the
 *                                 chunks that cover them are sent to the GPU and decoded (trc_decode_range_host)
 *
 * File = "TRCF" | u8 id | u8 cdfnum-1 | u16 0 | u64 raw length | u64 stored length | [cdf: (cdfnum+1) x u16, static coders]
 *        | stored bytes (the library's TRC1 container, or the raw input when it does not compress: the reference's
 *        "returned length == input length means stored" convention, include/turborc.h:46-59).
 *   trcfile C <in> <out> [bsize [fc]]  compress to the REFERENCE's file format, file codec fc = 1 (rcsenc per block, the
 *                                      default), 2 (rccsenc) or 4 (rcxsenc); see below
 *   trcfile D <in> <out>          decompress a reference-format file of codec 1, 2 or 4 / predictor "s" with blocks <= 65536
 * The reference's own file mode (hd_t / hdb_t, turborc.c:666-733,1044-1167) codes every block as one serial stream; with
 * blocks that are legal chunk sizes a block IS a chunk, and the two tools read each other's files (C / D below). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/turborc.h"
#include "../include/anscdf.h"
#include "../include/trc_hip.h"

typedef size_t (*fn3)(unsigned char *, size_t, unsigned char *);
typedef size_t (*fn5)(unsigned char *, size_t, unsigned char *, cdf_t *, unsigned);
typedef size_t (*fnp)(unsigned char *, size_t, unsigned char *, unsigned, unsigned);
/* file id of an "ss" coder = 128 | library id (62 and 63 are free TurboRC numbers here, 64 and 65 are not) */
static fnp pick_ss(int codec)
{
    switch (codec) {
    case TRC_RCSS: return rcssenc;
    case TRC_RC4SS: return rc4ssenc;
    case TRC_RC4CSS: return rc4cssenc;
    case TRC_RCU3SS: return rcu3ssenc;
    }
    return 0;
}
static size_t e65(unsigned char *i, size_t n, unsigned char *o, cdf_t *c, unsigned m) { (void)m; return anscdf4senc(i, n, o, c); }
static size_t d65(unsigned char *i, size_t n, unsigned char *o, cdf_t *c, unsigned m) { (void)m; return anscdf4sdec(i, n, o, c); }

/* the reference's file codecs with a GPU coder: 1 rcsenc, 2 rccsenc, 4 rcxsenc (turborc.c:1054-1057) -> container codec, decoder */
static int file_codec(unsigned fc, fn3 *dec)
{
    switch (fc) {
    case 1: *dec = rcsdec; return TRC_RCB;
    case 2: *dec = rccsdec; return TRC_RCC1;
    case 4: *dec = rcxsdec; return TRC_RCX1;
    }
    return 0;
}

static int pick(int id, fn3 *e3, fn3 *d3, fn5 *e5, fn5 *d5)
{
    *e3 = *d3 = 0; *e5 = *d5 = 0;
    switch (id) {
    case 1:  *e3 = rcsenc; *d3 = rcsdec; return 0;
    case 2:  *e3 = rccsenc; *d3 = rccsdec; return 0;
    case 4:  *e3 = rcxsenc; *d3 = rcxsdec; return 0;
    case 46: *e3 = rccdfenc; *d3 = rccdfdec; return 0;
    case 47: *e3 = rccdfienc; *d3 = rccdfidec; return 0;
    case 56: *e3 = anscdfenc; *d3 = anscdfdec; return 0;
    case 64: *e3 = anscdf1enc; *d3 = anscdf1dec; return 0;
    case 66: *e3 = ansbc; *d3 = ansbd; return 0;
    case 42: *e5 = rccdfsenc; *d5 = rccdfsbdec; return 0;
    case 44: *e5 = rccdfsmenc; *d5 = rccdfsmbdec; return 0;
    case 45: *e5 = rccdfs2enc; *d5 = rccdfsb2dec; return 0;
    case 65: *e5 = e65; *d5 = d65; return 0;
    }
    return -1;
}
/* TurboRC id -> the library's coder id, for the calls that take one (trcfile p) */
static int lib_codec(int id)
{
    switch (id) {
    case 1:  return TRC_RCB;
    case 2:  return TRC_RCC1;
    case 4:  return TRC_RCX1;
    case 42: return TRC_RCS1;
    case 44: return TRC_RCSM;
    case 45: return TRC_RCS2;
    case 46: return TRC_RCA;
    case 47: return TRC_RCAI;
    case 56: return TRC_ANSA;
    case 64: return TRC_ANSO1;
    case 65: return TRC_ANS4S;
    case 66: return TRC_ANSB;
    }
    return 0;
}
static int is_planes(const unsigned char *fb, size_t fl) { return fl >= 4 && !memcmp(fb, "TRCP", 4); }
/* a file of `trcfile f`.  `trcfile c` opens its files with the same four letters; there byte 5 is 0 for the coders without a CDF
 * and bytes 16 .. 19 belong to a length, here byte 5 is the version 1 and a TRCP container starts at byte 16 */
static int is_fplanes(const unsigned char *fb, size_t fl) { return fl >= 20 && !memcmp(fb, "TRCF", 4) && fb[5] == 1 && !memcmp(fb + 16, "TRCP", 4); }
/* a file of `trcfile s` */
static int is_splanes(const unsigned char *fb, size_t fl) { return fl >= 20 && !memcmp(fb, "TRCS", 4) && !memcmp(fb + 16, "TRCP", 4); }
/* a file of `trcfile o` */
static int is_oplanes(const unsigned char *fb, size_t fl) { return fl >= 20 && !memcmp(fb, "TRCO", 4) && !memcmp(fb + 16, "TRCP", 4); }
/* a file of `trcfile r` */
static int is_bplanes(const unsigned char *fb, size_t fl) { return fl >= 36 && !memcmp(fb, "TRCD", 4) && !memcmp(fb + 32, "TRCP", 4); }
static int write_file(const char *path, const unsigned char *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    if (fwrite(p, 1, n, f) != n) { perror("write"); fclose(f); return 2; }
    fclose(f);
    return 0;
}
static unsigned char *slurp(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return 0; }
    fseek(f, 0, SEEK_END); *n = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
    unsigned char *p = malloc(*n + 1024);
    if (!p || fread(p, 1, *n, f) != *n) { perror("read"); fclose(f); free(p); return 0; }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    fn3 e3, d3; fn5 e5, d5;
    /* c <id> <in> <out> [-r NM]: ids 62 .. 65 as "ss" coders (64 and 65 only with -r: they are TurboRC numbers too) */
    unsigned prm0 = 5, prm1 = 6;
    int with_r = 0;
    if ((argc == 7 && !strcmp(argv[1], "c") && !strcmp(argv[5], "-r")) || (argc == 6 && !strcmp(argv[1], "c") && !strncmp(argv[5], "-r", 2) && argv[5][2])) {
        const char *v = argc == 7 ? argv[6] : argv[5] + 2;
        if (v[0] < '1' || v[0] > '9' || v[1] < '1' || v[1] > '9' || v[2]) { fprintf(stderr, "-r %s: two digits 1..9\n", v); return 2; }
        prm0 = (unsigned)(v[0] - '0'); prm1 = (unsigned)(v[1] - '0');
        with_r = 1; argc = 5;
    }
    if (argc == 5 && !strcmp(argv[1], "c") && pick_ss(atoi(argv[2])) && (with_r || atoi(argv[2]) < 64)) {
        const int codec = atoi(argv[2]);
        size_t n;
        unsigned char *in = slurp(argv[3], &n);
        if (!in) return 2;
        unsigned char *out = malloc(n + n / 3 + 1024);
        if (!out) { perror("malloc"); return 2; }
        size_t l = n;
        if (n && !(l = pick_ss(codec)(in, n, out, prm0, prm1))) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        FILE *f = fopen(argv[4], "wb");
        if (!f) { perror(argv[4]); return 2; }
        const uint8_t hdr[8] = { 'T', 'R', 'C', 'F', (uint8_t)(128 | codec), 0, 0, 0 };
        const uint64_t raw = n, stored = l;
        fwrite(hdr, 1, 8, f); fwrite(&raw, 8, 1, f); fwrite(&stored, 8, 1, f);
        fwrite(l == n ? in : out, 1, l, f);
        fclose(f);
        printf("%zu -> %zu bytes (%.2f%%)%s\n", n, l, n ? 100.0 * l / n : 0.0, l == n ? "  stored" : "");
        return 0;
    }
    if (with_r) { fprintf(stderr, "-r goes with ids 62 .. 65\n"); return 2; }
    if (argc == 5 && !strcmp(argv[1], "c")) {
        const int id = atoi(argv[2]);
        size_t n;
        if (pick(id, &e3, &d3, &e5, &d5)) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        unsigned char *in = slurp(argv[3], &n);
        if (!in) return 2;
        unsigned char *out = malloc(n + n / 3 + 1024);
        if (!out) { perror("malloc"); return 2; }
        cdf_t cdf[257];
        unsigned m = 0;
        size_t l = n;
        if (n && e5) {
            for (size_t i = 0; i < n; i++) if (in[i] > m) m = in[i];
            if (cdfini(in, n, cdf, m + 1) < 0) { e5 = 0; e3 = 0; }        /* distribution the 15-bit CDF cannot hold: store */
        }
        if (n && (e3 || e5)) {
            l = e3 ? e3(in, n, out) : e5(in, n, out, cdf, m + 1);
            if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        }
        FILE *f = fopen(argv[4], "wb");
        if (!f) { perror(argv[4]); return 2; }
        const uint8_t hdr[8] = { 'T', 'R', 'C', 'F', (uint8_t)id, (uint8_t)m, 0, 0 };
        const uint64_t raw = n, stored = l;
        fwrite(hdr, 1, 8, f); fwrite(&raw, 8, 1, f); fwrite(&stored, 8, 1, f);
        if (e5) fwrite(cdf, sizeof(cdf_t), m + 2, f);
        fwrite(l == n ? in : out, 1, l, f);
        fclose(f);
        printf("%zu -> %zu bytes (%.2f%%)%s\n", n, l, n ? 100.0 * l / n : 0.0, l == n ? "  stored" : "");
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "p")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        unsigned char *in = slurp(argv[4], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_planes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = trc_encode_planes_host(codec, in, n, esize, 0, out, cap, cdfnum);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[5], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes\n", n, l, 100.0 * l / n, esize);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "f")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        const int filter = !strcmp(argv[4], "z") ? TRC_FILTER_ZDELTA : !strcmp(argv[4], "x") ? TRC_FILTER_XOR : TRC_FILTER_NONE;
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (filter == TRC_FILTER_NONE) { fprintf(stderr, "filter %s: z (zigzag delta) or x (xor)\n", argv[4]); return 2; }
        unsigned char *in = slurp(argv[5], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_fplanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = trc_encode_fplanes_host(codec, filter, in, n, esize, 0, out, cap, cdfnum);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[6], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, filter %s\n", n, l, 100.0 * l / n, esize, argv[4]);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "s")) {
        const int id = atoi(argv[2]), codec = lib_codec(id), stride = atoi(argv[5]);
        const unsigned esize = (unsigned)atoi(argv[3]);
        const int filter = !strcmp(argv[4], "z") ? TRC_FILTER_ZDELTA : !strcmp(argv[4], "x") ? TRC_FILTER_XOR : TRC_FILTER_NONE;
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (filter == TRC_FILTER_NONE) { fprintf(stderr, "filter %s: z (zigzag delta) or x (xor)\n", argv[4]); return 2; }
        if (stride < 2 || stride > TRC_STRIDE_MAX) { fprintf(stderr, "stride %s: 2 .. %d (stride 1 is trcfile f)\n", argv[5], TRC_STRIDE_MAX); return 2; }
        unsigned char *in = slurp(argv[6], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_splanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = trc_encode_splanes_host(codec, filter, stride, in, n, esize, 0, out, cap, cdfnum);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[7], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, filter %s, stride %d\n", n, l, 100.0 * l / n, esize, argv[4], stride);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "o")) {
        const int id = atoi(argv[2]), codec = lib_codec(id), order = atoi(argv[4]), stride = atoi(argv[5]);
        const unsigned esize = (unsigned)atoi(argv[3]);
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (order < 2 || order > TRC_ORDER_MAX) { fprintf(stderr, "order %s: 2 .. %d (order 1 is trcfile f or s, order 0 trcfile p)\n", argv[4], TRC_ORDER_MAX); return 2; }
        if (stride < 1 || stride > TRC_STRIDE_MAX) { fprintf(stderr, "stride %s: 1 .. %d\n", argv[5], TRC_STRIDE_MAX); return 2; }
        unsigned char *in = slurp(argv[6], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_oplanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = trc_encode_oplanes_host(codec, order, stride, in, n, esize, 0, out, cap, cdfnum);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[7], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, order %d, stride %d\n", n, l, 100.0 * l / n, esize, order, stride);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "O")) {
        const int id = atoi(argv[2]), codec = lib_codec(id), stride = atoi(argv[4]);
        const unsigned esize = (unsigned)atoi(argv[3]);
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (stride < 1 || stride > TRC_STRIDE_MAX) { fprintf(stderr, "stride %s: 1 .. %d\n", argv[4], TRC_STRIDE_MAX); return 2; }
        unsigned char *in = slurp(argv[5], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_oplanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        trc_planes_order_advice adv;
        const size_t l = trc_encode_aoplanes_host(codec, stride, in, n, esize, 0, out, cap, cdfnum, &adv);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[6], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, stride %d, order-0 estimate of orders 0 .. 3: %.0f %.0f %.0f %.0f bytes, choice order %d\n", n, l, 100.0 * l / n, esize,
               stride, adv.total_bits[0] / 8, adv.total_bits[1] / 8, adv.total_bits[2] / 8, adv.total_bits[3] / 8, adv.order);
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "r")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        const int filter = !strcmp(argv[4], "z") ? TRC_FILTER_ZDELTA : !strcmp(argv[4], "x") ? TRC_FILTER_XOR : TRC_FILTER_NONE;
        size_t n, bn;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (filter == TRC_FILTER_NONE) { fprintf(stderr, "filter %s: z (zigzag delta) or x (xor)\n", argv[4]); return 2; }
        unsigned char *base = slurp(argv[5], &bn), *in = base ? slurp(argv[6], &n) : 0;
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_bplanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        if (bn < n - n % esize) { fprintf(stderr, "the base holds %zu bytes, the elements of the input take %zu\n", bn, n - n % esize); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = trc_encode_bplanes_host(codec, filter, in, base, n, esize, 0, out, cap, cdfnum);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[7], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, filter %s against the base\n", n, l, 100.0 * l / n, esize, argv[4]);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "R")) {
        size_t fl, bn;
        unsigned char *fb = slurp(argv[2], &fl), *base = fb ? slurp(argv[3], &bn) : 0;
        if (!base) return 2;
        trc_planes_hdr ph;
        if (trc_bplanes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        memcpy(&ph, fb + sizeof(trc_bplanes_hdr), sizeof ph);
        unsigned char *out = malloc((size_t)ph.n + 1024);
        if (!out) { perror("malloc"); return 2; }
        if (trc_decode_bplanes_host(fb, fl, base, bn, out, (size_t)ph.n) != ph.n) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
        return write_file(argv[4], out, (size_t)ph.n);
    }
    if (argc == 6 && !strcmp(argv[1], "a")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        size_t n;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        unsigned char *in = slurp(argv[4], &n);
        if (!in) return 2;
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_fplanes_bound(n, esize, 0, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u with %zu bytes: esize is 2, 4 or 8 and the file holds at least one element\n", esize, n); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        trc_planes_advice adv;
        const size_t l = trc_encode_aplanes_host(codec, in, n, esize, 0, out, cap, cdfnum, &adv);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[5], out, l)) return 2;
        printf("%zu -> %zu bytes (%.2f%%)  %u planes, order-0 estimate n %.0f z %.0f x %.0f bytes, choice %c\n", n, l, 100.0 * l / n, esize,
               adv.total_bits[0] / 8, adv.total_bits[1] / 8, adv.total_bits[2] / 8, "nzx"[adv.filter]);
        return 0;
    }
    if (argc >= 8 && !strcmp(argv[1], "b")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        const uint32_t chunk = (uint32_t)strtoul(argv[4], 0, 10);
        const char *fl = argv[5];
        const size_t count = (size_t)(argc - 7);
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (strlen(fl) != 1 || !strchr("nzxao", fl[0])) { fprintf(stderr, "filter %s: n (none), z (zigzag delta), x (xor), a (the advisor, per item) or o (the order advisor at stride 1, per item)\n", fl); return 2; }
        trc_planes_item *items = calloc(count, sizeof *items);
        uint8_t *filters = calloc(count, 1), *orders = calloc(count, 1);
        if (!items || !filters || !orders) { perror("malloc"); return 2; }
        size_t total = 0;
        for (size_t i = 0; i < count; i++) {
            size_t n;
            if (!(items[i].d_ptr = slurp(argv[7 + i], &n))) return 2;
            items[i].n = n; total += n;
            filters[i] = fl[0] == 'z' ? TRC_FILTER_ZDELTA : fl[0] == 'x' ? TRC_FILTER_XOR : TRC_FILTER_NONE;
        }
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = fl[0] == 'o' ? trc_planes_obatch_bound(codec, items, count, esize, chunk, cdfnum) : trc_planes_batch_bound(codec, items, count, esize, chunk, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u, chunk %u: esize is 2, 4 or 8, the chunk 0 or a multiple of 64, and every file holds whole elements, at least one\n", esize, chunk); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = fl[0] == 'o' ? trc_encode_aoplanes_batch_host(codec, items, 0, count, esize, chunk, cdfnum, TRC_ITEMS_HOST, out, cap, filters, orders) :
                         fl[0] == 'a' ? trc_encode_aplanes_batch_host(codec, items, count, esize, chunk, cdfnum, TRC_ITEMS_HOST, out, cap, filters)
                                      : trc_encode_planes_batch_host(codec, items, filters, count, esize, chunk, cdfnum, TRC_ITEMS_HOST, out, cap);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[6], out, l)) return 2;
        if (fl[0] == 'a') for (size_t i = 0; i < count; i++) printf("item %zu: %llu bytes, choice %c  %s\n", i, (unsigned long long)items[i].n, "nzx"[filters[i]], argv[7 + i]);
        if (fl[0] == 'o') for (size_t i = 0; i < count; i++) printf("item %zu: %llu bytes, choice order %u  %s\n", i, (unsigned long long)items[i].n, filters[i] ? orders[i] : 0u, argv[7 + i]);
        printf("%zu items, %zu -> %zu bytes (%.2f%%)  %u planes\n", count, total, l, 100.0 * l / total, esize);
        return 0;
    }
    if (argc >= 9 && !((argc - 7) & 1) && !strcmp(argv[1], "e")) {
        const int id = atoi(argv[2]), codec = lib_codec(id);
        const unsigned esize = (unsigned)atoi(argv[3]);
        const uint32_t chunk = (uint32_t)strtoul(argv[4], 0, 10);
        const char *fl = argv[5];
        const size_t count = (size_t)(argc - 7) / 2;
        if (!codec) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        if (strlen(fl) != 1 || !strchr("zxa", fl[0])) { fprintf(stderr, "filter %s: z (zigzag delta), x (xor) or a (the advisor, per item)\n", fl); return 2; }
        trc_planes_item *items = calloc(count, sizeof *items);
        const void **bases = calloc(count, sizeof *bases);
        uint8_t *filters = calloc(count, 1);
        if (!items || !bases || !filters) { perror("malloc"); return 2; }
        size_t total = 0;
        for (size_t i = 0; i < count; i++) {
            size_t n, bn;
            if (!(items[i].d_ptr = slurp(argv[7 + 2 * i], &n))) return 2;
            items[i].n = n; total += n;
            if (strcmp(argv[8 + 2 * i], "-")) {
                if (!(bases[i] = slurp(argv[8 + 2 * i], &bn))) return 2;
                if (bn < n) { fprintf(stderr, "%s holds %zu bytes, its item %zu\n", argv[8 + 2 * i], bn, n); return 2; }
                filters[i] = fl[0] == 'z' ? TRC_FILTER_ZDELTA : TRC_FILTER_XOR;
            }
        }
        const unsigned cdfnum = (codec == TRC_ANS4S || codec == TRC_RCS1 || codec == TRC_RCS2 || codec == TRC_RCSM) ? 256u : 0u;
        const size_t cap = trc_planes_bbatch_bound(codec, items, count, esize, chunk, cdfnum);
        if (!cap) { fprintf(stderr, "esize %u, chunk %u: esize is 2, 4 or 8, the chunk 0 or a multiple of 64, and every file holds whole elements, at least one\n", esize, chunk); return 2; }
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        const size_t l = fl[0] == 'a' ? trc_encode_abplanes_batch_host(codec, items, bases, count, esize, chunk, cdfnum, TRC_ITEMS_HOST, out, cap, filters)
                                      : trc_encode_bplanes_batch_host(codec, items, bases, filters, count, esize, chunk, cdfnum, TRC_ITEMS_HOST, out, cap);
        if (!l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        if (write_file(argv[6], out, l)) return 2;
        if (fl[0] == 'a') for (size_t i = 0; i < count; i++) printf("item %zu: %llu bytes, choice %c  %s\n", i, (unsigned long long)items[i].n, "nzx"[filters[i]], argv[7 + 2 * i]);
        printf("%zu items, %zu -> %zu bytes (%.2f%%)  %u planes, %.4s\n", count, total, l, 100.0 * l / total, esize, (const char *)out);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "E")) {
        size_t fl, bn = 0;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        const int based = fl >= 4 && !memcmp(fb, "TRCE", 4);
        trc_planes_batch_hdr h;
        if (based ? trc_planes_bbatch_info(fb, fl, &h, 0, 0, 0, 0) : trc_planes_batch_info(fb, fl, &h, 0, 0, 0)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        const size_t count = (size_t)h.count, item = (size_t)strtoull(argv[3], 0, 10);
        if (item >= count) { fprintf(stderr, "item %zu of %zu\n", item, count); return 2; }
        uint64_t *n = calloc(count, sizeof *n);
        trc_planes_item *items = calloc(count, sizeof *items);
        const void **bases = calloc(count, sizeof *bases);
        if (!n || !items || !bases) { perror("malloc"); return 2; }
        if (based ? trc_planes_bbatch_info(fb, fl, &h, n, 0, 0, count) : trc_planes_batch_info(fb, fl, &h, n, 0, count)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        for (size_t i = 0; i < count; i++) items[i].n = n[i];
        unsigned char *out = malloc((size_t)n[item] + 1024);
        if (!out) { perror("malloc"); return 2; }
        items[item].d_ptr = out;
        if (strcmp(argv[4], "-")) {
            if (!(bases[item] = slurp(argv[4], &bn))) return 2;
            if (bn < n[item]) { fprintf(stderr, "%s holds %zu bytes, the item %llu\n", argv[4], bn, (unsigned long long)n[item]); return 2; }
        }
        if (trc_decode_bplanes_batch_host(fb, fl, items, bases, count, item, 1, TRC_ITEMS_HOST) != n[item]) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
        return write_file(argv[5], out, (size_t)n[item]);
    }
    if (argc == 3 && !strcmp(argv[1], "l")) {          /* a file of e: the TRCB listing with the bases' fingerprints */
        size_t fl;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        if (fl >= 4 && !memcmp(fb, "TRCE", 4)) {
            trc_planes_batch_hdr h;
            if (trc_planes_bbatch_info(fb, fl, &h, 0, 0, 0, 0)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            const size_t count = (size_t)h.count, lead = sizeof(trc_planes_bbatch_hdr) + ((8 * count + 15) & ~(size_t)15);
            uint64_t *n = calloc(count, sizeof *n), *fp = calloc(count, sizeof *fp);
            uint8_t *filters = calloc(count, 1);
            if (!n || !fp || !filters) { perror("malloc"); return 2; }
            if (trc_planes_bbatch_info(fb, fl, &h, n, filters, fp, count)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            trc_planes_hdr ph;
            memcpy(&ph, fb + lead + h.inner, sizeof ph);
            printf("%llu items, esize %u, chunk %u, codec %u, %llu -> %llu bytes, against bases\n", (unsigned long long)h.count, h.esize, h.chunk, ph.codec,
                   (unsigned long long)h.bytes, (unsigned long long)(lead + h.size));
            for (size_t i = 0; i < count; i++) {
                if (filters[i]) printf("item %zu: %llu bytes, filter %c, base %016llx\n", i, (unsigned long long)n[i], "nzx"[filters[i]], (unsigned long long)fp[i]);
                else printf("item %zu: %llu bytes, filter n\n", i, (unsigned long long)n[i]);
            }
            return 0;
        }
        free(fb);
    }
    if ((argc == 6 && !strcmp(argv[1], "B")) || (argc == 3 && !strcmp(argv[1], "l"))) {
        const int list = argv[1][0] == 'l';
        size_t fl;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        /* a TRCT file: the strides of the items, then the TRCB container (this tool reads it; it does not write one); a TRCU file: the
         * strides and the predictor orders of the items, then the TRCB container (b ... o writes one where an order above 1 is chosen) */
        const int strided = fl >= 4 && !memcmp(fb, "TRCT", 4), ordered = fl >= 4 && !memcmp(fb, "TRCU", 4);
        trc_planes_batch_hdr h;
        if (ordered ? trc_planes_obatch_info(fb, fl, &h, 0, 0, 0, 0, 0) : strided ? trc_planes_sbatch_info(fb, fl, &h, 0, 0, 0, 0) : trc_planes_batch_info(fb, fl, &h, 0, 0, 0)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        const size_t count = (size_t)h.count, lead = ordered ? sizeof(trc_planes_obatch_hdr) + 2 * ((count + 15) & ~(size_t)15) : strided ? sizeof(trc_planes_sbatch_hdr) + ((count + 15) & ~(size_t)15) : 0;
        uint64_t *n = calloc(count, sizeof *n);
        uint8_t *filters = calloc(count, 1), *strides = calloc(count, 1), *orders = calloc(count, 1);
        if (!n || !filters || !strides || !orders) { perror("malloc"); return 2; }
        if (ordered ? trc_planes_obatch_info(fb, fl, &h, n, filters, strides, orders, count) : strided ? trc_planes_sbatch_info(fb, fl, &h, n, filters, strides, count) : trc_planes_batch_info(fb, fl, &h, n, filters, count)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        if (list) {
            trc_planes_hdr ph;
            memcpy(&ph, fb + lead + h.inner, sizeof ph);
            printf("%llu items, esize %u, chunk %u, codec %u, %llu -> %llu bytes\n", (unsigned long long)h.count, h.esize, h.chunk, ph.codec,
                   (unsigned long long)h.bytes, (unsigned long long)(lead + h.size));
            for (size_t i = 0; i < count; i++) {
                if (ordered) printf("item %zu: %llu bytes, filter %c, stride %u, order %u\n", i, (unsigned long long)n[i], "nzx"[filters[i]], strides[i], orders[i]);
                else if (strided) printf("item %zu: %llu bytes, filter %c, stride %u\n", i, (unsigned long long)n[i], "nzx"[filters[i]], strides[i]);
                else printf("item %zu: %llu bytes, filter %c\n", i, (unsigned long long)n[i], "nzx"[filters[i]]);
            }
            return 0;
        }
        const size_t first = (size_t)strtoull(argv[3], 0, 10), cnt = (size_t)strtoull(argv[4], 0, 10);
        if (!cnt || first > count || cnt > count - first) { fprintf(stderr, "items [%zu, %zu + %zu) of %zu\n", first, first, cnt, count); return 2; }
        trc_planes_item *items = calloc(count, sizeof *items);
        if (!items) { perror("malloc"); return 2; }
        size_t bytes = 0;
        for (size_t i = first; i < first + cnt; i++) bytes += (size_t)n[i];
        unsigned char *out = malloc(bytes + 1024);
        if (!out) { perror("malloc"); return 2; }
        size_t pos = 0;
        for (size_t i = 0; i < count; i++) {
            items[i].n = n[i];
            if (i >= first && i < first + cnt) { items[i].d_ptr = out + pos; pos += (size_t)n[i]; }
        }
        if ((ordered ? trc_decode_oplanes_batch_host(fb, fl, items, count, first, cnt, TRC_ITEMS_HOST) :
             strided ? trc_decode_splanes_batch_host(fb, fl, items, count, first, cnt, TRC_ITEMS_HOST)
                     : trc_decode_planes_batch_host(fb, fl, items, count, first, cnt, TRC_ITEMS_HOST)) != bytes) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
        return write_file(argv[5], out, bytes);
    }
    if (argc == 4 && !strcmp(argv[1], "d")) {
        size_t fl;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        if (is_bplanes(fb, fl)) { fprintf(stderr, "a file of trcfile r, coded against a base: trcfile R <in> <base> <out> decodes it\n"); return 2; }
        /* a file of `trcfile p`, f, s or a: untrusted, so checked against what was read; the library looks at the magic itself
         * (trc_decode_xplanes_host = trc_decode_planes_host, trc_decode_fplanes_host or trc_decode_splanes_host) */
        if (is_fplanes(fb, fl) || is_splanes(fb, fl) || is_oplanes(fb, fl) || is_planes(fb, fl)) {
            const size_t lead = is_planes(fb, fl) ? 0 : sizeof(trc_fplanes_hdr);     /* (the TRCS and TRCO prefixes have the TRCF prefix's size) */
            trc_planes_hdr ph;
            if (is_oplanes(fb, fl) ? trc_oplanes_check(fb, fl, (size_t)-1) : is_splanes(fb, fl) ? trc_splanes_check(fb, fl, (size_t)-1) : lead ? trc_fplanes_check(fb, fl, (size_t)-1) : trc_planes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            memcpy(&ph, fb + lead, sizeof ph);
            unsigned char *out = malloc((size_t)ph.n + 1024);
            if (!out) { perror("malloc"); return 2; }
            if (trc_decode_xplanes_host(fb, fl, out, (size_t)ph.n) != ph.n) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
            return write_file(argv[3], out, (size_t)ph.n);
        }
        if (fl < 24 || memcmp(fb, "TRCF", 4)) { fprintf(stderr, "not a TRCF file\n"); return 2; }
        const int id = fb[4];
        const unsigned m = fb[5];
        uint64_t raw, stored;
        memcpy(&raw, fb + 8, 8); memcpy(&stored, fb + 16, 8);
        const int ss = id >= 128 && pick_ss(id & 127);                   /* an "ss" coder: the parameters are in the container's header */
        if (ss) { e3 = d3 = 0; e5 = d5 = 0; }
        else if (pick(id, &e3, &d3, &e5, &d5)) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        size_t pos = 24;
        cdf_t cdf[257];
        if (d5) {
            if (pos + (m + 2) * sizeof(cdf_t) > fl) { fprintf(stderr, "truncated file\n"); return 2; }
            memcpy(cdf, fb + pos, (m + 2) * sizeof(cdf_t)); pos += (m + 2) * sizeof(cdf_t);
        }
        if (stored > fl - pos || stored != fl - pos || stored > raw) { fprintf(stderr, "truncated or padded file\n"); return 2; }
        /* untrusted input: the decoders take no input length, so the container is validated against what was read */
        if (stored != raw && trc_container_check(fb + pos, (size_t)stored, 0, (size_t)raw)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
        unsigned char *out = malloc(raw + 1024);
        if (!out) { perror("malloc"); return 2; }
        if (stored == raw) memcpy(out, fb + pos, raw);                    /* stored: the caller copies (CCPY) */
        else if ((ss ? trc_decode_host(id & 127, fb + pos, (size_t)stored, out, (size_t)raw, 0, 0) : d3 ? d3(fb + pos, raw, out) : d5(fb + pos, raw, out, cdf, m + 1)) != raw) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
        FILE *f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 2; }
        fwrite(out, 1, raw, f);
        fclose(f);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "x")) {
        size_t fl;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        if (is_bplanes(fb, fl)) { fprintf(stderr, "a file of trcfile r, coded against a base: trcfile R <in> <base> <out> decodes it\n"); return 2; }
        if (is_splanes(fb, fl)) {
            const uint64_t off = strtoull(argv[3], 0, 10), len = strtoull(argv[4], 0, 10);
            trc_planes_hdr ph;
            if (trc_splanes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            memcpy(&ph, fb + sizeof(trc_splanes_hdr), sizeof ph);
            if (!len || off > ph.n || len > ph.n - off) { fprintf(stderr, "range outside the file's %llu bytes\n", (unsigned long long)ph.n); return 2; }
            unsigned char *out = malloc((size_t)len + 1024);
            if (!out) { perror("malloc"); return 2; }
            if (trc_decode_splanes_range_host(fb, fl, (size_t)off, (size_t)len, out) != len) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
            return write_file(argv[5], out, (size_t)len);
        }
        if (is_oplanes(fb, fl)) {
            const uint64_t off = strtoull(argv[3], 0, 10), len = strtoull(argv[4], 0, 10);
            trc_planes_hdr ph;
            if (trc_oplanes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            memcpy(&ph, fb + sizeof(trc_oplanes_hdr), sizeof ph);
            if (!len || off > ph.n || len > ph.n - off) { fprintf(stderr, "range outside the file's %llu bytes\n", (unsigned long long)ph.n); return 2; }
            unsigned char *out = malloc((size_t)len + 1024);
            if (!out) { perror("malloc"); return 2; }
            if (trc_decode_oplanes_range_host(fb, fl, (size_t)off, (size_t)len, out) != len) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
            return write_file(argv[5], out, (size_t)len);
        }
        if (is_fplanes(fb, fl)) {
            const uint64_t off = strtoull(argv[3], 0, 10), len = strtoull(argv[4], 0, 10);
            trc_planes_hdr ph;
            if (trc_fplanes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            memcpy(&ph, fb + sizeof(trc_fplanes_hdr), sizeof ph);
            if (!len || off > ph.n || len > ph.n - off) { fprintf(stderr, "range outside the file's %llu bytes\n", (unsigned long long)ph.n); return 2; }
            unsigned char *out = malloc((size_t)len + 1024);
            if (!out) { perror("malloc"); return 2; }
            if (trc_decode_fplanes_range_host(fb, fl, (size_t)off, (size_t)len, out) != len) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
            return write_file(argv[5], out, (size_t)len);
        }
        if (is_planes(fb, fl)) {
            const uint64_t off = strtoull(argv[3], 0, 10), len = strtoull(argv[4], 0, 10);
            trc_planes_hdr ph;
            if (trc_planes_check(fb, fl, (size_t)-1)) { fprintf(stderr, "corrupt file: %s\n", trc_last_error()); return 2; }
            memcpy(&ph, fb, sizeof ph);
            if (!len || off > ph.n || len > ph.n - off) { fprintf(stderr, "range outside the file's %llu bytes\n", (unsigned long long)ph.n); return 2; }
            unsigned char *out = malloc((size_t)len + 1024);
            if (!out) { perror("malloc"); return 2; }
            if (trc_decode_planes_range_host(fb, fl, (size_t)off, (size_t)len, out) != len) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
            return write_file(argv[5], out, (size_t)len);
        }
        if (fl < 24 || memcmp(fb, "TRCF", 4)) { fprintf(stderr, "not a TRCF file\n"); return 2; }
        const int id = fb[4];
        const unsigned m = fb[5];
        const uint64_t off = strtoull(argv[3], 0, 10), len = strtoull(argv[4], 0, 10);
        uint64_t raw, stored;
        memcpy(&raw, fb + 8, 8); memcpy(&stored, fb + 16, 8);
        if (id >= 128 && pick_ss(id & 127)) { e3 = d3 = 0; e5 = d5 = 0; }       /* an "ss" coder: no CDF, cdfnum 0 = the header's parameters */
        else if (pick(id, &e3, &d3, &e5, &d5)) { fprintf(stderr, "unknown id %d\n", id); return 2; }
        size_t pos = 24;
        cdf_t cdf[257];
        if (d5) {
            if (pos + (m + 2) * sizeof(cdf_t) > fl) { fprintf(stderr, "truncated file\n"); return 2; }
            memcpy(cdf, fb + pos, (m + 2) * sizeof(cdf_t)); pos += (m + 2) * sizeof(cdf_t);
        }
        if (stored != fl - pos || stored > raw) { fprintf(stderr, "truncated or padded file\n"); return 2; }
        if (!len || off > raw || len > raw - off) { fprintf(stderr, "range outside the file's %llu bytes\n", (unsigned long long)raw); return 2; }
        unsigned char *out = malloc(len + 1024);
        if (!out) { perror("malloc"); return 2; }
        if (stored == raw) memcpy(out, fb + pos + off, len);              /* stored: no container, the bytes are there */
        else {
            /* the file names the reference's id, the container the library's: taken from its header, which the call validates
             * against what was read (untrusted input) */
            trc_container_hdr h;
            if (stored < sizeof h) { fprintf(stderr, "corrupt file\n"); return 2; }
            memcpy(&h, fb + pos, sizeof h);
            if (trc_decode_range_host(h.codec, fb + pos, (size_t)stored, (size_t)raw, (size_t)off, (size_t)len, out, d5 ? cdf : 0, d5 ? m + 1 : 0) != len) {
                fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1;
            }
        }
        FILE *f = fopen(argv[5], "wb");
        if (!f) { perror(argv[5]); return 2; }
        fwrite(out, 1, len, f);
        fclose(f);
        return 0;
    }
    /* ---- the REFERENCE's own file format (hd_t / hdb_t, turborc.c:666-733; block loop :1044-1167) for file codec 1 with
     * the "s" predictor (`turborc -1 -b<bsize>B in out`): header u32 = codec << 12 | 0x154 (| bsize << 20 if bsize < 4096)
     * [u32 bsize] u16 = lev << 10 | prm2 << 6 | prm1 << 2 | (prdid - 1); per block u32 = clen << 2 | big << 1 | last
     * [u16 clen >> 30] [u32 inlen if last] then clen bytes = rcsenc(block), or the block itself when clen == inlen.
     * A block of the reference IS a chunk here when bsize is a legal chunk size (multiple of 64 in [256, 65536]): the
     * per-chunk payload equals rcsenc(block) bit for bit, so files written by `trcfile C` are read by the reference's
     * `turborc -d`, and `trcfile D` reads what `turborc -1 -b65536B` wrote -- every block of the file coded or decoded by
     * one launch. */
    if ((argc >= 4 && argc <= 6) && !strcmp(argv[1], "C")) {
        const unsigned bsize = argc >= 5 ? (unsigned)strtoul(argv[4], 0, 10) : 65536u;
        const unsigned fc = argc == 6 ? (unsigned)strtoul(argv[5], 0, 10) : 1u;
        fn3 dec;
        const int codec = file_codec(fc, &dec);
        if (!codec) { fprintf(stderr, "file codec %u: only 1 (rcs), 2 (rccs) and 4 (rcxs) are on the GPU path\n", fc); return 2; }
        size_t n;
        if (trc_set_chunk(bsize)) { fprintf(stderr, "block size must be a legal chunk size: %s\n", trc_last_error()); return 2; }
        unsigned char *in = slurp(argv[2], &n);
        if (!in) return 2;
        const size_t cap = trc_container_bound(n, bsize) + 1024;
        unsigned char *out = malloc(cap);
        if (!out) { perror("malloc"); return 2; }
        /* the container is wanted whatever its size: a 70-byte file is one coded block of 60 bytes for the reference, while
         * the reference-named call would hand back "raw" because 32 + 4 + 60 > 70 */
        size_t l = n ? trc_encode_host(codec, in, n, bsize, out, cap, 0, 0) : 0;
        if (n && !l) { fprintf(stderr, "encode failed: %s\n", trc_last_error()); return 1; }
        l = n + 1;                                             /* (never the "whole call raw" case below) */
        FILE *f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 2; }
        const uint32_t u32 = fc << 12 | 0x154u | (bsize < 4096u ? bsize << 20 : 0u);
        const uint16_t u16 = 8u << 10 | 6u << 6 | 5u << 2 | 0u;      /* lev 8, prm2 6, prm1 5 (the reference's defaults), predictor "s" */
        fwrite(&u32, 4, 1, f);
        if (bsize >= 4096u) fwrite(&bsize, 4, 1, f);
        fwrite(&u16, 2, 1, f);
        const size_t nblk = (n + bsize - 1) / bsize;
        const unsigned char *dir = out + 32, *pay = out + 32 + 4 * nblk;   /* TRC1 container: hdr | clen[] | payloads */
        for (size_t b = 0; b < nblk; b++) {
            const uint32_t inlen = (uint32_t)(n - b * bsize < bsize ? n - b * bsize : bsize);
            uint32_t clen = inlen;
            if (l != n) memcpy(&clen, dir + 4 * b, 4);
            const uint32_t h = clen << 2 | (inlen < bsize);
            fwrite(&h, 4, 1, f);
            if (inlen < bsize) fwrite(&inlen, 4, 1, f);
            if (l != n) { fwrite(pay, 1, clen, f); pay += clen; }
            else fwrite(in + b * bsize, 1, inlen, f);          /* the whole call came back raw: stored blocks */
        }
        fclose(f);
        printf("%zu bytes -> reference-format file, %zu blocks of %u\n", n, nblk, bsize);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "D")) {
        size_t fl;
        unsigned char *fb = slurp(argv[2], &fl);
        if (!fb) return 2;
        if (fl < 6) { fprintf(stderr, "not a TurboRC file\n"); return 2; }
        uint32_t u32; memcpy(&u32, fb, 4);
        size_t pos = 4;
        fn3 dec;
        const int codec = file_codec((u32 >> 12) & 0xffu, &dec);
        if ((u32 & 0xfffu) != 0x154u || !codec) { fprintf(stderr, "not a TurboRC file of codec 1, 2 or 4\n"); return 2; }
        uint32_t bsize = u32 >> 20;
        if (!bsize) { if (fl < 10) return 2; memcpy(&bsize, fb + 4, 4); pos = 8; }
        uint16_t u16; memcpy(&u16, fb + pos, 2); pos += 2;
        if ((u16 & 3u) != 0u) { fprintf(stderr, "predictor %u: only \"s\" (rcsenc) is on the GPU path\n", (u16 & 3u) + 1u); return 2; }
        if (trc_set_chunk(bsize)) { fprintf(stderr, "block size %u is not a legal chunk size (write with -b65536B or smaller multiples of 64)\n", bsize); return 2; }
        /* pass 1: walk the blocks, collect the directory */
        size_t nblk = 0, n = 0, paybytes = 0, p = pos;
        int allraw = 1;
        while (p + 4 <= fl) {
            uint32_t h; memcpy(&h, fb + p, 4); p += 4;
            if (h & 2u) { fprintf(stderr, "blocks above 1 GB are not supported\n"); return 2; }
            uint32_t inlen = bsize;
            if (h & 1u) { if (p + 4 > fl) { fprintf(stderr, "truncated file\n"); return 2; } memcpy(&inlen, fb + p, 4); p += 4; }
            const uint32_t clen = h >> 2;
            if (clen > fl - p || inlen > bsize || clen > inlen) { fprintf(stderr, "corrupt block header\n"); return 2; }
            if (clen != inlen) allraw = 0;
            p += clen; paybytes += clen; n += inlen; nblk++;
            if (inlen < bsize) break;
        }
        unsigned char *cont = malloc(32 + 4 * nblk + paybytes + 1024), *out = malloc(n + 1024);
        if (!cont || !out) { perror("malloc"); return 2; }
        trc_container_hdr hdr; memset(&hdr, 0, sizeof hdr);
        hdr.magic = TRC_MAGIC; hdr.codec = (uint8_t)codec; hdr.version = 1; hdr.chunk = bsize; hdr.nchunks = (uint32_t)nblk; hdr.n = n; hdr.payload = paybytes;
        memcpy(cont, &hdr, 32);
        unsigned char *dirp = cont + 32, *payp = cont + 32 + 4 * nblk;
        p = pos;
        for (size_t b = 0; b < nblk; b++) {
            uint32_t h; memcpy(&h, fb + p, 4); p += 4;
            if (h & 1u) p += 4;
            const uint32_t clen = h >> 2;
            memcpy(dirp + 4 * b, &clen, 4);
            memcpy(payp, fb + p, clen); payp += clen; p += clen;
        }
        if (n) {
            if (allraw) memcpy(out, cont + 32 + 4 * nblk, n);                 /* nothing coded: stored blocks */
            else if (trc_container_check(cont, 32 + 4 * nblk + paybytes, codec, n) || dec(cont, n, out) != n) { fprintf(stderr, "decode failed: %s\n", trc_last_error()); return 1; }
        }
        FILE *f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 2; }
        fwrite(out, 1, n, f);
        fclose(f);
        return 0;
    }
    fprintf(stderr, "usage: trcfile c <id> <in> <out> [-r NM] | trcfile p <id> <esize> <in> <out> | trcfile f <id> <esize> <z|x> <in> <out> | trcfile s <id> <esize> <z|x> <stride> <in> <out> | trcfile o <id> <esize> <order> <stride> <in> <out> | trcfile O <id> <esize> <stride> <in> <out> | trcfile a <id> <esize> <in> <out> | trcfile d <in> <out> | trcfile x <in> <offset> <len> <out> | trcfile C <in> <out> [bsize [1|2|4]] | trcfile D <in> <out>   (C/D: the reference's file format, codecs 1, 2, 4) | trcfile b <id> <esize> <chunk|0> <n|z|x|a> <out> <in>... (or o: the order advisor per item) | trcfile B <in> <first> <count> <out> | trcfile l <in> | trcfile r <id> <esize> <z|x> <base> <in> <out> | trcfile R <in> <base> <out> | trcfile e <id> <esize> <chunk|0> <z|x|a> <out> <in> <base|-> ... | trcfile E <in> <item> <base|-> <out>\n");
    return 2;
}
