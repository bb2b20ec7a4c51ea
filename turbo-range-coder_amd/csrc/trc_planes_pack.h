// trc_planes_pack.h -- what trc_planes_container.inc (host side, in trc_api.hip) hands to the pack kernel of trc_planes_pack.hip
#ifndef TRC_PLANES_PACK_H
#define TRC_PLANES_PACK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

struct PackArgs {
    uint8_t *out;                  // the TRCB container's start, 16-byte aligned; its front [0, inner) is there already
    uint64_t inner;                // offset of the inner TRCP container, a multiple of 8
    const uint32_t *clen;          // plane k's directory at clen + k * NC
    const uint8_t *payload;        // plane k's payload at payload + k * pitch, 256-byte aligned
    const uint64_t *total;         // plane k's payload bytes
    const uint16_t *cdf;           // static coders: plane k's CDF at cdf + k * TRC_PLANES_CDF_STRIDE; else NULL
    const int32_t *status;         // static coders: the planes' cdfini statuses; else NULL
    uint64_t *d_size;
    uint64_t M, NC, pitch;
    uint32_t esize;
    uint32_t cdfb;                 // bytes of a section's CDF: up8(2 (cdfnum + 1)), 0 where the coder has none
    uint32_t cdf_used;             // ... of which the CDF's own: 2 (cdfnum + 1)
    uint64_t ph[4];                // the inner trc_planes_hdr, its size (word 3) open
    uint64_t sh[4];                // a section's trc_container_hdr, its payload (word 3) open
};

int trc_planes_pack_launch(const PackArgs &a, hipStream_t s);
int trc_planes_pack_lead_launch(uint64_t *d_size, uint64_t lead, hipStream_t s);       // *d_size += lead where it is not 0

#endif
