// trc_planes_pack_lead.hip -- the size of a TRCT container (include/trc_hip.h): the TRCB container that trc_planes_pack.hip packs lies
// behind a prefix of strides.  A file of its own, so that the pack kernel's translation unit -- and with it its code -- stays as it is.
#include "trc_planes_vec.h"
#include "trc_planes_pack.h"

// behind the pack kernel on the same stream, for a container that lies `lead` bytes into a larger one (the strides in front of a
// TRCT container): the size the caller reads is the whole one; 0 (no container) stays 0.  One thread: the pack kernel stays as it is.
__global__ void trc_planes_pack_lead_kernel(uint64_t *d_size, uint64_t lead)
{
    if (*d_size) *d_size += lead;
}

int trc_planes_pack_lead_launch(uint64_t *d_size, uint64_t lead, hipStream_t s)
{
    hipLaunchKernelGGL(trc_planes_pack_lead_kernel, dim3(1), dim3(1), 0, s, d_size, lead);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRC_OK : trc_fail(TRC_E_HIP, "planes_sbatch_pack: %s", hipGetErrorString(e));
}
