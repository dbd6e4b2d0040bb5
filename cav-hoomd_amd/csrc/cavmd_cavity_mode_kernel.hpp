// cavity_mode_kernel, in a header of its own: it is no template, so every unit that includes its definition emits it, and
// only the unit that launches it (cavmd_observables.hip) may.  cavmd_observable_kernels.hpp, which the batch kernels include
// for its device functions, keeps HostMode.
#pragma once

#include "cavmd_observable_kernels.hpp"

namespace cavmd
{
// cavity_mode_numbers of the photon found by the last force evaluation (HOOMD keeps the mass in vel.w), zeros without one.
// The four numbers reach the host through mapped pinned memory: values first, then the call's sequence number
// (system-scope release) that cavmd_cavity_mode spins on -- no copy, no stream synchronisation.
__global__ void cavity_mode_kernel(const cavmd_result* __restrict__ res, const cavmd_double4* __restrict__ vel, double kB,
                                   double* __restrict__ out, HostMode* __restrict__ host, uint64_t sequence)
{
    const int p = res->photon_idx;
    double mode[4] = {0.0, 0.0, 0.0, 0.0};
    if (p >= 0)
    {
        const cavmd_double4 v = vel[p];
        cavity_mode_numbers(v.w, v.x, v.y, v.z, res->energy[0], kB, mode);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        out[k] = mode[k];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        host->v[k] = mode[k];
    __hip_atomic_store(&host->ready, sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
} // namespace cavmd
