// cavity_mode_kernel, in a header of its own: it is no template, so every unit that includes its definition emits it, and
// only the unit that launches it (cavmd_observables.hip) may.  cavmd_observable_kernels.hpp, which the batch kernels include
// for its device functions, keeps HostMode.
#pragma once

#include "cavmd_observable_kernels.hpp"

namespace cavmd
{
// Cavity-mode kinetic energy (reference: CavityModeTracker.compute_cavity_properties, src/cavitymd/analysis.py:1324-1368):
// KE = 1/2 m v.v of the photon found by the last force evaluation; HOOMD keeps the mass in vel.w.
// out[0..3] = KE, harmonic PE (from the result block), KE + PE, temperature = (2/3) KE / k_B.
// The four numbers reach the host through mapped pinned memory: values first, then the call's sequence number
// (system-scope release) that cavmd_cavity_mode spins on -- no copy, no stream synchronisation.
__global__ void cavity_mode_kernel(const cavmd_result* __restrict__ res, const cavmd_double4* __restrict__ vel, double kB,
                                   double* __restrict__ out, HostMode* __restrict__ host, uint64_t sequence)
{
    const int p = res->photon_idx;
    double ke = 0.0, pe = 0.0, tot = 0.0, temp = 0.0;
    if (p >= 0)
    {
        const cavmd_double4 v = vel[p];
        ke = 0.5 * v.w * ((v.x * v.x + v.y * v.y) + v.z * v.z);
        pe = res->energy[0];
        tot = ke + pe;
        temp = (2.0 / 3.0) * ke / kB;
    }
    out[0] = ke;
    out[1] = pe;
    out[2] = tot;
    out[3] = temp;
    host->v[0] = ke;
    host->v[1] = pe;
    host->v[2] = tot;
    host->v[3] = temp;
    __hip_atomic_store(&host->ready, sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
} // namespace cavmd
