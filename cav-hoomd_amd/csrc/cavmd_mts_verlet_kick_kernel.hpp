// cavmd_mts_verlet_kick_kernel.hpp -- cavmd_mts_verlet_kick of include/cavmd.h: a kick of a batch's velocities with a force
// that is none of the integrator's own arrays, in ONE launch, one workgroup per system: the outer half-kicks of the impulse
// multiple-time-step scheme (Verlet-I / r-RESPA) around n plain steps of cavmd_verlet_batch_kernel.hpp, with the LONG part of
// a split Coulomb batch (cavmd_coulomb_batch_kernel.hpp) as the force.
//
// The reference has no such step: its driver adds the two Coulomb forces to one HOOMD integrator.  include/cavmd.h carries the
// expressions as the contract, per particle and component:
//   h = weight * dt;  minv = 1.0 / m;  v_c = v_c + (f_c * minv) * h
// Every operation is one IEEE rounding (no FMA).  It is a kernel of its own, with its own text, so that the two step kernels
// and the bath kernel keep their device code; rows, order, input rows, tiles and the stores of v are step two's
// (verlet_step_two_kernel), which this restates.  The table of force pointers, the input row and the item's row are read when
// the kernel runs, so a captured launch follows all three.  Only vel.x, vel.y and vel.z are written.
#pragma once

#include "cavmd_verlet_batch_kernel.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void verlet_kick_kernel(const VerletRow* __restrict__ rows, const unsigned* __restrict__ order,
                                                            const VerletInput* __restrict__ inputs,
                                                            const v2d* const* __restrict__ forces, double weight)
{
    constexpr int UNROLL = kVerletUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const VerletRow* __restrict__ row = rows + item;
    const VerletInput* __restrict__ in = inputs + item;
    const unsigned n = row->n;
    const v2d* __restrict__ f = forces[item];
    if (n == 0 || in->skip != 0 || !f)
        return; // nothing of the item is read or written
    v2d* __restrict__ vel2 = row->vel2;
    const double h = weight * in->dt;
    const unsigned tiles = (n + TILE - 1) / TILE;

    for (unsigned t = 0; t < tiles; ++t)
    {
        // all of the tile's loads first: 2 x 16 B of vel and of the force per particle
        v2d vxy[UNROLL], vzw[UNROLL], fxy[UNROLL], fzw[UNROLL];
        const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            if (j < n)
            {
                vxy[u] = vel2[2 * (size_t)j];
                vzw[u] = vel2[2 * (size_t)j + 1];
                fxy[u] = f[2 * (size_t)j];
                fzw[u] = f[2 * (size_t)j + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            if (j >= n)
                continue;
            const double minv = 1.0 / vzw[u].y;
            vxy[u].x = vxy[u].x + (fxy[u].x * minv) * h;
            vxy[u].y = vxy[u].y + (fxy[u].y * minv) * h;
            const double vz = vzw[u].x + (fzw[u].x * minv) * h;
            vel2[2 * (size_t)j] = vxy[u];
            reinterpret_cast<double*>(vel2)[4 * (size_t)j + 2] = vz; // vel.w is never written
        }
    }
}
} // namespace cavmd
