// cavmd_bath_kernel.hpp -- the second half-step of velocity Verlet with a Langevin bath on ANY set of particles of every system
// of a batch, in ONE launch, one workgroup per system: verlet_step_two_kernel of cavmd_verlet_batch_kernel.hpp with the 3 N
// variates of the bath drawn where they are used.
//
// The reference's driver offers `--molecular-bath langevin` (examples/05_advanced_run.py:649-666): HOOMD-blue's Langevin method
// on every molecular particle, with tally_reservoir_energy=True.  include/cavmd.h ("a Langevin bath on any set of particles")
// carries the contract; in short, per item and particle j that is not the row's Langevin particle, with j < bath N and
// gamma_j > 0 (anything else, NaN included, is not coupled):
//   generator  Philox4x32-10 (draw_philox of cavmd_draw_kernel.hpp), key = the item's seed, counter = (draws low, draws high, j,
//              0x80000000 + b), b = 0, 1; `draws` is the item's counter in DEVICE memory, read when the kernel runs
//   variates   u_x from w0,w1 and u_y from w2,w3 of block 0, u_z from w0,w1 of block 1, each 2 * (k * 2^-53) - 1
//   bath       coeff_j = sqrt(((6 gamma_j) kT) / dt);  bd_c = u_c coeff_j - gamma_j v_c (v from BEFORE the kick);  F_c += bd_c;
//              tally_j = (bd_x v'_x + bd_y v'_y) + bd_z v'_z, v' being the velocity the kernel stores (AFTER the kick): the
//              work the bath does on the particle over the half-step, whose mean is 0 at the bath's temperature
//   per item   coupled = their number;  T = the double-double sum of the tallies in an order fixed by N (lane-serial over the
//              tiles, then block_tally of cavmd_reduce.hpp: a shuffle tree over the wave, the four waves in wave order), rounded
//              once;  reservoir -= T dt;  draws += 1
// Everything else is verlet_step_two_kernel's, expression for expression, the bath of the row's one Langevin particle included.
// It RESTATES that kernel's tile loop, and the counter layout of DrawStream::block (cavmd_draw_kernel.hpp): as one function for
// both kernels, and with the blocks drawn through DrawStream, the captured step missed the timing bound against the parent
// (profiles/shared_step_two/README.md), so tests/test_gpu_bath_batch.py still holds the two texts together byte for byte.
// The variates never touch memory.  Philox, the division and the square root run on coupled lanes only.
//
// `draws` is read by every wave and written back by one thread of the same workgroup: every use of the value read lies in the
// tile loop, BEFORE the workgroup barrier of the tally reduction, and the store comes AFTER that barrier.  Workgroups never wait
// for each other; every loop is bounded by N; no atomics, nothing mapped; the states are written with plain vector stores.
#pragma once

#include "cavmd_draw_kernel.hpp"
#include "cavmd_reduce.hpp"
#include "cavmd_verlet_batch_kernel.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
// Particles per lane and tile.  Two, as kVerletUnroll has it, cost 140 VGPRs, 2 spilled SGPRs and 3 waves per SIMD with four force
// arrays, gamma and Philox in flight; one is 87 VGPRs, no spill, 5 waves, and measured no slower (profiles/bath_batch/README.md).
constexpr int kBathUnroll = 1;
constexpr unsigned kBathPurpose = 0x80000000u;    // + b: the fourth counter word; cavmd_draw's purposes are all below 48

// One item's bath as the kernel reads it: the layout of cavmd_bath_item (the table is uploaded as it is).
struct BathRow
{
    const double* gamma;
    uint64_t seed;
    double kT;
    unsigned n;
    unsigned pad0;
    uint64_t pad[4];
};
static_assert(sizeof(BathRow) == 64, "one bath row = 64 bytes");

// Per-item counters in device memory (the layout of cavmd_bath_state).
struct BathState
{
    uint64_t draws;
    uint64_t coupled;
    double reservoir;
    double pad;
};
static_assert(sizeof(BathState) == 32, "one bath state = 32 bytes");

// blockIdx.x -> order[blockIdx.x] (the INTEGRATOR's order: items by N descending) -> the integrator's row and the bath's row,
// both fetched once per workgroup with scalar loads.  States are indexed by ITEM, never by block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void verlet_step_two_bath_kernel(const VerletRow* __restrict__ rows,
                                                                     const unsigned* __restrict__ order,
                                                                     const VerletInput* __restrict__ inputs,
                                                                     VerletState* __restrict__ state_all,
                                                                     const BathRow* __restrict__ bath_rows,
                                                                     BathState* __restrict__ bath_state_all)
{
    constexpr int UNROLL = kBathUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const VerletRow* __restrict__ row = rows + item;
    const unsigned n = row->n;
    if (n == 0)
        return;
    const VerletInput* __restrict__ in = inputs + item;
    if (in->skip != 0)
        return;
    const double dt = in->dt;
    const double gamma = in->gamma;
    const double coeff = in->coeff;
    const double ux = in->uniform[0];
    const double uy = in->uniform[1];
    const double uz = in->uniform[2];
    const int langevin = (gamma != 0.0) ? row->langevin : -1;
    const BathRow* __restrict__ bath = bath_rows + item;
    const double* __restrict__ gam = bath->gamma; // NULL: no bath on this item, none of its bath state is read or written
    const unsigned bath_n = gam ? (bath->n < n ? bath->n : n) : 0u;
    const double kT = bath->kT;
    const uint2 key = make_uint2((unsigned)bath->seed, (unsigned)(bath->seed >> 32));
    const uint64_t draws = gam ? bath_state_all[item].draws : 0;
    v2d* __restrict__ vel2 = row->vel2;
    double* __restrict__ accel = row->accel;
    v2d* __restrict__ net2 = row->net2;
    const v2d* __restrict__ f0 = row->force2[0];
    const v2d* __restrict__ f1 = row->force2[1];
    const v2d* __restrict__ f2 = f1 ? row->force2[2] : nullptr; // the list ends at the first NULL
    const v2d* __restrict__ f3 = f2 ? row->force2[3] : nullptr;
    const unsigned tiles = (n + TILE - 1) / TILE;

    double t_hi = 0.0, t_lo = 0.0; // this lane's tallies, double-double
    unsigned coupled = 0;
    for (unsigned t = 0; t < tiles; ++t)
    {
        // all of the tile's loads first: 2 x 16 B of vel and of every force array, 8 B of gamma per particle
        v2d vxy[UNROLL], vzw[UNROLL], axy[UNROLL], azw[UNROLL], bxy[UNROLL], bzw[UNROLL], cxy[UNROLL], czw[UNROLL], dxy[UNROLL],
            dzw[UNROLL];
        double g[UNROLL];
        const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            g[u] = 0.0;
            if (j < n)
            {
                vxy[u] = vel2[2 * (size_t)j];
                vzw[u] = vel2[2 * (size_t)j + 1];
                axy[u] = f0[2 * (size_t)j];
                azw[u] = f0[2 * (size_t)j + 1];
                if (f1)
                {
                    bxy[u] = f1[2 * (size_t)j];
                    bzw[u] = f1[2 * (size_t)j + 1];
                }
                if (f2)
                {
                    cxy[u] = f2[2 * (size_t)j];
                    czw[u] = f2[2 * (size_t)j + 1];
                }
                if (f3)
                {
                    dxy[u] = f3[2 * (size_t)j];
                    dzw[u] = f3[2 * (size_t)j + 1];
                }
                if (j < bath_n) // d_gamma is read below min(bath N, N) only
                    g[u] = gam[j];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            if (j >= n)
                continue;
            const double minv = 1.0 / vzw[u].y;
            v2d Fxy = axy[u], Fzw = azw[u]; // left to right over the arrays present, .w (the per-particle energy) as well
            if (f1)
            {
                Fxy = Fxy + bxy[u];
                Fzw = Fzw + bzw[u];
            }
            if (f2)
            {
                Fxy = Fxy + cxy[u];
                Fzw = Fzw + czw[u];
            }
            if (f3)
            {
                Fxy = Fxy + dxy[u];
                Fzw = Fzw + dzw[u];
            }
            if (net2) // without any bath term
            {
                net2[2 * (size_t)j] = Fxy;
                net2[2 * (size_t)j + 1] = Fzw;
            }
            double Fx = Fxy.x, Fy = Fxy.y, Fz = Fzw.x;
            double bdx = 0.0, bdy = 0.0, bdz = 0.0;
            const bool of_row = (int)j == langevin;
            const bool of_group = !of_row && g[u] > 0.0; // NaN, 0, negative, beyond bath N: not coupled
            if (of_row)
            {
                // the row's bath of the one cavity particle, as verlet_step_two_kernel has it; it wins over the group's
                bdx = ux * coeff - gamma * vxy[u].x;
                bdy = uy * coeff - gamma * vxy[u].y;
                bdz = uz * coeff - gamma * vzw[u].x;
            }
            else if (of_group)
            {
                const double gj = g[u];
                // the counter layout restates DrawStream::block (see above)
                const uint4 w0 = draw_philox(make_uint4((unsigned)draws, (unsigned)(draws >> 32), j, kBathPurpose), key);
                const uint4 w1 = draw_philox(make_uint4((unsigned)draws, (unsigned)(draws >> 32), j, kBathPurpose + 1u), key);
                const double cj = sqrt(((6.0 * gj) * kT) / dt);
                // the force from the velocity BEFORE the kick
                bdx = (2.0 * draw_unit(w0.x, w0.y) - 1.0) * cj - gj * vxy[u].x;
                bdy = (2.0 * draw_unit(w0.z, w0.w) - 1.0) * cj - gj * vxy[u].y;
                bdz = (2.0 * draw_unit(w1.x, w1.y) - 1.0) * cj - gj * vzw[u].x;
            }
            if (of_row || of_group)
            {
                Fx = Fx + bdx;
                Fy = Fy + bdy;
                Fz = Fz + bdz;
            }
            const double ax = Fx * minv, ay = Fy * minv, az = Fz * minv;
            accel[3 * (size_t)j] = ax;
            accel[3 * (size_t)j + 1] = ay;
            accel[3 * (size_t)j + 2] = az;
            vxy[u].x = vxy[u].x + (0.5 * ax) * dt;
            vxy[u].y = vxy[u].y + (0.5 * ay) * dt;
            const double vz = vzw[u].x + (0.5 * az) * dt;
            vel2[2 * (size_t)j] = vxy[u];
            reinterpret_cast<double*>(vel2)[4 * (size_t)j + 2] = vz; // vel.w is never written
            // the tallies, with the velocity just stored (AFTER the kick)
            if (of_row)
            {
                const double tally = (bdx * vxy[u].x + bdy * vxy[u].y) + bdz * vz;
                state_all[item].reservoir = state_all[item].reservoir - tally * dt;
            }
            else if (of_group)
            {
                dd_acc(t_hi, t_lo, (bdx * vxy[u].x + bdy * vxy[u].y) + bdz * vz);
                coupled += 1;
            }
        }
    }
    if (threadIdx.x == 0)
        state_all[item].steps += 1;
    if (!gam) // (uniform over the workgroup)
        return;

    // the item's tally, in an order fixed by N alone; every wave's use of `draws` lies before the workgroup barrier inside
    // block_tally, the store to it after
    block_tally<BLOCK, 1, 1>(&t_hi, &t_lo, &coupled);
    if (threadIdx.x == 0)
    {
        const double T = t_hi + t_lo; // the one rounding of the sum
        BathState* __restrict__ st = bath_state_all + item;
        st->draws = draws + 1;
        st->coupled = coupled;
        st->reservoir = st->reservoir - T * dt;
    }
}
} // namespace cavmd
