// cavmd_verlet_batch_kernel.hpp -- the two half-steps of velocity Verlet for a batch of independent small systems, each half
// in ONE launch, one workgroup per system: the step between cavmd_batch_kernel.hpp's forces and cavmd_bussi_batch_kernel.hpp's
// thermostat.
//
// The reference has no integrator of its own: its driver hands the molecules to HOOMD-blue's ConstantVolume method and the
// one cavity particle to HOOMD-blue's Langevin method (examples/05_advanced_run.py:652, 677).  The expressions below restate
// TwoStepConstantVolume::integrateStepOne / integrateStepTwo and TwoStepLangevin::integrateStepTwo of HOOMD-blue 4.x
// [HOOMD upstream, not in checkout]; include/cavmd.h carries them as the contract:
//   step one   v += (0.5 a) dt;  x += dt v;  one wrap per axis into [-L/2, L/2) with the image flag following
//   step two   F = ((f0 + f1) + f2) + f3;  on the Langevin particle F += uniform * coeff - gamma v;  a = F / m as F * (1/m);
//              v += (0.5 a) dt
// Every operation is one IEEE rounding (no FMA).  A workgroup reads its step's inputs (dt, the Langevin coefficients and
// variates) from a row in DEVICE memory when it runs, so a captured launch follows an adaptive dt and fresh variates on
// replay.  Workgroups never wait for each other; the per-item state is updated by threads of the owning workgroup with
// plain vector stores.
#pragma once

#include "cavmd_reduce.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr int kVerletUnroll = 2; // particles per lane and tile: 512 per tile, the production system (N = 501) is one tile
constexpr int kVerletMaxForces = 4;

// One system as the kernels read it: the layout of cavmd_verlet_item (the table is uploaded as it is).
struct VerletRow
{
    v2d* pos2;
    int* image;
    v2d* vel2;
    double* accel;
    const v2d* force2[kVerletMaxForces];
    v2d* net2;
    double Lx, Ly, Lz;
    unsigned n;
    int langevin;
    uint64_t pad[3];
};
static_assert(sizeof(VerletRow) == 128, "one integrator row = 128 bytes");

// One step's inputs of one item (the layout of cavmd_verlet_input), in device memory, written by the caller in stream order.
struct VerletInput
{
    double dt, gamma, coeff;
    double uniform[3];
    uint64_t skip;
    uint64_t pad;
};
static_assert(sizeof(VerletInput) == 64, "one integrator input row = 64 bytes");

// Per-item counters in device memory (the layout of cavmd_verlet_state).
struct VerletState
{
    uint64_t steps;
    uint64_t out_of_box;
    double reservoir;
    double pad;
};
static_assert(sizeof(VerletState) == 32, "one integrator state = 32 bytes");

// sum over the workgroup of a per-thread count; the total is returned to thread 0 (other threads: unspecified).  It restates
// block_tally of cavmd_reduce.hpp for no double and one count: as block_tally<BLOCK, 0, 1> it reordered 16 instruction lines
// of verlet_step_one_kernel, which runs every step and was to keep its text (profiles/shared_step_two/README.md).
template <int BLOCK>
__device__ __forceinline__ unsigned verlet_block_count(unsigned c)
{
    __shared__ unsigned s_count[BLOCK / kWave];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
        c += __shfl_down(c, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0)
        s_count[threadIdx.x / kWave] = c;
    __syncthreads();
    unsigned total = 0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w)
            total += s_count[w];
    return total;
}

// one axis of step one for one particle: kick, drift, one wrap; returns 1 if the coordinate is still outside [lo, hi)
__device__ __forceinline__ unsigned verlet_axis_step_one(double& x, double& v, int& img, double a, double dt, double L)
{
    v = v + (0.5 * a) * dt;
    x = x + dt * v;
    const double hi = L * 0.5;
    const double lo = -hi;
    if (x >= hi)
    {
        x -= L;
        img += 1;
    }
    else if (x < lo)
    {
        x += L;
        img -= 1;
    }
    return (x >= lo && x < hi) ? 0u : 1u; // NaN is counted
}

// blockIdx.x -> order[blockIdx.x] (items by N descending, sorted on the host) -> the row, fetched once per workgroup with
// scalar loads.  States are indexed by ITEM, never by block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void verlet_step_one_kernel(const VerletRow* __restrict__ rows,
                                                                const unsigned* __restrict__ order,
                                                                const VerletInput* __restrict__ inputs,
                                                                VerletState* __restrict__ state_all)
{
    constexpr int UNROLL = kVerletUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const VerletRow* __restrict__ row = rows + item;
    const VerletInput* __restrict__ in = inputs + item;
    const unsigned n = row->n;
    if (n == 0 || in->skip != 0)
        return; // dt == 0 or an empty system: nothing of the item is read or written
    v2d* __restrict__ pos2 = row->pos2;
    v2d* __restrict__ vel2 = row->vel2;
    int* __restrict__ image = row->image;
    const double* __restrict__ accel = row->accel;
    const double dt = in->dt;
    const double Lx = row->Lx, Ly = row->Ly, Lz = row->Lz;
    const unsigned tiles = (n + TILE - 1) / TILE;

    unsigned outside = 0;
    for (unsigned t = 0; t < tiles; ++t)
    {
        // all of the tile's loads first: 2 x 16 B of pos, 2 x 16 B of vel, 3 x 8 B of accel, 3 x 4 B of image per particle
        v2d pxy[UNROLL], pzw[UNROLL], vxy[UNROLL], vzw[UNROLL];
        double a[UNROLL][3];
        int img[UNROLL][3];
        const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            if (j < n)
            {
                pxy[u] = pos2[2 * (size_t)j];
                pzw[u] = pos2[2 * (size_t)j + 1];
                vxy[u] = vel2[2 * (size_t)j];
                vzw[u] = vel2[2 * (size_t)j + 1];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                {
                    a[u][c] = accel[3 * (size_t)j + c];
                    img[u][c] = image[3 * (size_t)j + c];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
            if (j >= n)
                continue;
            const int ix = img[u][0], iy = img[u][1], iz = img[u][2];
            double x = pxy[u].x, y = pxy[u].y, z = pzw[u].x, vx = vxy[u].x, vy = vxy[u].y, vz = vzw[u].x;
            outside += verlet_axis_step_one(x, vx, img[u][0], a[u][0], dt, Lx);
            outside += verlet_axis_step_one(y, vy, img[u][1], a[u][1], dt, Ly);
            outside += verlet_axis_step_one(z, vz, img[u][2], a[u][2], dt, Lz);
            // only what can change goes back: x, y, z (pos.w and vel.w are never written) and an image that moved
            const v2d xy = {x, y}, vxy_new = {vx, vy};
            pos2[2 * (size_t)j] = xy;
            reinterpret_cast<double*>(pos2)[4 * (size_t)j + 2] = z;
            vel2[2 * (size_t)j] = vxy_new;
            reinterpret_cast<double*>(vel2)[4 * (size_t)j + 2] = vz;
            if (img[u][0] != ix)
                image[3 * (size_t)j] = img[u][0];
            if (img[u][1] != iy)
                image[3 * (size_t)j + 1] = img[u][1];
            if (img[u][2] != iz)
                image[3 * (size_t)j + 2] = img[u][2];
        }
    }
    const unsigned total = verlet_block_count<BLOCK>(outside);
    if (threadIdx.x == 0 && total != 0)
        state_all[item].out_of_box += total;
}

// ACCEL_ONLY: a = F / m and the net force, nothing else (what HOOMD does once at the start of a run); `inputs` is not read.
template <int BLOCK, bool ACCEL_ONLY>
__global__ __launch_bounds__(BLOCK) void verlet_step_two_kernel(const VerletRow* __restrict__ rows,
                                                                const unsigned* __restrict__ order,
                                                                const VerletInput* __restrict__ inputs,
                                                                VerletState* __restrict__ state_all)
{
    constexpr int UNROLL = kVerletUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const VerletRow* __restrict__ row = rows + item;
    const unsigned n = row->n;
    if (n == 0)
        return;
    double dt = 0.0, gamma = 0.0, coeff = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    int langevin = -1;
    if constexpr (!ACCEL_ONLY)
    {
        const VerletInput* __restrict__ in = inputs + item;
        if (in->skip != 0)
            return;
        dt = in->dt;
        gamma = in->gamma;
        coeff = in->coeff;
        ux = in->uniform[0];
        uy = in->uniform[1];
        uz = in->uniform[2];
        langevin = (gamma != 0.0) ? row->langevin : -1;
    }
    v2d* __restrict__ vel2 = row->vel2;
    double* __restrict__ accel = row->accel;
    v2d* __restrict__ net2 = row->net2;
    const v2d* __restrict__ f0 = row->force2[0];
    const v2d* __restrict__ f1 = row->force2[1];
    const v2d* __restrict__ f2 = f1 ? row->force2[2] : nullptr; // the list ends at the first NULL
    const v2d* __restrict__ f3 = f2 ? row->force2[3] : nullptr;
    const unsigned tiles = (n + TILE - 1) / TILE;

    for (unsigned t = 0; t < tiles; ++t)
    {
        // all of the tile's loads first: 2 x 16 B of vel and of every force array per particle
        v2d vxy[UNROLL], vzw[UNROLL], axy[UNROLL], azw[UNROLL], bxy[UNROLL], bzw[UNROLL], cxy[UNROLL], czw[UNROLL], dxy[UNROLL],
            dzw[UNROLL];
        const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const unsigned j = base + u * BLOCK;
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
            if (net2)
            {
                net2[2 * (size_t)j] = Fxy;
                net2[2 * (size_t)j + 1] = Fzw;
            }
            double Fx = Fxy.x, Fy = Fxy.y, Fz = Fzw.x;
            double bdx = 0.0, bdy = 0.0, bdz = 0.0;
            if constexpr (!ACCEL_ONLY)
            {
                if ((int)j == langevin)
                {
                    // the bath of the one cavity particle: the force from the velocity BEFORE the kick
                    bdx = ux * coeff - gamma * vxy[u].x;
                    bdy = uy * coeff - gamma * vxy[u].y;
                    bdz = uz * coeff - gamma * vzw[u].x;
                    Fx = Fx + bdx;
                    Fy = Fy + bdy;
                    Fz = Fz + bdz;
                }
            }
            const double ax = Fx * minv, ay = Fy * minv, az = Fz * minv;
            accel[3 * (size_t)j] = ax;
            accel[3 * (size_t)j + 1] = ay;
            accel[3 * (size_t)j + 2] = az;
            if constexpr (!ACCEL_ONLY)
            {
                vxy[u].x = vxy[u].x + (0.5 * ax) * dt;
                vxy[u].y = vxy[u].y + (0.5 * ay) * dt;
                const double vz = vzw[u].x + (0.5 * az) * dt;
                vel2[2 * (size_t)j] = vxy[u];
                reinterpret_cast<double*>(vel2)[4 * (size_t)j + 2] = vz; // vel.w is never written
                if ((int)j == langevin)
                {
                    // the tally, with the velocity just stored (AFTER the kick); this lane owns the item's reservoir word
                    const double tally = (bdx * vxy[u].x + bdy * vxy[u].y) + bdz * vz;
                    state_all[item].reservoir = state_all[item].reservoir - tally * dt;
                }
            }
        }
    }
    if constexpr (!ACCEL_ONLY)
        if (threadIdx.x == 0)
            state_all[item].steps += 1;
}
} // namespace cavmd
