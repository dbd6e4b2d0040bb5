// cavmd_thermalize_kernel.hpp -- the START of a run for every system of a batch, in ONE launch, one workgroup per system:
// seeded Maxwell-Boltzmann velocities on any set of particles, their total momentum taken out, and the cavity particle's
// velocity and placement (q = 0, or displaced by the molecular dipole of the cavity batch's result block).
//
// The reference's driver does both on the host before its first step (examples/05_advanced_run.py:710-750 thermalize_system,
// :455-494 create_cavity_particle), with one numpy generator walked through the systems in order.  include/cavmd.h ("the start
// of a batch") carries the contract; in short, per item, `draws` being the item's counter in DEVICE memory when the kernel runs:
//   generator  Philox4x32-10 (draw_philox of cavmd_draw_kernel.hpp), key = the item's seed, counter = (draws low, draws high, j,
//              purpose): 0xC0000000 + c for velocity component c of particle j, 0xC0000008 + c for the photon's position
//   normal     sqrt(-2 log u1) * cospi(2 u2), one block per normal (DrawStream::normal)
//   members    for j of the list (or of the default set) with j < N and a finite mass m = vel.w > 0: v_c = sqrt(kT / m) * n_c;
//              anything else is left as it is and counted
//   momentum   P_c = the double-double sum of m * v_c in an order fixed by N and the list (lane-serial over the tiles of
//              kThermalizeTile entries, then block_tally of cavmd_reduce.hpp: a shuffle tree over the wave, the four waves in
//              wave order), rounded once;
//              v_c = v_c - (P_c / double(thermalised)) / m
//   photon     v_c = sqrt(kT / m_p) * n_c;  x_c = finite_q ? ((-d_c) * g) / K : 0, x_z = 0;  x_c += sqrt(kT / K) * n_c if g != 0;
//              i_c = floor((x_c + L_c / 2) / L_c);  pos_c = x_c - i_c * L_c;  image = i
// The second pass re-reads the velocities the SAME thread stored in the first (the same entries of the same tiles), so it needs
// no fence of its own.  `draws` is read by every thread at the top and written by thread 0 after the workgroup barrier of the
// reduction.  The photon's row is written by thread 0 after a further barrier, behind every member store of the workgroup.
// Workgroups never wait for each other; every loop is bounded by N or by the list's length; no atomics, nothing mapped; the
// state is written with plain vector stores by its own workgroup.  Philox, log, cospi, the division and the square root run
// on lanes that hold a particle to write only.
#pragma once

#include "cavmd_draw_kernel.hpp"
#include "cavmd_reduce.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
// Entries per lane and tile.  Three normals a particle are three Philox blocks, three logs and three cospis: two particles in
// flight give the scheduler independent chains without approaching the register budget (profiles/thermalize/README.md).
constexpr int kThermalizeUnroll = 2;
constexpr unsigned kThermalizeTile = 256 * kThermalizeUnroll; // T of the contract: the sum's order is stated in these tiles
constexpr unsigned kThermalizePurposeVelocity = 0xC0000000u;  // + c; apart from cavmd_draw's purposes (< 48) and the bath's
constexpr unsigned kThermalizePurposePosition = 0xC0000008u;  // + c   (0x80000000 + b)

constexpr unsigned kThermalizeZeroMomentum = 1u; // the bits of cavmd_thermalize_item.flags
constexpr unsigned kThermalizePlacePhoton = 2u;
constexpr unsigned kThermalizeFiniteQ = 4u;
constexpr unsigned kThermalizePhotonVelocity = 8u;

// One item as the kernel reads it: the layout of cavmd_thermalize_item (the table is uploaded as it is).
struct ThermalizeRow
{
    v2d* vel2;
    const unsigned* members;
    v2d* pos2;
    int* image;
    const cavmd_result* res;
    uint64_t seed;
    double kT;
    unsigned n;
    unsigned n_members;
    unsigned flags;
    unsigned pad0;
    double L[3];
    double omegac, couplstr, K, phmass;
    uint64_t pad[4];
};
static_assert(sizeof(ThermalizeRow) == 160, "one thermalize row = 160 bytes");

// Per-item counters in device memory (the layout of cavmd_thermalize_state).
struct ThermalizeState
{
    uint64_t draws;
    uint64_t thermalised;
    uint64_t skipped;
    double momentum[3];
    int photon;
    unsigned pad0;
    uint64_t pad;
};
static_assert(sizeof(ThermalizeState) == 64, "one thermalize state = 64 bytes");

// a mass the contract thermalises: finite and > 0 (a NaN fails both comparisons)
__device__ __forceinline__ bool thermalize_mass_ok(double m)
{
    return m > 0.0 && m <= 0x1.fffffffffffffp+1023;
}

// entry k of the item's set -> the particle it names; *in_set is false past the set's end and for the photon of the default set
__device__ __forceinline__ unsigned thermalize_entry(const unsigned* __restrict__ members, unsigned count, int photon, unsigned k,
                                                     bool* in_set)
{
    *in_set = k < count;
    if (!*in_set)
        return 0u;
    if (members)
        return members[k];
    *in_set = (int)k != photon;
    return k;
}

// The velocity draw of particle j of mass m, for members and photon alike: sigma = sqrt(kT / m), three normals of purpose
// 0xC0000000 + c, two stores (vel.w is never written).  Returns the three components.
__device__ __forceinline__ double3 thermalize_velocity(DrawStream s, v2d* __restrict__ vel2, unsigned j, double kT, double m)
{
    s.item = j;
    const double sigma = sqrt(kT / m);
    double3 v;
    v.x = sigma * s.normal(kThermalizePurposeVelocity);
    v.y = sigma * s.normal(kThermalizePurposeVelocity + 1u);
    v.z = sigma * s.normal(kThermalizePurposeVelocity + 2u);
    const v2d vxy = {v.x, v.y};
    vel2[2 * (size_t)j] = vxy;
    reinterpret_cast<double*>(vel2)[4 * (size_t)j + 2] = v.z;
    return v;
}

// blockIdx.x -> order[blockIdx.x] (items by N descending, sorted on the host) -> the row, fetched once per workgroup with scalar
// loads.  States are indexed by ITEM, never by block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void thermalize_batch_kernel(const ThermalizeRow* __restrict__ rows,
                                                                 const unsigned* __restrict__ order,
                                                                 ThermalizeState* __restrict__ state_all)
{
    constexpr int UNROLL = kThermalizeUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    static_assert(TILE == kThermalizeTile, "the tile the contract names");
    __shared__ double s_P[3];
    __shared__ unsigned s_total;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const ThermalizeRow* __restrict__ row = rows + item;
    const unsigned n = row->n;
    if (n == 0)
        return;
    const unsigned flags = row->flags;
    const double kT = row->kT;
    const uint2 key = make_uint2((unsigned)row->seed, (unsigned)(row->seed >> 32));
    const uint64_t draws = state_all[item].draws;
    const DrawStream gen = {(unsigned)draws, (unsigned)(draws >> 32), 0u, key};
    v2d* __restrict__ vel2 = row->vel2;
    const unsigned* __restrict__ members = row->members;
    const cavmd_result* __restrict__ res = row->res;
    int photon = -1; // the a8 no-photon rule: a result block of another N, or without a photon, names none
    if (res)
    {
        const int p = res->photon_idx;
        if (res->n_particles == n && p >= 0 && (unsigned)p < n)
            photon = p;
    }
    const unsigned count = members ? row->n_members : n;
    const unsigned tiles = (count + TILE - 1) / TILE;
    const bool zero = (flags & kThermalizeZeroMomentum) != 0;

    // ---- pass one: the velocities, and this lane's share of the momentum (double-double) -----------------------------------
    double p_hi[3] = {0.0, 0.0, 0.0}, p_lo[3] = {0.0, 0.0, 0.0};
    unsigned counts[2] = {0, 0}; // thermalised, skipped
    for (unsigned t = 0; t < tiles; ++t)
    {
        unsigned j[UNROLL];
        bool in_set[UNROLL], write[UNROLL];
        v2d vzw[UNROLL];
        const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            j[u] = thermalize_entry(members, count, photon, base + u * BLOCK, &in_set[u]);
            write[u] = in_set[u] && j[u] < n; // an index at or beyond N is never dereferenced
            if (write[u])
                vzw[u] = vel2[2 * (size_t)j[u] + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            if (!in_set[u])
                continue;
            const double m = write[u] ? vzw[u].y : 0.0;
            if (!write[u] || !thermalize_mass_ok(m))
            {
                counts[1] += 1;
                continue;
            }
            const double3 v = thermalize_velocity(gen, vel2, j[u], kT, m);
            if (zero)
            {
                dd_acc(p_hi[0], p_lo[0], m * v.x);
                dd_acc(p_hi[1], p_lo[1], m * v.y);
                dd_acc(p_hi[2], p_lo[2], m * v.z);
            }
            counts[0] += 1;
        }
    }

    // ---- the item's totals, in an order fixed by N and the list alone; every thread's use of `draws` lies before the barrier
    // in block_tally, the store to it after -------------------------------------------------------------------------------------
    block_tally<BLOCK, 3, 2>(p_hi, p_lo, counts);
    if (threadIdx.x == 0)
    {
        const unsigned total = counts[0], skip = counts[1];
        double P[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
        {
            P[c] = (zero && total != 0) ? p_hi[c] + p_lo[c] : 0.0; // the one rounding of the sum
            s_P[c] = P[c];
        }
        s_total = total;
        ThermalizeState st;
        st.draws = draws + 1;
        st.thermalised = total;
        st.skipped = skip;
        st.momentum[0] = P[0];
        st.momentum[1] = P[1];
        st.momentum[2] = P[2];
        st.photon = photon;
        st.pad0 = 0;
        st.pad = 0;
        // four 16-byte stores: the states are allocated by the library, 64 bytes each
        __builtin_memcpy(__builtin_assume_aligned(state_all + item, 16), &st, sizeof(st));
    }
    __syncthreads();

    // ---- pass two: the momentum taken out of the particles pass one wrote (each thread re-reads its own stores) --------------
    const unsigned total = s_total;
    if (zero && total != 0)
    {
        const double share[3] = {s_P[0] / (double)total, s_P[1] / (double)total, s_P[2] / (double)total};
        for (unsigned t = 0; t < tiles; ++t)
        {
            const unsigned base = t * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                bool in_set;
                const unsigned jj = thermalize_entry(members, count, photon, base + u * BLOCK, &in_set);
                if (!in_set || jj >= n)
                    continue;
                v2d vxy = vel2[2 * (size_t)jj];
                const v2d vzw = vel2[2 * (size_t)jj + 1];
                const double m = vzw.y;
                if (!thermalize_mass_ok(m))
                    continue;
                vxy.x = vxy.x - share[0] / m;
                vxy.y = vxy.y - share[1] / m;
                vel2[2 * (size_t)jj] = vxy;
                reinterpret_cast<double*>(vel2)[4 * (size_t)jj + 2] = vzw.x - share[2] / m;
            }
        }
    }
    if (photon < 0 || (flags & (kThermalizePhotonVelocity | kThermalizePlacePhoton)) == 0) // (uniform over the workgroup)
        return;
    __syncthreads(); // the photon's row goes last: behind the store of a list that names it

    // ---- the photon: its velocity (the driver's :729) and its placement (:464-494), one thread --------------------------------
    if (threadIdx.x != 0)
        return;
    if (flags & kThermalizePhotonVelocity)
    {
        const double m = vel2[2 * (size_t)photon + 1].y;
        if (thermalize_mass_ok(m)) // no momentum term: the photon is not one of the members
            thermalize_velocity(gen, vel2, (unsigned)photon, kT, m);
    }
    if (flags & kThermalizePlacePhoton)
    {
        const double g = row->couplstr, K = row->K;
        DrawStream s = gen;
        s.item = (unsigned)photon;
        double x[3] = {0.0, 0.0, 0.0};
        if (flags & kThermalizeFiniteQ)
        {
            x[0] = ((-res->dipole[0]) * g) / K;
            x[1] = ((-res->dipole[1]) * g) / K; // x_z stays 0
        }
        if (g != 0.0)
        {
            const double spread = sqrt(kT / K);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                x[c] = x[c] + spread * s.normal(kThermalizePurposePosition + (unsigned)c);
        }
        int im[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
        {
            const double L = row->L[c];
            const double i = floor((x[c] + L / 2.0) / L);
            x[c] = x[c] - i * L;
            im[c] = (int)i;
        }
        v2d* __restrict__ pos2 = row->pos2;
        v2d pxy;
        pxy.x = x[0];
        pxy.y = x[1];
        pos2[2 * (size_t)photon] = pxy;
        reinterpret_cast<double*>(pos2)[4 * (size_t)photon + 2] = x[2]; // pos.w (the type id) is never written
        int* __restrict__ image = row->image + 3 * (size_t)photon;
        image[0] = im[0];
        image[1] = im[1];
        image[2] = im[2];
    }
}
} // namespace cavmd
