// cavmd_ledger_kernel.hpp -- every term of the conserved energy of a batch of independent small systems in ONE launch, one
// workgroup per system, appended to a time series in DEVICE memory: the energy ledger next to cavmd_recorder_kernel.hpp, whose
// structure this kernel has (the path from blockIdx to the row, the decision whether a call records, the counters, the ring).
//
// What the reference's EnergyTracker (src/cavitymd/analysis.py:425-1046) writes per output step -- the potential of every
// force, the three cavity energies, the molecular, cavity and total kinetic energy, the system total, the reservoir energy of
// every bath and universe_total_energy, its [CONSERVED] column -- is one 192-byte row here (cavmd_ledger_row).  Every input is
// read from device memory when the kernel RUNS, so a graph replay appends the row of the state it finds.
//
// Bits, per item: kinetic_group is recorder_batch_kernel's kinetic_energy for the same member list (the same tile load, addend,
// tree and fold, called here unchanged); kinetic_cavity is its cavity_kinetic (cavity_mode_numbers' first output).  A potential
// term is the sum of the .w column of one force array: the same tiles of BLOCK x UNROLL entries, the same per-lane dd_acc with
// addend w_i (a padding slot adds +0), block_reduce_dd1 per tile into LDS and recorder_fold, then hi + lo rounded once -- a
// fixed-order compensated sum within 2 ulp of the exact value.  Every other column is the listed expression of include/cavmd.h,
// one IEEE operation per +, * and / (the units are compiled with -ffp-contract=off).
#pragma once

#include "cavmd_recorder_kernel.hpp"

namespace cavmd
{
constexpr int kLedgerTerms = 4;      // d_energy[4]
constexpr int kLedgerReservoirs = 4; // d_reservoir[4]

// One system as the kernel reads it: the layout of cavmd_ledger_item (the table is uploaded as it is).
struct LedgerItem
{
    const cavmd_result* res;
    const v2d* vel2;
    const unsigned* members;
    unsigned n_members;
    unsigned N;
    const double* energy[kLedgerTerms]; // Scalar4 arrays, read as 4 doubles an entry
    const double* reservoir[kLedgerReservoirs];
    const double* time;
    double dof;
    unsigned add_cavity_kinetic;
    unsigned pad0;
    uint64_t pad;
};
static_assert(sizeof(LedgerItem) == 128, "one ledger item = 128 bytes");

// the .w of tile t's entries of one force array; padding slots (and an absent term): +0
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void ledger_load_w(const double* __restrict__ force, unsigned N, unsigned t, double (&w)[UNROLL])
{
    const size_t base = (size_t)t * (BLOCK * UNROLL) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
    {
        const size_t i = base + (size_t)u * BLOCK;
        w[u] = (force && i < N) ? force[4 * i + 3] : 0.0;
    }
}

template <int UNROLL>
__device__ __forceinline__ DD ledger_potential_terms(const double (&w)[UNROLL])
{
    DD acc {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        dd_acc(acc.hi, acc.lo, w[u]);
    return acc;
}

// blockIdx.x -> order[blockIdx.x] (items by max(N, n_members) descending, sorted on the host) -> the item, fetched once per
// workgroup.  Counters and series are indexed by ITEM, never by block.
// Both kernels have one body, cavmd_ledger_body.inc.  The first is the kernel of an object without a time rule, as it was
// before there was one; the second is launched while cavmd_runclock_ledger_set_rule has a rule on (last_time: n_items doubles).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void ledger_batch_kernel(const LedgerItem* __restrict__ items,
                                                             const unsigned* __restrict__ order, unsigned n_items,
                                                             uint64_t capacity, uint64_t period, double kB,
                                                             cavmd_ledger_row* __restrict__ series,
                                                             uint64_t* __restrict__ counters)
{
    constexpr bool TIMED = false;
    constexpr double time_interval = 0.0, max_time = 0.0;
    double* const last_time = nullptr;
#include "cavmd_ledger_body.inc"
}

template <int BLOCK, bool TIMED>
__global__ __launch_bounds__(BLOCK) void ledger_batch_kernel(const LedgerItem* __restrict__ items,
                                                             const unsigned* __restrict__ order, unsigned n_items,
                                                             uint64_t capacity, double kB, cavmd_ledger_row* __restrict__ series,
                                                             uint64_t* __restrict__ counters, double time_interval,
                                                             double max_time, double* __restrict__ last_time)
{
    constexpr uint64_t period = 1;
#include "cavmd_ledger_body.inc"
}
} // namespace cavmd
