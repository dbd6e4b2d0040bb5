// cavmd_recorder_kernel.hpp -- the per-step observables of a batch of independent small systems in ONE launch, one workgroup
// per system, appended to a time series in DEVICE memory: the third kernel of the batched step next to cavmd_batch_kernel.hpp
// (forces) and cavmd_bussi_batch_kernel.hpp (thermostat).
//
// What the reference's trackers write every step for every replica -- EnergyTracker (src/cavitymd/analysis.py:425-),
// CavityModeTracker (:1285-1417), DipoleAutocorrelation (:1424-) and the reduction of AdaptiveTimestepUpdater
// (src/cavitymd/simulation.py:66-92) -- is one 128-byte row here.  The write position lives in device memory, so a graph
// replay appends a NEW row each time; the host reads the series when it likes, behind a stream synchronisation.  Workgroups
// never wait for each other; the item's workgroup is the only writer of its counters and of its series (no atomics).
//
// Bits, per item: the result columns are the bytes of the cavmd_result block; the cavity mode is cavity_mode_numbers, which
// cavity_mode_kernel calls too; kinetic_energy and force_mass_sum are what cavmd_kinetic_energy / cavmd_force_mass_sum give that
// item alone on a device with at least kRecorderMaxTiles compute units: there kinetic_fused_kernel / force_mass_fused_kernel run
// one workgroup per tile of BLOCK * UNROLL entries (grid = min(tiles, CUs)), each leaving one double-double partial
// (block_reduce_dd1), and the last one folds them as "thread t merges partials t, t + BLOCK, ...; then block_reduce_dd1".  The
// workgroup below walks the same tiles with the same addends (kinetic_addend, force_mass_addend), reduces each with the same
// tree into a partial kept in LDS (tile_partial_to_lds), and folds them in that same order.
#pragma once

#include "cavmd_observable_kernels.hpp"

namespace cavmd
{
constexpr int kRecorderUnroll = kObservableUnroll; // entries per lane and tile: the tile of the two single paths
constexpr unsigned kRecorderMaxTiles = 64;  // CAVMD_BATCH_MAX_ITEM_N / (256 * 4)

// One system as the kernel reads it: the layout of cavmd_recorder_item (the table is uploaded as it is).
struct RecorderRow
{
    const cavmd_result* res;
    const v2d* vel2;
    const v2d* force2;
    const unsigned* members;
    unsigned N;
    unsigned n_members;
    uint64_t pad[3];
};
static_assert(sizeof(RecorderRow) == 64, "one recorder row = 64 bytes");

// Four words per item, kept as four arrays of n_items (rows first: that array is what cavmd_recorder_device_ptr hands out).
// phase and slot are calls % period and rows % capacity, carried along so that the kernel never divides.
enum RecorderCounter
{
    kRecRows = 0,
    kRecCalls = 1,
    kRecPhase = 2,
    kRecSlot = 3,
    kRecCounters = 4
};

// tile t's net forces; padding slots: force 0, as in force_mass_fused_kernel (whose loads are non-temporal)
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void recorder_load_force(const v2d* __restrict__ force2, unsigned N, unsigned t, v2d (&fxy)[UNROLL],
                                                    v2d (&fzw)[UNROLL])
{
    const size_t base = (size_t)t * (BLOCK * UNROLL) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
    {
        const size_t i = base + (size_t)u * BLOCK;
        const bool ok = i < N;
        const v2d zero = {0.0, 0.0};
        fxy[u] = ok ? force2[2 * i] : zero;
        fzw[u] = ok ? force2[2 * i + 1] : zero;
    }
}

// the (vz, m) half of tile t's velocities for |F| / m; padding slots: mass 1 ("padding lanes add 0 / 1")
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void recorder_load_mass(const v2d* __restrict__ vel2, unsigned N, unsigned t, v2d (&vzw)[UNROLL])
{
    const size_t base = (size_t)t * (BLOCK * UNROLL) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
    {
        const size_t i = base + (size_t)u * BLOCK;
        const v2d one = {0.0, 1.0};
        vzw[u] = i < N ? vel2[2 * i + 1] : one;
    }
}

template <int UNROLL>
__device__ __forceinline__ DD recorder_kinetic_terms(const v2d (&vxy)[UNROLL], const v2d (&vzw)[UNROLL])
{
    DD acc {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        dd_acc(acc.hi, acc.lo, kinetic_addend(vzw[u].y, vxy[u].x, vxy[u].y, vzw[u].x));
    return acc;
}

template <int UNROLL>
__device__ __forceinline__ DD recorder_force_mass_terms(const v2d (&fxy)[UNROLL], const v2d (&fzw)[UNROLL],
                                                        const v2d (&vzw)[UNROLL])
{
    DD acc {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        dd_acc(acc.hi, acc.lo, force_mass_addend(fxy[u], fzw[u], vzw[u]));
    return acc;
}

// the fold of fold_by_last_block: thread t merges partials t, t + BLOCK, ..., then the block tree; total in thread 0
template <int BLOCK>
__device__ __forceinline__ DD recorder_fold(const double (*part)[2], unsigned tiles)
{
    DD tot {0.0, 0.0};
    for (unsigned p = threadIdx.x; p < tiles; p += BLOCK)
        dd_merge(tot.hi, tot.lo, part[p][0], part[p][1]);
    tot = block_reduce_dd1<BLOCK>(tot);
    __syncthreads();
    return tot;
}

// blockIdx.x -> order[blockIdx.x] (items by max(N, n_members) descending, sorted on the host) -> the row, fetched once per
// workgroup.  Counters and series are indexed by ITEM, never by block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void recorder_batch_kernel(const RecorderRow* __restrict__ rows,
                                                               const unsigned* __restrict__ order, unsigned n_items,
                                                               uint64_t capacity, uint64_t period, double kB,
                                                               cavmd_record* __restrict__ series,
                                                               uint64_t* __restrict__ counters)
{
    constexpr int UNROLL = kRecorderUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    __shared__ double s_ke[kRecorderMaxTiles][2];
    __shared__ double s_fm[kRecorderMaxTiles][2];
    __shared__ int s_record;

    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const RecorderRow* __restrict__ row = rows + item;
    uint64_t* __restrict__ c_rows = counters + (size_t)kRecRows * n_items + item;
    uint64_t* __restrict__ c_calls = counters + (size_t)kRecCalls * n_items + item;
    uint64_t* __restrict__ c_phase = counters + (size_t)kRecPhase * n_items + item;
    uint64_t* __restrict__ c_slot = counters + (size_t)kRecSlot * n_items + item;

    // 1. does this call record?  Thread 0 alone reads the counters (it is also their only writer) and tells the others.
    //    (field_recorder_batch_kernel restates this: as a shared function it changed both kernels' register counts.)
    uint64_t calls = 0, phase = 0;
    if (threadIdx.x == 0)
    {
        calls = *c_calls + 1;
        phase = *c_phase + 1;
        s_record = (phase >= period);
    }
    __syncthreads();
    if (!s_record)
    {
        if (threadIdx.x == 0)
        {
            *c_calls = calls;
            *c_phase = phase;
        }
        return;
    }

    const v2d* __restrict__ vel2 = row->vel2;
    const v2d* __restrict__ force2 = row->force2;
    const unsigned* __restrict__ members = row->members;
    const unsigned n_ke = vel2 ? row->n_members : 0;
    const unsigned n_fm = (vel2 && force2) ? row->N : 0;
    const unsigned tiles_ke = (n_ke + TILE - 1) / TILE;
    const unsigned tiles_fm = (n_fm + TILE - 1) / TILE;

    // 2. one double-double partial per tile and sum.  Where the group is the whole system the velocities serve both sums:
    //    all 16 loads of a lane are in flight before the first addend (the production case: one tile, one round trip).
    if (!members && n_ke == n_fm)
    {
        for (unsigned t = 0; t < tiles_ke; ++t)
        {
            v2d vxy[UNROLL], vzw[UNROLL], fxy[UNROLL], fzw[UNROLL], mzw[UNROLL];
            sum_tile_load<BLOCK, UNROLL>(vel2, nullptr, n_ke, t, vxy, vzw);
            recorder_load_force<BLOCK, UNROLL>(force2, n_fm, t, fxy, fzw);
            __builtin_amdgcn_sched_barrier(0);
            const size_t base = (size_t)t * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) // the same (vz, m) half; a padding slot divides by 1, not by its mass 0
            {
                const v2d one = {0.0, 1.0};
                mzw[u] = (base + (size_t)u * BLOCK) < n_fm ? vzw[u] : one;
            }
            tile_partial_to_lds<BLOCK>(recorder_kinetic_terms<UNROLL>(vxy, vzw), s_ke, t);
            tile_partial_to_lds<BLOCK>(recorder_force_mass_terms<UNROLL>(fxy, fzw, mzw), s_fm, t);
        }
    }
    else
    {
        for (unsigned t = 0; t < tiles_ke; ++t)
        {
            v2d vxy[UNROLL], vzw[UNROLL];
            sum_tile_load<BLOCK, UNROLL>(vel2, members, n_ke, t, vxy, vzw);
            __builtin_amdgcn_sched_barrier(0);
            tile_partial_to_lds<BLOCK>(recorder_kinetic_terms<UNROLL>(vxy, vzw), s_ke, t);
        }
        for (unsigned t = 0; t < tiles_fm; ++t)
        {
            v2d fxy[UNROLL], fzw[UNROLL], mzw[UNROLL];
            recorder_load_force<BLOCK, UNROLL>(force2, n_fm, t, fxy, fzw);
            recorder_load_mass<BLOCK, UNROLL>(vel2, n_fm, t, mzw);
            __builtin_amdgcn_sched_barrier(0);
            tile_partial_to_lds<BLOCK>(recorder_force_mass_terms<UNROLL>(fxy, fzw, mzw), s_fm, t);
        }
    }
    const DD ke = recorder_fold<BLOCK>(s_ke, tiles_ke);
    const DD fm = recorder_fold<BLOCK>(s_fm, tiles_fm);

    // 3. the row: the evaluation's block as it is, the cavity mode, the two sums
    if (threadIdx.x == 0)
    {
        const cavmd_result* __restrict__ res = row->res;
        const uint64_t n_rows = *c_rows;
        const uint64_t slot = *c_slot;
        cavmd_record rec;
        rec.call = calls;
        rec.eval_sequence = res->sequence;
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            rec.energy[k] = res->energy[k];
            rec.total_dipole[k] = res->total_dipole[k];
            rec.q[k] = res->q[k];
        }
        const int p = res->photon_idx;
        double mode[4] = {0.0, 0.0, 0.0, 0.0};
        if (p >= 0 && vel2)
        {
            const v2d pxy = vel2[2 * (size_t)p], pzw = vel2[2 * (size_t)p + 1];
            cavity_mode_numbers(pzw.y, pxy.x, pxy.y, pzw.x, rec.energy[0], kB, mode);
        }
        rec.cavity_kinetic = mode[0];
        rec.cavity_temperature = mode[3];
        rec.kinetic_energy = 0.5 * (ke.hi + ke.lo);
        rec.force_mass_sum = fm.hi + fm.lo;
        rec.reserved = 0.0;
        series[(size_t)item * capacity + slot] = rec;
        record_counters_store(c_rows, c_calls, c_phase, c_slot, n_rows, slot, capacity, calls);
    }
}
} // namespace cavmd
