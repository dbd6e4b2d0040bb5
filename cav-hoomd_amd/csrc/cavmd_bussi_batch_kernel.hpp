// cavmd_bussi_batch_kernel.hpp -- the translational Bussi thermostat step of a batch of independent small systems in ONE
// launch, one workgroup per system: the other half of cavmd_batch_kernel.hpp's step.
//
// Every replica of the reference's production workload (N = 501 x 500 replicas, submit.sh:3) is thermostatted each step
// (src/BussiReservoirThermostat.h:43-98, 177-225).  cavmd_bussi_step_device does that for ONE system with two launches and
// takes its variates as kernel arguments; here a workgroup does the whole step of its system -- kinetic energy, the rule, the
// books, the rescale -- and reads the step's random inputs from a row in DEVICE memory, so the launch can be captured into a
// graph and stays stochastic on replay.  Workgroups never wait for each other.
//
// Bits: per item what cavmd_bussi_step_device gives that item alone on a device with at least kBussiBatchMaxTiles compute
// units.  There the single path's first launch has one workgroup per tile of BLOCK * UNROLL members (grid = min(tiles, CUs)),
// each leaving one double-double partial (kinetic_partial -> block_reduce_dd1), and its second launch folds them as "thread t
// merges partials t, t + BLOCK, ...; then block_reduce_dd1".  The workgroup below walks the same tiles (sum_tile_load) with the
// same addend (kinetic_addend), reduces each with the same tree into a partial kept in LDS (tile_partial_to_lds), and folds
// them in that same order: same addends, same tree, same K.
#pragma once

#include "cavmd_observable_kernels.hpp"

namespace cavmd
{
constexpr int kBussiBatchUnroll = kObservableUnroll; // members per lane and tile: the tile of cavmd_bussi_step_device
constexpr unsigned kBussiBatchMaxTiles = 64; // CAVMD_BATCH_MAX_ITEM_N / (256 * 4)

// One system of a thermostat batch as the kernel reads it: the layout of cavmd_bussi_batch_item (the table is uploaded as it is).
struct BussiBatchRow
{
    v2d* vel2;
    const unsigned* members;
    unsigned n;
    unsigned reserved0;
    double dof;
    uint64_t pad[4];
};
static_assert(sizeof(BussiBatchRow) == 64, "one thermostat batch row = 64 bytes");

// One step's inputs of one item (the layout of cavmd_bussi_batch_input), in device memory, written by the caller in stream
// order before the step.
struct BussiBatchInput
{
    double normal_variate, gamma_variate, c, set_T;
    uint64_t skip;
    uint64_t pad[3];
};
static_assert(sizeof(BussiBatchInput) == 64, "one thermostat input row = 64 bytes");

// Per-item block in mapped, coherent pinned host memory: the state after the item's last applied step and the stamp of the
// last step that passed over the item (skipped steps stamp too, so that a read never waits for an item with nothing to do).
struct HostBussiBatch
{
    BussiDevice state;
    uint64_t ready;
    uint64_t pad;
};
static_assert(sizeof(HostBussiBatch) == 64, "one host block = 64 bytes");

// tile t of the item into a ScaleTile: the sum's load, with the indices the rescale stores through
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void bussi_batch_tile_load(const v2d* __restrict__ vel2, const unsigned* __restrict__ members,
                                                      unsigned n, unsigned t, ScaleTile<BLOCK, UNROLL>& r)
{
    sum_tile_load<BLOCK, UNROLL>(vel2, members, n, t, r.xy, r.zw, r.j);
}

// blockIdx.x -> order[blockIdx.x] (items by n_members descending, sorted on the host) -> the row, fetched once per workgroup
// with scalar loads.  States and host blocks are indexed by ITEM, never by block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void bussi_batch_kernel(const BussiBatchRow* __restrict__ rows,
                                                            const unsigned* __restrict__ order,
                                                            const BussiBatchInput* __restrict__ inputs, uint64_t sequence,
                                                            BussiDevice* __restrict__ state_all,
                                                            HostBussiBatch* __restrict__ host_all)
{
    constexpr int UNROLL = kBussiBatchUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    __shared__ double s_part[kBussiBatchMaxTiles][2];
    __shared__ double s_alpha;

    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const BussiBatchRow* __restrict__ row = rows + item;
    const BussiBatchInput* __restrict__ in = inputs + item;
    HostBussiBatch* __restrict__ host = host_all + item;
    const unsigned n = row->n;
    if (n == 0 || in->skip != 0)
    {
        // dt == 0 (src/BussiReservoirThermostat.h:45-48) or an empty group: what cavmd_bussi_step_device does by enqueuing
        // nothing.  Only the stamp moves; the host block keeps the state of the item's last applied step.
        if (threadIdx.x == 0)
            __hip_atomic_store(&host->ready, sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    v2d* __restrict__ vel2 = row->vel2;
    const unsigned* __restrict__ members = row->members;
    const unsigned tiles = (n + TILE - 1) / TILE;

    // 1. one double-double partial per tile, each through the tree the single path's first launch runs per workgroup.  The
    //    LAST tile stays in registers for the rescale (the only tile of the production case: 64 n bytes moved, not 96 n).
    ScaleTile<BLOCK, UNROLL> r;
    for (unsigned t = 0; t < tiles; ++t)
    {
        bussi_batch_tile_load<BLOCK, UNROLL>(vel2, members, n, t, r);
        __builtin_amdgcn_sched_barrier(0);
        DD acc {0.0, 0.0};
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            dd_acc(acc.hi, acc.lo, kinetic_addend(r.zw[u].y, r.xy[u].x, r.xy[u].y, r.zw[u].x));
        tile_partial_to_lds<BLOCK>(acc, s_part, t);
    }
    // the single path's second launch: thread t merges partials t, t + BLOCK, ... (at most one here), then the block tree --
    // also for ONE partial, which goes through thread 0 and a second tree exactly as it does there
    DD tot {0.0, 0.0};
    for (unsigned p = threadIdx.x; p < tiles; p += BLOCK)
        dd_merge(tot.hi, tot.lo, s_part[p][0], s_part[p][1]);
    tot = block_reduce_dd1<BLOCK>(tot);

    // 2. the rule and the books (bussi_rescale_fused_kernel's, per item)
    BussiDevice s = {};
    if (threadIdx.x == 0)
    {
        const double dof = row->dof;
        const double K = 0.5 * (tot.hi + tot.lo);
        const bool refused = (dof != 0 && K == 0); // "Bussi thermostat requires non-zero initial momenta." (:57-61)
        const double alpha = refused ? 1.0 : bussi_alpha_from_c(K, dof, in->c, in->set_T, in->normal_variate, in->gamma_variate);
        s_alpha = alpha;
        s = state_all[item];
        s.kinetic = K;
        s.alpha = alpha;
        if (refused)
        {
            s.instantaneous = 0.0; // nothing is rescaled; counted, and reported by the next cavmd_bussi_batch_read
            s.errors += 1;
        }
        else
        {
            const double delta = K * (1.0 - alpha * alpha); // src/BussiReservoirThermostat.h:86-95
            s.reservoir += delta;
            s.instantaneous = delta;
            s.steps += 1;
        }
        state_all[item] = s;
    }
    __syncthreads();
    const double alpha = s_alpha;

    // 3. v.xyz *= alpha; alpha == 1 (a refused step, 0 degrees of freedom) leaves the array untouched, as the single path does
    if (alpha != 1.0)
    {
        scale_tile_store<BLOCK, UNROLL>(vel2, alpha, r); // the last tile, still in registers
        for (unsigned t = 0; t + 1 < tiles; ++t)         // the others again (L2-hot: this workgroup has just read them)
        {
            bussi_batch_tile_load<BLOCK, UNROLL>(vel2, members, n, t, r);
            __builtin_amdgcn_sched_barrier(0);
            scale_tile_store<BLOCK, UNROLL>(vel2, alpha, r);
        }
    }
    __syncthreads(); // every wave has issued its velocity stores
    if (threadIdx.x == 0)
    {
        host->state = s;
        __hip_atomic_store(&host->ready, sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
} // namespace cavmd
