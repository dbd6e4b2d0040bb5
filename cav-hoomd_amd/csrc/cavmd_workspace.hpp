// Host-only: struct cavmd_workspace, and what BOTH units that see inside it use (cavmd_capi.hip: create, destroy, the
// evaluation and its results, profiling, tunables; cavmd_observables.hip: the observables and the workspace thermostat).
// No other unit includes this: the eleven batch objects reach a workspace through its WorkspaceTie (cavmd_item_table.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "cavmd.h"
#include "cavmd_force_kernels.hpp"      // HostResult
#include "cavmd_persistent_kernel.hpp"  // kSyncFailed, kSyncRepaired
#include "cavmd_observable_kernels.hpp" // HostMode, HostScalar, BussiDevice, HostBussi
#include "cavmd_host_support.hpp"       // the buffer owners, stream_capturing
#include "cavmd_item_table.hpp"         // WorkspaceTie

namespace
{
constexpr int kSmallSystemMaxN = 1024;         // single-block path (one batch of 4 x 256 particles) wins up to ~1000 particles against the
                                               // single-launch kernel: 5.0 vs 6.0 us at N = 501, 6.0 vs 6.0 at 1001, 7.0 vs 6.1 at 1101,
                                               // 7.9 vs 6.2 at 1401 (profiles/r02/ab_small_system.txt)
constexpr uint64_t kSuspendFirst = 1ull << 16, kSuspendMax = 1ull << 31, kSuspendForever = ~0ull;
constexpr unsigned kResultHistory = 64;          // default depth of the result ring ("result_history"): 16 KiB pinned
} // namespace

namespace cavmd
{
// The fixed part of the workspace's mapped host memory (never reallocated): the starvation flag of the single-launch kernel,
// and the one block every evaluation publishes into once the workspace has been captured (a replay cannot pick a ring slot).
struct HostControl
{
    HostResult fixed;
    unsigned sync_error; // kSyncFailed / kSyncRepaired, raised by a starved single-launch evaluation (consume_sync_timeout)
    unsigned pad[63];
};
} // namespace cavmd

struct cavmd_workspace : WorkspaceTie // device and dependents: what the batch objects may see (cavmd_item_table.hpp)
{
    int num_cu = 0;
    char arch[64] = {0};
    size_t max_N = 0;
    unsigned max_parts = 0;
    cavmd::DeviceArray<double> d_part;
    cavmd::DeviceArray<int> d_ipart;
    cavmd::DeviceArray<cavmd_result> d_result;
    cavmd::MappedBlock<cavmd::HostResult> h_ring;     // ring_depth result slots; evaluation s publishes into slot s % ring_depth
    unsigned ring_depth = kResultHistory;
    uint64_t history_first = 1;         // oldest sequence the ring can hold (raised when "result_history" reallocates it)
    cavmd::MappedBlock<cavmd::HostControl> h_ctl;     // fixed: starvation flag + the block of a captured workspace
    hipStream_t last_stream = nullptr;
    bool computed = false;
    uint64_t sequence = 0;
    // tunables
    // Defaults from interleaved A/B runs on MI355X (csrc/microbench.hip; profiles/r01/microbench_*.txt):
    int reduce_blocks_per_cu = 1; // <= 256 partials: the fused force map folds them with one load per thread
    int map_blocks_per_cu = 2;    // every fused block re-folds the partials, so few, long-lived blocks
    int map_nt_store = -1;        // -1 auto (non-temporal from kNtStoreMinN particles up), 0 plain, 1 non-temporal, 2 write-through
    int reduce_nt_load = -1;      // -1 auto, 0 plain, 1 pos+image non-temporal, 2 all non-temporal.  The two-launch reduction
                                  // only: the single launch always reads with policy 1 (a third dispatch dimension would
                                  // triple its instantiations, and it never runs where the charges outgrow the cache)
    int fused_finalize = 1;       // 1: two launches (finalize folded into the force map), 0: three launches
    int map_reverse = -1;         // -1 auto, 1: the force map walks its tiles last-to-first, 0: first-to-last
    int small_system_max_n = kSmallSystemMaxN; // at or below this N: one single-block launch does everything; 0 disables
    int reduce_unroll = -1;       // particles per lane and tile of the reduction: -1 auto, 1 or 2
    int persistent = -1;          // -1 auto, 0 never, 1 whenever the grid is <= 256 blocks: ONE launch per evaluation
    int rho_lane_particle = -1;   // density field mapping: 0 lane = wavevector, 1 / 2 / 3 lane = particle with 25 / 10 / 5
                                  // wavevectors per chunk, -1 auto (lane = particle with 5 where n_k fills the 64-lane
                                  // chunks of the first mapping to less than 3/4)
    int persistent_lds_kb = 0;    // LDS budget per block of the single-launch kernel in KiB (0 = default: all of a CU's usable LDS
                                  // when forced on, half of it when chosen automatically); tiles beyond it are read twice
    int persistent_balanced = -1; // partition of the particles over the blocks of the single-launch kernel: -1 auto, 0 tiles
                                  // dealt round-robin (the two-launch path's partition), 1 contiguous, equal shares
    // single-launch evaluation: granule slab + epoch word (device), see cavmd_persistent_kernel.hpp
    cavmd::DeviceArray<unsigned long long> d_granules;
    cavmd::DeviceArray<unsigned> d_epoch;
    int debug_spin_limit = 0;     // tests: poll rounds of the single-launch kernel's bounded waits (0 = kSpinLimit)
    int debug_late_block = -1;    // tests: this block of the single-launch grid starts debug_late_ticks late (-1 = none)
    int debug_late_ticks = 0;     //        (100 MHz wall clock)
    int debug_silent_block = -1;  // tests: this block never publishes its record: the evaluation cannot be completed (-1 = none)
    int debug_skip_publish = 0;   // tests: the kernels publish into a scratch block instead of the one the host reads -- what a
                                  //        launch that failed on the device looks like from the host
    cavmd::MappedBlock<cavmd::HostResult> h_scratch; // (hooks build only) that scratch block
    // after a starved evaluation the single launch is suspended: until sequence reaches suspend_until, then one probe; every
    // further starvation multiplies the pause by 8 (2^16 evaluations at first, 2^31 at most); a FAILED one suspends for good
    uint64_t suspend_until = 0;
    uint64_t suspend_backoff = kSuspendFirst;
    bool sync_state_dirty = false;  // a starved evaluation may have left records or counts behind: wipe before the next single launch
    bool sync_timeout_seen = false; // an inter-workgroup wait of the single-launch kernel gave up once: two launches from then on
    bool captured = false; // some evaluation was enqueued into a stream capture: the host-side flag protocol is off
    uint64_t captured_from = 0; // sequence of the last evaluation before the first captured one (its block stays in the ring)
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> events; // kEventsPerSlot per slot: start/stop of each of the three kernels
    int pending = 0;
    std::vector<unsigned> slot_mask; // which of the three kernels a slot's evaluation launched
    double acc_ms[3] = {0, 0, 0};
    uint64_t acc_launches = 0;
    std::vector<float> samples; // 3 per evaluation, capped at kMaxSamples evaluations
    // observables (rows f2 / f3)
    size_t n_k = 0;
    unsigned n_chunks = 0;
    unsigned rho_blocks = 0;
    cavmd::DeviceArray<double> d_kvec, d_rho_part, d_rho; // set together with n_k, n_chunks and rho_blocks (cavmd_set_wavevectors)
    cavmd::PinnedBlock<double> h_rho;
    hipStream_t rho_stream = nullptr;
    bool rho_computed = false;
    int rho_last_mapping = -1; // what the last cavmd_density_field call launched: mapping 0..3 after the automatic rule,
    int rho_last_blocks = -1;  // and the grid's x extent, which is also the fold's nblocks (-1: no call yet); read-only tunables
    cavmd::DeviceArray<double> d_mode;
    cavmd::MappedBlock<cavmd::HostMode> h_mode;   // cavity_mode_kernel publishes here
    uint64_t mode_sequence = 0;
    cavmd::DeviceArray<double> d_fm_part; // [2][max_parts] + 1 result
    cavmd::MappedBlock<cavmd::HostScalar> h_fm;  // the scalar reductions publish here, the host spins on `ready`
    uint64_t fm_sequence = 0;
    cavmd::DeviceArray<unsigned> d_fm_ticket; // ticket counter of the one-launch scalar reductions (reset by the folding block)
    // on-device Bussi thermostat (cavmd_bussi_step_device)
    cavmd::DeviceArray<cavmd::BussiDevice> d_bussi;
    cavmd::MappedBlock<cavmd::HostBussi> h_bussi;
    uint64_t bussi_sequence = 0;
    uint64_t bussi_refused_seen = 0;  // refusals already reported to the caller
    hipStream_t bussi_stream = nullptr; // stream of the last enqueued step: the one whose idleness ends a wait for its flag
};

namespace cavmd
{
inline unsigned grid_for(size_t work_items, unsigned tile, int num_cu, int blocks_per_cu)
{
    size_t tiles = (work_items + tile - 1) / tile;
    size_t cap = (size_t)num_cu * (size_t)blocks_per_cu;
    size_t g = tiles < cap ? tiles : cap;
    return (unsigned)(g ? g : 1);
}

// A single-launch evaluation whose blocks were not resident together (other grids held the CUs) either got completed by its
// last block alone (kSyncRepaired: results valid, it just took a second) or failed (kSyncFailed: NaN forces) -- see the
// bail path of cavity_persistent_kernel.  Whoever notices first -- the next enqueue or the result read -- suspends the
// single-launch path for this workspace: what starved the grid is a property of how the GPU is shared at the moment, not of
// one step, and the two-launch path does not depend on residency.  Returns 0 (nothing happened), kSyncRepaired or kSyncFailed.
inline unsigned consume_sync_timeout(cavmd_workspace* ws)
{
    if (!ws->h_ctl.host || !__atomic_load_n(&ws->h_ctl.host->sync_error, __ATOMIC_ACQUIRE))
        return 0;
    // kSyncFailed is provisional while the kernel runs (the first block that gives up raises it, the last one may still
    // complete the evaluation): the verdict is the flag once the stream has drained.  A stream that is being captured cannot
    // be waited for; the provisional value then counts.
    if (!stream_capturing(ws->last_stream))
        (void)hipStreamSynchronize(ws->last_stream);
    const unsigned verdict = __atomic_load_n(&ws->h_ctl.host->sync_error, __ATOMIC_ACQUIRE);
    __atomic_store_n(&ws->h_ctl.host->sync_error, 0u, __ATOMIC_RELEASE);
    ws->sync_timeout_seen = true;
    ws->sync_state_dirty = true;
    if (verdict == kSyncRepaired)
    {
        // two launches for a while, then one probe: whoever held the CUs may have gone.  A probe that starves again costs one
        // slow (valid) evaluation and an 8 times longer pause.
        if (ws->sequence - ws->suspend_until > ws->suspend_backoff)
            ws->suspend_backoff = kSuspendFirst; // the single launch had been healthy for longer than the last pause: start over
        ws->suspend_until = ws->sequence + ws->suspend_backoff;
        ws->suspend_backoff = ws->suspend_backoff * 8 < kSuspendMax ? ws->suspend_backoff * 8 : kSuspendMax;
        return kSyncRepaired;
    }
    ws->suspend_until = kSuspendForever; // not understood: stay off until the caller switches it on again
    ws->computed = false;                // the result block still holds the evaluation BEFORE the failed one
    return kSyncFailed;
}
} // namespace cavmd
