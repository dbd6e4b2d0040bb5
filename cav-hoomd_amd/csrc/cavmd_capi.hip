// cavmd_capi.hip -- implementation of include/cavmd.h on top of the kernels in cavmd_kernels.hpp.
//
// Host side of the replaced reference code: CavityForceComputeGPU::computeForces
// (src/CavityForceComputeGPU.cc:102-253) and kernel::gpu_compute_cavity_force
// (src/CavityForceComputeGPU.cu:507-617).  Where the reference does 4 memsets, 1 H2D and 2 blocking
// D2H copies, a device synchronise and a host scan of the position array per step, this enqueues
// one kernel (two above ~2.4e6 particles) on the caller's stream and returns; the energies reach the host through a
// block of mapped pinned memory that cavmd_energies polls (no copy, no stream synchronisation).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "cavmd.h"
#include "cavmd_kernels.hpp"
#include "cavmd_host_support.hpp" // the capture query, the wait for a stamp, the buffer owners, runtime value -> template argument

using namespace cavmd;

namespace
{
constexpr int kReduceBlock = 256;
constexpr int kReduceUnroll = 2; // particles per lane and tile; 2 beats 4 by 6 % at 1e6 and 11 % at 3e5, ties at 1e7
constexpr int kFinalizeBlock = 256;
constexpr int kMapBlock = 256;
constexpr int kMapUnroll = 4; // 1024 chunks = 512 particles per tile: the SAME particle range as a reduction tile, so with
                              // grids that are multiples of 8 tile t is reduced and mapped on the same XCD (t mod 8)
constexpr int kMaxBlocksPerCU = 16;
constexpr int kEventsPerSlot = 6;
constexpr int kProfileSlots = 512; // evaluations buffered between profile reads
constexpr size_t kMaxSamples = 4096;
constexpr int kSmallBlock = 256;
constexpr int kSmallSystemMaxN = 1024;         // single-block path (one batch of 4 x 256 particles) wins up to ~1000 particles against the
                                               // single-launch kernel: 5.0 vs 6.0 us at N = 501, 6.0 vs 6.0 at 1001, 7.0 vs 6.1 at 1101,
                                               // 7.9 vs 6.2 at 1401 (profiles/r02/ab_small_system.txt)
constexpr size_t kNtStoreMinN = 200000;       // force stores: neutral at 1e5, -3.6 % at 3e5, -4.3 % at 1e6, -5.8 % at 1e7
constexpr size_t kChargeTemporalMaxN = 25000000; // charges stay temporal while the 8 N bytes fit in the 256 MiB Infinity Cache
                                                 // next to the streams: re-measured in round 2 (the round-1 crossover at
                                                 // 5e6 dated from before the scratch-traffic fix): -8 % per evaluation at
                                                 // 6e6 and 1e7, -5 % at 2e7, tie at 5e7 (profiles/r02/ab_two_launch_knobs.txt)
constexpr int kPersistBlock = 256;
constexpr size_t kPersistMaxLds = 156 * 1024; // dynamic LDS of the single-launch kernel (charges of a block's tiles); 160 KiB per CU
constexpr uint64_t kSuspendFirst = 1ull << 16, kSuspendMax = 1ull << 31, kSuspendForever = ~0ull;
constexpr size_t kPersistSharedLds = 76 * 1024; // default ceiling: two such blocks (+ 1.7 KiB static each) fit on one CU, so two concurrent grids stay resident
constexpr unsigned kResultHistory = 64;          // default depth of the result ring ("result_history"): 16 KiB pinned
constexpr unsigned kResultHistoryMax = 16384;

static_assert(sizeof(cavmd_double4) == 32, "Scalar4 layout");
static_assert(sizeof(cavmd_int3) == 12, "int3 layout");
static_assert(sizeof(cavmd_params) == 32, "params layout");
static_assert(sizeof(cavmd_result) == 192, "result layout");

// The fixed part of the workspace's mapped host memory (never reallocated): the starvation flag of the single-launch kernel,
// and the one block every evaluation publishes into once the workspace has been captured (a replay cannot pick a ring slot).
struct HostControl
{
    HostResult fixed;
    unsigned sync_error; // kSyncFailed / kSyncRepaired, raised by a starved single-launch evaluation (consume_sync_timeout)
    unsigned pad[63];
};
} // namespace

struct cavmd_workspace
{
    int device = -1;
    int num_cu = 0;
    char arch[64] = {0};
    size_t max_N = 0;
    unsigned max_parts = 0;
    DeviceArray<double> d_part;
    DeviceArray<int> d_ipart;
    DeviceArray<cavmd_result> d_result;
    MappedBlock<HostResult> h_ring;     // ring_depth result slots; evaluation s publishes into slot s % ring_depth
    unsigned ring_depth = kResultHistory;
    uint64_t history_first = 1;         // oldest sequence the ring can hold (raised when "result_history" reallocates it)
    MappedBlock<HostControl> h_ctl;     // fixed: starvation flag + the block of a captured workspace
    hipStream_t last_stream = nullptr;
    bool computed = false;
    uint64_t sequence = 0;
    // tunables
    // Defaults from interleaved A/B runs on MI355X (csrc/microbench.hip; profiles/r01/microbench_*.txt):
    int reduce_blocks_per_cu = 1; // <= 256 partials: the fused force map folds them with one load per thread
    int map_blocks_per_cu = 2;    // every fused block re-folds the partials, so few, long-lived blocks
    int map_nt_store = -1;        // -1 auto (non-temporal from kNtStoreMinN particles up), 0 plain, 1 non-temporal, 2 write-through
    int reduce_nt_load = -1;      // -1 auto, 0 plain, 1 pos+image non-temporal, 2 all non-temporal
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
    DeviceArray<unsigned long long> d_granules;
    DeviceArray<unsigned> d_epoch;
    int debug_spin_limit = 0;     // tests: poll rounds of the single-launch kernel's bounded waits (0 = kSpinLimit)
    int debug_late_block = -1;    // tests: this block of the single-launch grid starts debug_late_ticks late (-1 = none)
    int debug_late_ticks = 0;     //        (100 MHz wall clock)
    int debug_silent_block = -1;  // tests: this block never publishes its record: the evaluation cannot be completed (-1 = none)
    int debug_skip_publish = 0;   // tests: the kernels publish into a scratch block instead of the one the host reads -- what a
                                  //        launch that failed on the device looks like from the host
    MappedBlock<HostResult> h_scratch; // (hooks build only) that scratch block
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
    DeviceArray<double> d_kvec, d_rho_part, d_rho; // set together with n_k, n_chunks and rho_blocks (cavmd_set_wavevectors)
    PinnedBlock<double> h_rho;
    hipStream_t rho_stream = nullptr;
    bool rho_computed = false;
    int rho_last_mapping = -1; // what the last cavmd_density_field call launched: mapping 0..3 after the automatic rule,
    int rho_last_blocks = -1;  // and the grid's x extent, which is also the fold's nblocks (-1: no call yet); read-only tunables
    DeviceArray<double> d_mode;
    MappedBlock<HostMode> h_mode;   // cavity_mode_kernel publishes here
    uint64_t mode_sequence = 0;
    DeviceArray<double> d_fm_part; // [2][max_parts] + 1 result
    MappedBlock<HostScalar> h_fm;  // the scalar reductions publish here, the host spins on `ready`
    uint64_t fm_sequence = 0;
    DeviceArray<unsigned> d_fm_ticket; // ticket counter of the one-launch scalar reductions (reset by the folding block)
    // on-device Bussi thermostat (cavmd_bussi_step_device)
    DeviceArray<BussiDevice> d_bussi;
    MappedBlock<HostBussi> h_bussi;
    uint64_t bussi_sequence = 0;
    uint64_t bussi_refused_seen = 0;  // refusals already reported to the caller
    hipStream_t bussi_stream = nullptr; // stream of the last enqueued step: the one whose idleness ends a wait for its flag
    unsigned dependents = 0;            // live objects created from this workspace (ItemTable::attach): cavmd_destroy refuses
};

namespace
{
struct DeviceGuard
{
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev)
        {
            switched = (hipSetDevice(dev) == hipSuccess);
        }
    }
    ~DeviceGuard()
    {
        if (switched)
            (void)hipSetDevice(prev);
    }
};

inline int hip_status(hipError_t e)
{
    return e == hipSuccess ? CAVMD_OK : (int)e;
}

#define CAVMD_HIP_TRY(expr)              \
    do                                   \
    {                                    \
        hipError_t _e = (expr);          \
        if (_e != hipSuccess)            \
            return (int)_e;              \
    } while (0)

DeviceParams derive(const cavmd_params* p)
{
    DeviceParams d;
    d.g = p->couplstr;
    d.K = p->K;
    d.gK = p->couplstr / p->K;                   // as `m_params.couplstr / m_params.K`, src/CavityForceCompute.cc:183
    d.g2K = p->couplstr * p->couplstr / p->K;    // as `couplstr * couplstr / K`, :176 (host code is built -ffp-contract=off)
    return d;
}

bool params_ok(const cavmd_params* p)
{
    return p && isfinite(p->omegac) && isfinite(p->couplstr) && isfinite(p->K) && isfinite(p->phmass) && p->K != 0.0;
}

int drain_profile(cavmd_workspace* ws)
{
    for (int s = 0; s < ws->pending; ++s)
    {
        hipEvent_t* ev = &ws->events[kEventsPerSlot * s];
        const unsigned used = ws->slot_mask[s];
        float sample[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k)
        {
            if (!(used & (1u << k)))
                continue;
            CAVMD_HIP_TRY(hipEventSynchronize(ev[2 * k + 1]));
            float ms = 0.f;
            CAVMD_HIP_TRY(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            ws->acc_ms[k] += (double)ms;
            sample[k] = ms;
        }
        ws->acc_launches += 1;
        if (ws->samples.size() >= 3 * kMaxSamples)
            ws->samples.erase(ws->samples.begin(), ws->samples.begin() + 3);
        ws->samples.insert(ws->samples.end(), sample, sample + 3);
    }
    ws->pending = 0;
    return CAVMD_OK;
}

// A captured evaluation carries a frozen `sequence` argument: from the second replay on the host-visible ready flag
// already holds that value, so the flag protocol of cavmd_result_read cannot tell a finished replay from a running one.
// Once a workspace has been captured its results are read behind a device synchronisation instead (include/cavmd.h).
void note_capture(cavmd_workspace* ws, hipStream_t stream)
{
    if (!ws->captured && stream_capturing(stream))
    {
        ws->captured = true;
        ws->captured_from = ws->sequence;
    }
}

// Where the single-launch evaluation is the default (measured on MI355X, profiles/r02/microbench_persistent_*.txt): at
// every N that passes the residency and LDS conditions of plan_evaluation.
constexpr bool kPersistentAuto = true;
// Contiguous equal shares measured SLOWER than tiles dealt round-robin wherever the streaming matters (21.5 vs 20.3 us at
// N = 1e6, 63.8 vs 57.8 at 4e6: 256 sequential streams a fixed distance apart load the HBM channels less evenly than one
// 4 MB window that all blocks sweep together); only 3e5 gained (12.0 vs 12.2).  Kept as a tunable, off.
constexpr bool kPersistentBalancedAuto = false;

unsigned grid_for(size_t work_items, unsigned tile, int num_cu, int blocks_per_cu)
{
    size_t tiles = (work_items + tile - 1) / tile;
    size_t cap = (size_t)num_cu * (size_t)blocks_per_cu;
    size_t g = tiles < cap ? tiles : cap;
    return (unsigned)(g ? g : 1);
}

constexpr int kScaleBlocksPerCu = 4; // velocity rescale: 256-thread blocks per CU (4 particles per lane and tile)
constexpr size_t kTicketBytes = 128;

// Scratch of the scalar reductions (sum |F| / m, kinetic energy): partials + the host-visible scalar + the ticket counter.
int ensure_scalar_scratch(cavmd_workspace* ws)
{
    if (ws->d_fm_part.ptr)
        return CAVMD_OK;
    DeviceArray<double> part;
    MappedBlock<HostScalar> host;
    DeviceArray<unsigned> ticket;
    CAVMD_HIP_TRY(part.alloc(2 * (size_t)ws->max_parts + 1));
    CAVMD_HIP_TRY(host.alloc());
    CAVMD_HIP_TRY(ticket.alloc_zeroed(kTicketBytes / sizeof(unsigned)));
    ws->d_fm_part = std::move(part);
    ws->h_fm = std::move(host);
    ws->d_fm_ticket = std::move(ticket);
    return CAVMD_OK;
}

// Wait for the scalar the fold kernel publishes: about a PCIe write after the kernel has it, instead of a copy plus a stream
// synchronisation.
int wait_scalar(cavmd_workspace* ws, hipStream_t stream, double* out)
{
    const StampWait w = wait_for_stamp(&ws->h_fm.host->ready, ws->fm_sequence, stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
    {
        // the kernel never published (failed or aborted launch): its blocks may have left the ticket counter
        // part-way, after which no block would ever be "last" again -- put it back before reporting
        (void)hipMemsetAsync(ws->d_fm_ticket.ptr, 0, kTicketBytes, stream);
        return (int)hipErrorLaunchFailure;
    }
    *out = ws->h_fm.host->value;
    return CAVMD_OK;
}

// The variants of the kernels the two entry points choose among, by the values their template parameters take.  The launches
// (with_constant) and allow_large_lds (with_each_constant) walk the same lists, so what is launched is what is instantiated.
constexpr IntList<2, 1> kUnrolls;          // particles per lane and tile of the reduction
constexpr IntList<0, 1, 2> kLoadPolicies;  // reduction loads: plain, pos+image non-temporal, all non-temporal
constexpr IntList<2, 1, 0> kStorePolicies; // force stores: write-through, non-temporal, plain

// The single-launch kernel keeps the charges of a block's tiles in dynamic LDS (up to kPersistMaxLds); HIP wants the
// ceiling raised per kernel before a launch may ask for more than 64 KiB.
hipError_t allow_large_lds()
{
    // (per device: called from cavmd_create under its device guard)
    hipError_t once = [] {
        hipError_t e = hipSuccess;
        const auto allow = [&e](auto kernel) {
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kPersistMaxLds);
        };
        with_each_constant(kUnrolls, [&](auto u) {
            with_each_constant(kStorePolicies, [&](auto s) {
                allow(&cavity_persistent_kernel<kPersistBlock, decltype(u)::value, decltype(s)::value>);
            });
        });
#ifdef CAVMD_TEST_HOOKS
        // the fault-injection instantiations (tests: "debug_late_block", "debug_silent_block"; libcavmd_hooks.so only)
        with_each_constant(kUnrolls, [&](auto u) { allow(&cavity_persistent_kernel<kPersistBlock, decltype(u)::value, 0, true>); });
#endif
        return e;
    }();
    return once;
}

// Per-kernel timing for bench.py's roofline leg.  When profiling is on, every kernel is launched through
// hipExtLaunchKernelGGL with its own start/stop events: those take the dispatch packet's begin/end timestamps (what
// rocprofv3 --kernel-trace reports), unlike hipEventRecord markers between kernels, which add ~2.5 us each.
struct LaunchScope
{
    cavmd_workspace* ws;
    hipStream_t stream;
    hipEvent_t* ev = nullptr;
    unsigned used = 0;
    int status = CAVMD_OK;
    LaunchScope(cavmd_workspace* w, hipStream_t s) : ws(w), stream(s)
    {
        if (!ws->profiling)
            return;
        if (ws->pending == kProfileSlots)
            status = drain_profile(ws);
        if (status == CAVMD_OK)
            ev = &ws->events[kEventsPerSlot * ws->pending];
    }
    template <class K, class... Args>
    int launch_lds(int slot, size_t lds_bytes, K kernel, unsigned grid, unsigned block, Args... args)
    {
        if (ev)
        {
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, ev[2 * slot], ev[2 * slot + 1], 0,
                                  args...);
            used |= 1u << slot;
        }
        else
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, args...);
        return hip_status(hipGetLastError());
    }
    template <class K, class... Args>
    int launch(int slot, K kernel, unsigned grid, unsigned block, Args... args)
    {
        return launch_lds(slot, 0, kernel, grid, block, args...);
    }
    void commit()
    {
        if (ev)
        {
            ws->slot_mask[ws->pending] = used;
            ws->pending += 1;
        }
    }
};

// ---- the plan of one evaluation: which kernels, which variants, which grids -------------------------------------------------
// Pure host arithmetic on (N, CU count, tunables); tests/test_gpu_dispatch_matrix.py::dispatch_mirror restates it line for
// line and is checked against what the launches leave behind.  What depends on the workspace's history (a suspended single
// launch, the dirty hand-off slabs, a starved evaluation not yet reported) is the entry point's business, not the plan's.
enum class Layout
{
    aos,    // Scalar4 arrays (cavmd_compute_hoomd)
    strided // per-field strided views (cavmd_compute_soa)
};

enum class Path
{
    single_block,  // cavity_small_system_kernel: one block reduces, finalises and maps
    single_launch, // cavity_persistent_kernel
    two_launches,  // reduction, then a force map that folds the partials itself
    three_launches // reduction, finalize, force map (kept for A/B)
};

struct EvalPlan
{
    Path path = Path::two_launches;
    Path multi_launch = Path::two_launches; // what a suspended single launch falls back to ("fused_finalize")
    int unroll = kReduceUnroll;             // particles per lane and tile of the reduction
    unsigned g1 = 1, g2 = 1;                // grids of the reduction (= number of partials) and of the force map
    int nt_load = 0;                        // load policy of the two-launch reduction (kLoadPolicies)
    int nt_store = 0;                       // store policy of the force map (kStorePolicies)
    unsigned lds_slots = 0;                 // single launch: tiles of a block whose charges stay in LDS,
    size_t lds_bytes = 0;                   //                and the dynamic LDS that takes
    bool balanced = false;                  // single launch: contiguous equal shares instead of tiles dealt round-robin
    bool map_reverse = false;               // the force map walks its tiles last-to-first
};

EvalPlan plan_evaluation(const cavmd_workspace& ws, size_t N, Layout layout)
{
    EvalPlan p;
    p.multi_launch = ws.fused_finalize ? Path::two_launches : Path::three_launches;
    p.path = p.multi_launch;
    // ---- small systems (the reference's own N = 501): one block reduces, finalises and maps in ONE launch
    if (layout == Layout::aos && ws.small_system_max_n > 0 && N <= (size_t)ws.small_system_max_n)
    {
        p.path = Path::single_block;
        return p;
    }
    // Tile depth: 2 particles per lane (512 per block; 8 loads in flight per lane); 1 while that leaves at most about one
    // tile per CU (re-measured with the single-launch kernel: 1 wins by 9 % at N = 5e4 and 4 % at 1.3e5, ties at 1e5,
    // loses by 6 % from 2e5 up: profiles/r02/ab_reduce_unroll.txt).  One rule for both layouts, so that they share one
    // summation tree (and give equal bits).
    p.unroll = kReduceUnroll;
    while (p.unroll > 1 && N / ((size_t)kReduceBlock * p.unroll) < (size_t)ws.num_cu * 5 / 4)
        p.unroll >>= 1;
    if (ws.reduce_unroll == 1 || ws.reduce_unroll == 2)
        p.unroll = ws.reduce_unroll;
    p.g1 = grid_for(N, kReduceBlock * p.unroll, ws.num_cu, ws.reduce_blocks_per_cu);
    if (layout == Layout::strided)
    {
        p.g2 = grid_for(N, kMapBlock * 4, ws.num_cu, ws.map_blocks_per_cu); // the strided map's tile: 4 particles per lane
        return p;
    }
    p.g2 = grid_for(2 * N, kMapBlock * kMapUnroll, ws.num_cu, ws.map_blocks_per_cu);
    // Force stores bypass the caches for all but small N: the array is consumed much later (by the integrator, after
    // every other force of the step), and not leaving 32 N dirty bytes behind shortens this kernel's drain and spares
    // the next reduction the evictions (measured on whole evaluations, profiles/r01/microbench_*.txt).
    p.nt_store = ws.map_nt_store < 0 ? (N >= kNtStoreMinN ? 1 : 0) : ws.map_nt_store;
    // Load policy of the reduction.  pos and image are read once per evaluation: non-temporal.  charge is read again
    // by the force map: keeping it temporal lets the map find it in the Infinity Cache while 8 N bytes fit there
    // (measured per evaluation: -8 % at N = 6e6 and 1e7, -5 % at 2e7, tie at 5e7); non-temporal above.
    p.nt_load = ws.reduce_nt_load < 0 ? (N <= kChargeTemporalMaxN ? 1 : 2) : ws.reduce_nt_load;
    // Reverse tile order in the force map: the charge lines the reduction touched last are then asked for first.  It only
    // matters where the per-XCD share of the charges (N bytes) is about the size of an XCD's 4 MiB L2: -3.3 % per
    // evaluation at N = 4e6, neutral at 3e5 / 1e6 / 2e6 / 1e7 (scripts/ab_tunable.py map_reverse 0 1 ...).
    p.map_reverse = ws.map_reverse < 0 ? (N > 2500000 && N <= 5000000) : (ws.map_reverse != 0);

    // ---- ONE launch (cavmd_persistent_kernel.hpp): the same grid as the reduction; with the strided partition also the
    // same tiles, hence the same partials and (same fold) the same bits as two launches.  Needs the whole grid resident at
    // once: g1 <= CUs x blocks per CU by construction, <= 256 blocks (the two-level all-reduce), LDS and registers admit
    // that many blocks per CU.  The charges of a block's first lds_slots tiles stay in LDS; tiles beyond (N >~ 5e6) are
    // read a second time.
    const size_t tile = (size_t)kReduceBlock * p.unroll;
    p.balanced = ws.persistent_balanced < 0 ? kPersistentBalancedAuto : (ws.persistent_balanced != 0);
    size_t slots;
    if (p.balanced)
    {
        const size_t units = (N + kWave - 1) / kWave;
        slots = (((units + p.g1 - 1) / p.g1) * kWave + tile - 1) / tile; // the largest share, in tiles (ragged one included)
    }
    else
        slots = ((N + tile - 1) / tile + p.g1 - 1) / p.g1;
    size_t budget = kPersistMaxLds / (size_t)ws.reduce_blocks_per_cu - 1024;
    if (ws.persistent_lds_kb > 0 && (size_t)ws.persistent_lds_kb * 1024 < budget)
        budget = (size_t)ws.persistent_lds_kb * 1024;
    const size_t cap_slots = budget / (tile * sizeof(double));
    p.lds_slots = (unsigned)(slots < cap_slots ? slots : cap_slots);
    p.lds_bytes = p.lds_slots * tile * sizeof(double);
    const bool resident = p.g1 <= kMaxPersistGrid && ws.reduce_blocks_per_cu <= 4;
    // auto: only while every tile of a block fits in LDS.  With overflow tiles re-read in the second phase (one block per
    // CU) the kernel loses to two launches: 142 against 137 us at N = 1e7 (profiles/r02/ab_overflow.txt).
    // Nor by default beyond half a CU's LDS per block (N >~ 2.4e6): two such grids from different streams or processes
    // could then not be resident side by side, and two half-resident grids would wait for each other until their
    // bounded spins give up (a loud CAVMD_ERR_SYNC_TIMEOUT, but a failure).  persistent = 1 lifts both limits.
    if (resident
        && (ws.persistent > 0
            || (ws.persistent < 0 && slots <= cap_slots && p.lds_bytes <= kPersistSharedLds && kPersistentAuto)))
        p.path = Path::single_launch;
    return p;
}

// what both entry points do once every launch of an evaluation went through
int evaluation_enqueued(cavmd_workspace* ws, LaunchScope& ls, hipStream_t stream)
{
    ls.commit();
    ws->last_stream = stream;
    ws->computed = true;
    return CAVMD_OK;
}
} // namespace

extern "C"
{

cavmd_params cavmd_make_params(double omegac, double couplstr, double phmass)
{
    cavmd_params p;
    p.omegac = omegac;
    p.couplstr = couplstr;
    p.phmass = phmass;
    p.K = phmass * omegac * omegac; // src/CavityForceCompute.h:41, evaluated left to right
    return p;
}

int cavmd_create(int device, size_t max_N, cavmd_workspace** out_ws)
{
    if (!out_ws)
        return CAVMD_ERR_INVALID_VALUE;
    *out_ws = nullptr;
    if (max_N > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY; // indices travel as int32 (photon_idx), as in the reference
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return CAVMD_ERR_NO_DEVICE;
    if (device < 0)
    {
        if (hipGetDevice(&device) != hipSuccess)
            return CAVMD_ERR_NO_DEVICE;
    }
    if (device >= count)
        return CAVMD_ERR_INVALID_VALUE;

    cavmd_workspace* ws = new (std::nothrow) cavmd_workspace();
    if (!ws)
        return (int)hipErrorOutOfMemory;
    ws->device = device;
    ws->max_N = max_N;
    // deployment-level switch for GPUs shared by several processes (see "persistent" in cavmd.h): CAVMD_PERSISTENT=0|1
    if (const char* env = getenv("CAVMD_PERSISTENT"))
    {
        if (!strcmp(env, "0"))
            ws->persistent = 0;
        else if (!strcmp(env, "1"))
            ws->persistent = 1;
    }
    DeviceGuard guard(device);

    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess)
    {
        delete ws;
        return (int)e;
    }
    ws->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    strncpy(ws->arch, prop.gcnArchName, sizeof(ws->arch) - 1);
    ws->max_parts = (unsigned)(ws->num_cu * kMaxBlocksPerCU);

    e = ws->d_part.alloc((size_t)kNumPartDoubles * ws->max_parts);
    if (e == hipSuccess)
        e = ws->d_ipart.alloc((size_t)kNumPartInts * ws->max_parts);
    if (e == hipSuccess)
        e = ws->d_result.alloc_zeroed(1);
    if (e == hipSuccess) // tag 0 = never valid
        e = ws->d_granules.alloc_zeroed((size_t)2 * kGranulesPerRecord * kMaxPersistGrid);
    if (e == hipSuccess)
        e = ws->d_epoch.alloc(4);
    if (e == hipSuccess)
    {
        const unsigned init[4] = {1u, 0u, 0u, 0u}; // first tag; no block has given up; not poisoned
        e = hipMemcpy(ws->d_epoch.ptr, init, sizeof(init), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = allow_large_lds();
    if (e == hipSuccess)
        e = ws->h_ring.alloc(ws->ring_depth);
    if (e == hipSuccess)
        e = ws->h_ctl.alloc();
    if (e != hipSuccess)
    {
        delete ws; // nobody has seen it: the owners free what was allocated (the guard above is still in place)
        return (int)e;
    }
    *out_ws = ws;
    return CAVMD_OK;
}

int cavmd_destroy(cavmd_workspace* ws)
{
    if (!ws)
        return CAVMD_OK;
    if (ws->dependents != 0) // a thermostat batch, recorder, integrator or force batch outlives nothing of its workspace
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    for (hipEvent_t ev : ws->events)
        (void)hipEventDestroy(ev);
    delete ws; // every buffer is freed by its owner
    return CAVMD_OK;
}

namespace
{
// Where the kernels of evaluation ws->sequence publish the result block for the host: its slot of the ring in mapped host
// memory; once the workspace has been captured, the one fixed block (a replayed kernel keeps the address it was captured
// with, so the ring could not tell replays apart) -- or, in the test-hooks build with "debug_skip_publish" set, a scratch
// block the host never looks at (what a launch that died on the device looks like).
inline HostResult* host_block(cavmd_workspace* ws)
{
#ifdef CAVMD_TEST_HOOKS
    if (ws->debug_skip_publish && ws->h_scratch.dev)
        return ws->h_scratch.dev;
#endif
    if (ws->captured)
        return &ws->h_ctl.dev->fixed;
    return ws->h_ring.dev + ws->sequence % ws->ring_depth;
}

// Host address of evaluation s's slot.
inline HostResult* ring_slot(cavmd_workspace* ws, uint64_t s)
{
    return ws->h_ring.host + s % ws->ring_depth;
}

// The block the synchronous getters read: the last evaluation's slot; on a captured workspace the fixed block, until the
// first evaluation after the capture has published there the slot of the last one before it.
inline HostResult* last_block(cavmd_workspace* ws)
{
    if (ws->captured)
        return __atomic_load_n(&ws->h_ctl.host->fixed.ready, __ATOMIC_ACQUIRE) ? &ws->h_ctl.host->fixed
                                                                               : ring_slot(ws, ws->captured_from);
    return ring_slot(ws, ws->sequence);
}

// A single-launch evaluation whose blocks were not resident together (other grids held the CUs) either got completed by its
// last block alone (kSyncRepaired: results valid, it just took a second) or failed (kSyncFailed: NaN forces) -- see the
// bail path of cavity_persistent_kernel.  Whoever notices first -- the next enqueue or the result read -- suspends the
// single-launch path for this workspace: what starved the grid is a property of how the GPU is shared at the moment, not of
// one step, and the two-launch path does not depend on residency.  Returns 0 (nothing happened), kSyncRepaired or kSyncFailed.
unsigned consume_sync_timeout(cavmd_workspace* ws)
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
} // namespace

int cavmd_compute_hoomd(cavmd_workspace* ws, void* stream_, size_t N, const cavmd_double4* d_pos, const double* d_charge,
                        const cavmd_int3* d_image, double Lx, double Ly, double Lz, int L_typeid,
                        const cavmd_params* params, cavmd_double4* d_force)
{
    // argument validation first, as kernel::gpu_compute_cavity_force does (src/CavityForceComputeGPU.cu:522-532)
    if (!ws || !d_pos || !d_charge || !d_image || !d_force || !params)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)d_pos & 15) || ((uintptr_t)d_force & 15) || ((uintptr_t)d_charge & 7) || ((uintptr_t)d_image & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (N == 0)
        return CAVMD_OK;
    if (N > ws->max_N)
        return CAVMD_ERR_CAPACITY;
    if (!params_ok(params))
        return CAVMD_ERR_BAD_PARAMS;
    // an EARLIER evaluation was starved and nobody read the result since.  Failed (its forces are NaN): report it here,
    // nothing is enqueued by this call.  Repaired: nothing to report.  Either way two launches from now on.
    if (consume_sync_timeout(ws) == kSyncFailed)
        return CAVMD_ERR_SYNC_TIMEOUT;

    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    note_capture(ws, stream);
    LaunchScope ls(ws, stream);
    if (ls.status != CAVMD_OK)
        return ls.status;

    AosInput in;
    in.pos2 = reinterpret_cast<const v2d*>(d_pos);
    in.charge = d_charge;
    in.image = reinterpret_cast<const int*>(d_image);
    Partials part {ws->d_part.ptr, ws->d_ipart.ptr, ws->max_parts};
    const unsigned n = (unsigned)N;
    const DeviceParams dp = derive(params);
    v2d* force2 = reinterpret_cast<v2d*>(d_force);
    cavmd_result* const d_result = ws->d_result.ptr;
    int st;

    EvalPlan plan = plan_evaluation(*ws, N, Layout::aos);
    if (plan.path == Path::single_launch && ws->sequence < ws->suspend_until)
        plan.path = plan.multi_launch; // suspended after a starved evaluation (consume_sync_timeout)

    if (plan.path == Path::single_block)
    {
        ws->sequence += 1;
        st = ls.launch(0, cavity_small_system_kernel<kSmallBlock>, 1u, kSmallBlock, in, n, Lx, Ly, Lz, dp, L_typeid,
                       ws->sequence, d_result, host_block(ws), force2);
        return st != CAVMD_OK ? st : evaluation_enqueued(ws, ls, stream);
    }

    if (plan.path == Path::single_launch)
    {
        if (ws->sync_state_dirty)
        {
            // re-enabled after a starved evaluation: records or give-up counts of that launch must not meet this one
            CAVMD_HIP_TRY(hipMemsetAsync(ws->d_granules.ptr, 0, sizeof(unsigned long long) * 2 * kGranulesPerRecord * kMaxPersistGrid, stream));
            CAVMD_HIP_TRY(hipMemsetAsync(ws->d_epoch.ptr + 1, 0, 2 * sizeof(unsigned), stream)); // give-up count and poison
            ws->sync_state_dirty = false;
        }
        ws->sequence += 1;
        const AosInputT<2> inx {in.pos2, in.charge, in.image};
        const SyncState sync {ws->d_granules.ptr, ws->d_epoch.ptr,
                              ws->debug_spin_limit > 0 ? (unsigned)ws->debug_spin_limit : kSpinLimit, ws->debug_late_block,
                              (unsigned)ws->debug_late_ticks, ws->debug_silent_block, &ws->h_ctl.dev->sync_error};
        const auto launch = [&](auto kernel) {
            return ls.launch_lds(0, plan.lds_bytes, kernel, plan.g1, kPersistBlock, inx, n, Lx, Ly, Lz, dp, L_typeid, sync,
                                 ws->sequence, d_result, host_block(ws), force2, plan.lds_slots, plan.balanced);
        };
#ifdef CAVMD_TEST_HOOKS
        // fault injection (tests): one block starts late -> the grid starves itself and has to be repaired; or one block
        // never publishes -> the evaluation cannot be completed
        if (ws->debug_late_block >= 0 || ws->debug_silent_block >= 0)
            st = with_constant(kUnrolls, plan.unroll, [&](auto u) {
                return launch(&cavity_persistent_kernel<kPersistBlock, decltype(u)::value, 0, true>);
            });
        else
#endif
            st = with_constant(kUnrolls, plan.unroll, [&](auto u) {
                return with_constant(kStorePolicies, plan.nt_store, [&](auto s) {
                    return launch(&cavity_persistent_kernel<kPersistBlock, decltype(u)::value, decltype(s)::value>);
                });
            });
        return st != CAVMD_OK ? st : evaluation_enqueued(ws, ls, stream);
    }

    // ---- launch 1: per-block partial sums + photon search
    st = with_constant(kUnrolls, plan.unroll, [&](auto u) {
        return with_constant(kLoadPolicies, plan.nt_load, [&](auto nt) {
            using Input = AosInputT<decltype(nt)::value>;
            return ls.launch(0, &dipole_partials_kernel<Input, kReduceBlock, decltype(u)::value, false>, plan.g1, kReduceBlock,
                             Input {in.pos2, in.charge, in.image}, n, Lx, Ly, Lz, L_typeid, part);
        });
    });
    if (st != CAVMD_OK)
        return st;

    ws->sequence += 1;
    if (plan.path == Path::two_launches)
    {
        // ---- launch 2 of 2: every force-map block folds the partials itself, block 0 publishes the result block
        st = with_constant(kStorePolicies, plan.nt_store, [&](auto s) {
            return ls.launch(2, &force_map_aos_fused_kernel<kMapBlock, kMapUnroll, decltype(s)::value>, plan.g2, kMapBlock, in, n,
                             plan.g1, Lx, Ly, Lz, dp, L_typeid, part, ws->sequence, d_result, host_block(ws), force2,
                             plan.map_reverse);
        });
    }
    else
    {
        // ---- three-launch variant (kept for A/B): finalize, then a force map that reads the result block
        st = ls.launch(1, finalize_kernel<AosInput, kFinalizeBlock>, 1u, kFinalizeBlock, in, n, plan.g1, Lx, Ly, Lz, dp, part,
                       ws->sequence, d_result, host_block(ws));
        if (st != CAVMD_OK)
            return st;
        const cavmd_result* res = d_result;
        st = with_constant(IntList<1, 0> {}, plan.nt_store != 0, [&](auto nts) {
            return ls.launch(2, &force_map_aos_kernel<kMapBlock, kMapUnroll, decltype(nts)::value != 0>, plan.g2, kMapBlock,
                             d_charge, in.pos2, n, params->couplstr, L_typeid, res, force2);
        });
    }
    return st != CAVMD_OK ? st : evaluation_enqueued(ws, ls, stream);
}

int cavmd_compute_soa(cavmd_workspace* ws, void* stream_, size_t N, const double* d_position, size_t position_stride,
                      const int32_t* d_typeid, size_t typeid_stride, const int32_t* d_image, size_t image_stride,
                      const double* d_charge, size_t charge_stride, double Lx, double Ly, double Lz, int L_typeid,
                      const cavmd_params* params, double* d_force, size_t force_stride, double* d_potential_energy,
                      size_t potential_energy_stride)
{
    if (!ws || !d_position || !d_typeid || !d_image || !d_charge || !d_force || !params)
        return CAVMD_ERR_INVALID_VALUE;
    if (position_stride < 24 || typeid_stride < 4 || image_stride < 12 || charge_stride < 8 || force_stride < 24
        || (d_potential_energy && potential_energy_stride < 8))
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)d_position & 7) || (position_stride & 7) || ((uintptr_t)d_charge & 7) || (charge_stride & 7)
        || ((uintptr_t)d_force & 7) || (force_stride & 7) || ((uintptr_t)d_typeid & 3) || (typeid_stride & 3)
        || ((uintptr_t)d_image & 3) || (image_stride & 3)
        || (d_potential_energy && (((uintptr_t)d_potential_energy & 7) || (potential_energy_stride & 7))))
        return CAVMD_ERR_INVALID_VALUE;
    if (N == 0)
        return CAVMD_OK;
    if (N > ws->max_N)
        return CAVMD_ERR_CAPACITY;
    if (!params_ok(params))
        return CAVMD_ERR_BAD_PARAMS;

    // HOOMD's GPU local snapshot hands out strided VIEWS of its Scalar4 buffers (position = pos[:, :3], typeid = the
    // int in pos.w, force = force4[:, :3], potential_energy = force4[:, 3]).  That is exactly the AoS layout, so the
    // force.Custom route gets the tuned two-launch path.
    {
        const char* p0 = reinterpret_cast<const char*>(d_position);
        const char* f0 = reinterpret_cast<const char*>(d_force);
        if (position_stride == 32 && typeid_stride == 32 && reinterpret_cast<const char*>(d_typeid) == p0 + 24
            && image_stride == 12 && charge_stride == 8 && force_stride == 32 && d_potential_energy
            && potential_energy_stride == 32 && reinterpret_cast<const char*>(d_potential_energy) == f0 + 24
            && !((uintptr_t)p0 & 15) && !((uintptr_t)f0 & 15))
        {
            return cavmd_compute_hoomd(ws, stream_, N, reinterpret_cast<const cavmd_double4*>(d_position), d_charge,
                                       reinterpret_cast<const cavmd_int3*>(d_image), Lx, Ly, Lz, L_typeid, params,
                                       reinterpret_cast<cavmd_double4*>(d_force));
        }
    }

    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    note_capture(ws, stream);
    LaunchScope ls(ws, stream);
    if (ls.status != CAVMD_OK)
        return ls.status;

    StridedInput in;
    in.pos = reinterpret_cast<const char*>(d_position);
    in.tid = reinterpret_cast<const char*>(d_typeid);
    in.img = reinterpret_cast<const char*>(d_image);
    in.chg = reinterpret_cast<const char*>(d_charge);
    in.pos_stride = position_stride;
    in.tid_stride = typeid_stride;
    in.img_stride = image_stride;
    in.chg_stride = charge_stride;
    Partials part {ws->d_part.ptr, ws->d_ipart.ptr, ws->max_parts};
    const unsigned n = (unsigned)N;
    const DeviceParams dp = derive(params);
    cavmd_result* const d_result = ws->d_result.ptr;

    const EvalPlan plan = plan_evaluation(*ws, N, Layout::strided);
    int st = with_constant(kUnrolls, plan.unroll, [&](auto u) {
        return ls.launch(0, &dipole_partials_kernel<StridedInput, kReduceBlock, decltype(u)::value, false>, plan.g1, kReduceBlock,
                         in, n, Lx, Ly, Lz, L_typeid, part);
    });
    if (st != CAVMD_OK)
        return st;
    ws->sequence += 1;
    char* f_out = reinterpret_cast<char*>(d_force);
    char* pe_out = reinterpret_cast<char*>(d_potential_energy);
    if (plan.path == Path::two_launches)
    {
        st = ls.launch(2, force_map_strided_fused_kernel<kMapBlock>, plan.g2, kMapBlock, in, n, plan.g1, Lx, Ly, Lz, dp, L_typeid,
                       part, ws->sequence, d_result, host_block(ws), f_out, force_stride, pe_out, potential_energy_stride);
    }
    else
    {
        st = ls.launch(1, finalize_kernel<StridedInput, kFinalizeBlock>, 1u, kFinalizeBlock, in, n, plan.g1, Lx, Ly, Lz, dp, part,
                       ws->sequence, d_result, host_block(ws));
        if (st != CAVMD_OK)
            return st;
        const cavmd_result* res = d_result;
        st = ls.launch(2, force_map_strided_kernel<kMapBlock>, plan.g2, kMapBlock, in, n, params->couplstr, L_typeid, res, f_out,
                       force_stride, pe_out, potential_energy_stride);
    }
    return st != CAVMD_OK ? st : evaluation_enqueued(ws, ls, stream);
}

int cavmd_result_read(cavmd_workspace* ws, cavmd_result* out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->computed)
        return CAVMD_ERR_NOT_COMPUTED;
    DeviceGuard guard(ws->device);
    bool published = true;
    if (ws->captured)
    {
        // graph replays: the flag cannot be trusted (frozen sequence) and the replay stream is unknown -> wait for the device
        CAVMD_HIP_TRY(hipDeviceSynchronize());
    }
    else
    {
        // The publishing block stores the result block and then a sequence flag (system-scope release) into mapped pinned
        // host memory.  Spin on that flag: the energies arrive as soon as the block that computes the scalars has them,
        // about a PCIe write after, instead of a stream synchronisation (~15 us).  The stream going idle ends the wait as
        // well (a failed launch, or a timed-out single-launch kernel, never sets the flag).
        const StampWait w = wait_for_stamp(&ring_slot(ws, ws->sequence)->ready, ws->sequence, ws->last_stream);
        if (w.error != hipSuccess)
            return (int)w.error;
        published = w.arrived;
    }
    // A starved evaluation that failed (NaN forces): the result block still holds the PREVIOUS evaluation, which is
    // invalidated so that a second read reports "nothing computed" instead of handing that out as if it were current.
    // One that its last block completed has published its result like any other.
    if (consume_sync_timeout(ws) == kSyncFailed)
        return CAVMD_ERR_SYNC_TIMEOUT;
    if (!published)
    {
        // the stream is idle and the flag does not carry this evaluation's sequence: its launch failed on the device.  The
        // block in host memory belongs to an EARLIER evaluation: not handed out, and invalidated (as wait_scalar does for the
        // scalar reductions)
        ws->computed = false;
        return (int)hipErrorLaunchFailure;
    }
    memcpy(out, &last_block(ws)->result, sizeof(cavmd_result));
    return CAVMD_OK;
}

int cavmd_energies(cavmd_workspace* ws, double out[3])
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->computed)
    {
        // the reference's getters return the 0.0 its constructor stored (src/CavityForceCompute.cc:33-36)
        out[0] = out[1] = out[2] = 0.0;
        return CAVMD_OK;
    }
    cavmd_result r;
    int st = cavmd_result_read(ws, &r);
    if (st != CAVMD_OK)
        return st;
    out[0] = r.energy[0];
    out[1] = r.energy[1];
    out[2] = r.energy[2];
    return CAVMD_OK;
}

int cavmd_last_sequence(cavmd_workspace* ws, uint64_t* out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = ws->sequence;
    return CAVMD_OK;
}

// Result of evaluation `sequence`, read from its own slot of the ring: waits for THAT evaluation only, so a tracker can
// enqueue step k and read step k - 1 while step k keeps the GPU busy.  No seqlock: slot s % depth is reused only by the
// enqueue of evaluation s + depth, which this (one) host thread would have to make itself, and the range check below
// refuses every s whose slot that enqueue has already handed out.
int cavmd_result_at(cavmd_workspace* ws, uint64_t sequence, cavmd_result* out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    if (ws->sequence == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    if (ws->captured) // replays publish into one fixed block under their frozen sequence: no history to read
        return CAVMD_ERR_INVALID_VALUE;
    const uint64_t last = ws->sequence;
    if (sequence == 0 || sequence > last)
        return CAVMD_ERR_INVALID_VALUE;
    if (sequence < ws->history_first || last - sequence >= ws->ring_depth)
        return CAVMD_ERR_EXPIRED;
    DeviceGuard guard(ws->device);
    const HostResult* h = ring_slot(ws, sequence);
    // The evaluation is over once a LATER one has published (the stream runs them in order) or the stream is idle.
    // Never a stream synchronisation, and never the workspace-wide starvation flag: either would wait behind newer
    // evaluations (a starved one among them can take a third of a second).
    const StampWait w = wait_for_stamp(&h->ready, sequence, ws->last_stream, [&] {
        for (uint64_t j = sequence + 1; j <= last; ++j)
            if (__atomic_load_n(&ring_slot(ws, j)->ready, __ATOMIC_ACQUIRE) == j)
                return true;
        return false;
    });
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
    {
        // over, and its slot does not carry it: a starved single-launch evaluation that could not be completed tagged its
        // slot with its own sequence; anything else is a launch that died on the device.  Never an earlier occupant's block.
        const uint64_t failed = __atomic_load_n(&h->failed, __ATOMIC_ACQUIRE);
        return failed == ((sequence << 2) | kSyncFailed) ? CAVMD_ERR_SYNC_TIMEOUT : (int)hipErrorLaunchFailure;
    }
    memcpy(out, &h->result, sizeof(cavmd_result));
    return CAVMD_OK;
}

int cavmd_energies_at(cavmd_workspace* ws, uint64_t sequence, double out[3])
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    cavmd_result r;
    const int st = cavmd_result_at(ws, sequence, &r);
    if (st != CAVMD_OK)
        return st;
    out[0] = r.energy[0];
    out[1] = r.energy[1];
    out[2] = r.energy[2];
    return CAVMD_OK;
}

int cavmd_result_device_ptr(cavmd_workspace* ws, const cavmd_result** out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = ws->d_result.ptr;
    return CAVMD_OK;
}

int cavmd_set_wavevectors(cavmd_workspace* ws, size_t n_k, const double* h_wavevectors)
{
    if (!ws || !h_wavevectors || n_k == 0 || n_k > (size_t)1 << 20)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    // the old set goes first (its memory may be what the new one needs); from here to the commit the workspace has none
    ws->d_kvec.free();
    ws->d_rho_part.free();
    ws->d_rho.free();
    ws->h_rho.free();
    ws->rho_computed = false;
    ws->n_k = 0;
    const unsigned n_chunks = (unsigned)((n_k + kWave - 1) / kWave);
    const unsigned rho_blocks = (unsigned)ws->num_cu * 4; // capacity of the partial buffer: three 256-thread blocks per CU (lane =
                                                          // particle mapping) or one 1024-thread block per CU (lane = wavevector)
    DeviceArray<double> kvec, rho_part, rho;
    PinnedBlock<double> h_rho;
    CAVMD_HIP_TRY(kvec.alloc(3 * n_k));
    CAVMD_HIP_TRY(rho_part.alloc(2 * kWave * (size_t)n_chunks * rho_blocks));
    CAVMD_HIP_TRY(rho.alloc(2 * n_k));
    CAVMD_HIP_TRY(h_rho.alloc(2 * n_k));
    CAVMD_HIP_TRY(hipMemcpy(kvec.ptr, h_wavevectors, sizeof(double) * 3 * n_k, hipMemcpyHostToDevice));
    ws->d_kvec = std::move(kvec);
    ws->d_rho_part = std::move(rho_part);
    ws->d_rho = std::move(rho);
    ws->h_rho = std::move(h_rho);
    ws->n_k = n_k;
    ws->n_chunks = n_chunks;
    ws->rho_blocks = rho_blocks;
    return CAVMD_OK;
}

int cavmd_density_field(cavmd_workspace* ws, void* stream_, size_t N, const double* d_position, size_t position_stride)
{
    if (!ws || !d_position || position_stride < 24 || (position_stride & 7) || ((uintptr_t)d_position & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (ws->n_k == 0)
        return CAVMD_ERR_NOT_COMPUTED; // no wavevectors stored yet
    if (N > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    constexpr int kBlock = 1024;
    const size_t tiles = (N + kWave - 1) / kWave;
    unsigned gb;
    // lane = wavevector costs ceil(n_k / 64) * 64 lane-slots per particle, lane = particle n_k slots that measured 1.33x
    // as expensive each (N = 1e6: n_k = 17: 53 vs 87 us, 50: 99 vs 95, 64: 118 vs 88, 100: 170 vs 165)
    int lp = ws->rho_lane_particle;
    if (lp < 0)
        lp = (ws->n_k * 4 < (size_t)ws->n_chunks * kWave * 3) ? 3 : 0;
    if (lp)
    {
        // lane = particle: 256-thread blocks, KC wavevectors per chunk (2 KC running sums per lane in registers)
        constexpr int kLpBlock = 256;
        size_t g = (tiles + (kLpBlock / kWave) - 1) / (kLpBlock / kWave);
        if (g > ws->rho_blocks)
            g = ws->rho_blocks;
        gb = (unsigned)(g ? g : 1);
        with_constant(IntList<25, 10, 5> {}, lp == 1 ? 25 : lp == 2 ? 10 : 5, [&](auto kc) {
            constexpr int KC = decltype(kc)::value; // wavevectors per chunk
            hipLaunchKernelGGL((density_partials_lp_kernel<kLpBlock, KC>), dim3(gb, (unsigned)((ws->n_k + KC - 1) / KC)),
                               dim3(kLpBlock), 0, stream, reinterpret_cast<const char*>(d_position), position_stride, (unsigned)N,
                               ws->d_kvec.ptr, (unsigned)ws->n_k, make_sincos_coef(), ws->d_rho_part.ptr);
        });
    }
    else
    {
        size_t g = (tiles + (kBlock / kWave) - 1) / (kBlock / kWave);
        if (g > (size_t)ws->num_cu)
            g = (size_t)ws->num_cu;
        gb = (unsigned)(g ? g : 1);
        hipLaunchKernelGGL((density_partials_kernel<kBlock>), dim3(gb, ws->n_chunks), dim3(kBlock), 0, stream,
                           reinterpret_cast<const char*>(d_position), position_stride, (unsigned)N, ws->d_kvec.ptr,
                           (unsigned)ws->n_k, make_sincos_coef(), ws->d_rho_part.ptr);
    }
    CAVMD_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((density_fold_kernel<kBlock>), dim3(ws->n_chunks), dim3(kBlock), 0, stream, ws->d_rho_part.ptr,
                       gb, (unsigned)ws->n_k, ws->d_rho.ptr);
    CAVMD_HIP_TRY(hipGetLastError());
    ws->rho_stream = stream;
    ws->rho_computed = true;
    ws->rho_last_mapping = lp;
    ws->rho_last_blocks = (int)gb;
    return CAVMD_OK;
}

int cavmd_density_field_read(cavmd_workspace* ws, double* h_out)
{
    if (!ws || !h_out)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->rho_computed)
        return CAVMD_ERR_NOT_COMPUTED;
    DeviceGuard guard(ws->device);
    CAVMD_HIP_TRY(hipMemcpyAsync(ws->h_rho.host, ws->d_rho.ptr, sizeof(double) * 2 * ws->n_k, hipMemcpyDeviceToHost, ws->rho_stream));
    CAVMD_HIP_TRY(hipStreamSynchronize(ws->rho_stream));
    memcpy(h_out, ws->h_rho.host, sizeof(double) * 2 * ws->n_k);
    return CAVMD_OK;
}

int cavmd_cavity_mode(cavmd_workspace* ws, void* stream_, const cavmd_double4* d_vel, double kB, double out[4])
{
    if (!ws || !d_vel || !out || !(kB > 0.0) || ((uintptr_t)d_vel & 15))
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->computed)
        return CAVMD_ERR_NOT_COMPUTED;
    // the photon index and E_h are read from the last evaluation's device-side result: if that evaluation was starved and
    // could not be completed, the block on the device still belongs to the evaluation BEFORE it -> say so instead
    if (consume_sync_timeout(ws) == kSyncFailed)
        return CAVMD_ERR_SYNC_TIMEOUT;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    if (!ws->d_mode.ptr)
    {
        DeviceArray<double> mode;
        MappedBlock<HostMode> host;
        CAVMD_HIP_TRY(mode.alloc(4));
        CAVMD_HIP_TRY(host.alloc());
        ws->d_mode = std::move(mode);
        ws->h_mode = std::move(host);
    }
    const cavmd_result* res = ws->d_result.ptr;
    ws->mode_sequence += 1;
    hipLaunchKernelGGL(cavity_mode_kernel, dim3(1), dim3(1), 0, stream, res, d_vel, kB, ws->d_mode.ptr, ws->h_mode.dev,
                       ws->mode_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    const StampWait w = wait_for_stamp(&ws->h_mode.host->ready, ws->mode_sequence, stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
        return (int)hipErrorLaunchFailure;
    for (int k = 0; k < 4; ++k)
        out[k] = ws->h_mode.host->v[k];
    return CAVMD_OK;
}

int cavmd_force_mass_sum(cavmd_workspace* ws, void* stream_, size_t N, const cavmd_double4* d_net_force,
                         const cavmd_double4* d_vel, double* out)
{
    if (!ws || !d_net_force || !d_vel || !out || ((uintptr_t)d_net_force & 15) || ((uintptr_t)d_vel & 15))
        return CAVMD_ERR_INVALID_VALUE;
    if (N > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (N == 0)
    {
        *out = 0.0;
        return CAVMD_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    {
        const int st0 = ensure_scalar_scratch(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = 256, kUnroll = 4;
    // one block per CU: every block draws a ticket from ONE counter (~12 ns each, serialised at the memory side); with four
    // blocks per CU the 1024 tickets alone took 12 us
    const unsigned g = grid_for(N, kBlock * kUnroll, ws->num_cu, 1);
    double* d_out = ws->d_fm_part.ptr + 2 * (size_t)ws->max_parts;
    ws->fm_sequence += 1;
    hipLaunchKernelGGL((force_mass_fused_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_net_force), reinterpret_cast<const v2d*>(d_vel), (unsigned)N,
                       ws->d_fm_part.ptr, ws->d_fm_ticket.ptr, d_out, ws->h_fm.dev, ws->fm_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    return wait_scalar(ws, stream, out);
}

int cavmd_kinetic_energy(cavmd_workspace* ws, void* stream_, const cavmd_double4* d_vel, const uint32_t* d_members,
                         size_t n_members, double* out)
{
    if (!ws || !d_vel || !out || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (n_members == 0)
    {
        *out = 0.0;
        return CAVMD_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    {
        const int st0 = ensure_scalar_scratch(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = 256, kUnroll = 4;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, 1); // one ticket per CU, see cavmd_force_mass_sum
    double* d_out = ws->d_fm_part.ptr + 2 * (size_t)ws->max_parts;
    ws->fm_sequence += 1;
    hipLaunchKernelGGL((kinetic_fused_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr,
                       ws->d_fm_ticket.ptr, d_out, ws->h_fm.dev, ws->fm_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    return wait_scalar(ws, stream, out);
}

int cavmd_scale_velocities(cavmd_workspace* ws, void* stream_, cavmd_double4* d_vel, const uint32_t* d_members,
                           size_t n_members, double alpha)
{
    if (!ws || !d_vel || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (n_members == 0)
        return CAVMD_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    constexpr int kBlock = 256, kUnroll = 4;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, kScaleBlocksPerCu);
    hipLaunchKernelGGL((scale_velocities_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream, reinterpret_cast<v2d*>(d_vel),
                       d_members, (unsigned)n_members, alpha);
    return hip_status(hipGetLastError());
}

// ---- Bussi reservoir thermostat: the scalar rule (host arithmetic; the file is built with -ffp-contract=off) ---------
int cavmd_bussi_rescale_factor(double K, double degrees_of_freedom, double deltaT, double set_T, double tau,
                               double normal_variate, double gamma_variate, double* alpha)
{
    if (!alpha)
        return CAVMD_ERR_INVALID_VALUE;
    // src/BussiReservoirThermostat.h:186-190  c = exp(-dt / tau), 0 for tau == 0 (instantaneous thermalisation); the rest of
    // the rule (:183-213) is bussi_alpha_from_c, the function the on-device step runs too
    const double c = (tau != 0.0) ? exp(-deltaT / tau) : 0.0;
    *alpha = bussi_alpha_from_c(K, degrees_of_freedom, c, set_T, normal_variate, gamma_variate);
    return CAVMD_OK;
}

int cavmd_bussi_step(cavmd_bussi_reservoir* state, double K_translational, double dof_translational, double K_rotational,
                     double dof_rotational, double deltaT, double set_T, double tau, const double variates[4],
                     double factors[2])
{
    if (!state || !variates || !factors)
        return CAVMD_ERR_INVALID_VALUE;
    // src/BussiReservoirThermostat.h:45-48
    if (deltaT == 0.0)
    {
        factors[0] = factors[1] = 1.0;
        return CAVMD_OK;
    }
    // :57-61 "Bussi thermostat requires non-zero initial momenta."
    if ((dof_translational != 0 && K_translational == 0) || (dof_rotational != 0 && K_rotational == 0))
        return CAVMD_ERR_BAD_PARAMS;
    double at = 1.0, ar = 1.0;
    (void)cavmd_bussi_rescale_factor(K_translational, dof_translational, deltaT, set_T, tau, variates[0], variates[1], &at);
    (void)cavmd_bussi_rescale_factor(K_rotational, dof_rotational, deltaT, set_T, tau, variates[2], variates[3], &ar);
    // :86-95  energy handed to the reservoir = KE_old - KE_new = KE_old (1 - alpha^2)
    const double delta_t = K_translational * (1.0 - at * at);
    const double delta_r = K_rotational * (1.0 - ar * ar);
    state->reservoir_translational += delta_t;
    state->reservoir_rotational += delta_r;
    state->instantaneous_translational = delta_t;
    state->instantaneous_rotational = delta_r;
    factors[0] = at;
    factors[1] = ar;
    return CAVMD_OK;
}

namespace
{
int ensure_bussi_state(cavmd_workspace* ws)
{
    if (ws->d_bussi.ptr)
        return CAVMD_OK;
    DeviceArray<BussiDevice> state;
    MappedBlock<HostBussi> host;
    CAVMD_HIP_TRY(state.alloc_zeroed(1));
    CAVMD_HIP_TRY(host.alloc());
    ws->d_bussi = std::move(state);
    ws->h_bussi = std::move(host);
    return CAVMD_OK;
}
} // namespace

int cavmd_bussi_step_device(cavmd_workspace* ws, void* stream_, cavmd_double4* d_vel, const uint32_t* d_members,
                            size_t n_members, double dof_translational, double deltaT, double set_T, double tau,
                            double normal_variate, double gamma_variate)
{
    if (!ws || !d_vel || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    hipStream_t stream = (hipStream_t)stream_;
    // The variates, c, set_T and dof travel by value in BussiStepArgs: a captured step would apply the same R and gamma on
    // every replay (a thermostat that is no longer stochastic).  Refused before anything is allocated, enqueued or counted.
    // A capture query that fails refuses too.
    if (capture_state(stream) != Capture::none)
        return CAVMD_ERR_INVALID_VALUE;
    if (deltaT == 0.0 || n_members == 0) // src/BussiReservoirThermostat.h:45-48: factors {1, 1}, counters untouched
        return CAVMD_OK;
    DeviceGuard guard(ws->device);
    {
        int st0 = ensure_scalar_scratch(ws);
        if (st0 == CAVMD_OK)
            st0 = ensure_bussi_state(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = 256, kUnroll = 4;
    BussiStepArgs a;
    a.dof = dof_translational;
    a.c = (tau != 0.0) ? exp(-deltaT / tau) : 0.0; // :186-190
    a.set_T = set_T;
    a.normal_variate = normal_variate;
    a.gamma_variate = gamma_variate;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, 1);
    ws->bussi_sequence += 1;
    ws->bussi_stream = stream;
    hipLaunchKernelGGL((kinetic_partials_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr);
    CAVMD_HIP_TRY(hipGetLastError());
    const unsigned g2 = grid_for(n_members, kBlock * kUnroll, ws->num_cu, kScaleBlocksPerCu);
    hipLaunchKernelGGL((bussi_rescale_fused_kernel<kBlock, kUnroll>), dim3(g2), dim3(kBlock), 0, stream,
                       reinterpret_cast<v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr, g, a, ws->d_bussi.ptr,
                       ws->h_bussi.dev, ws->bussi_sequence);
    return hip_status(hipGetLastError());
}

int cavmd_bussi_device_read(cavmd_workspace* ws, cavmd_bussi_device_state* out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    memset(out, 0, sizeof(*out));
    if (!ws->d_bussi.ptr || ws->bussi_sequence == 0)
        return CAVMD_OK;
    DeviceGuard guard(ws->device);
    // (on the stream the last step went to, whatever stream the caller is on now)
    const StampWait w = wait_for_stamp(&ws->h_bussi.host->ready, ws->bussi_sequence, ws->bussi_stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
        return (int)hipErrorLaunchFailure; // a launch that never published
    const BussiDevice s = ws->h_bussi.host->state;
    out->reservoir_translational = s.reservoir;
    out->instantaneous_translational = s.instantaneous;
    out->last_alpha = s.alpha;
    out->last_kinetic_energy = s.kinetic;
    out->steps = s.steps;
    out->refused = s.errors;
    if (s.errors != ws->bussi_refused_seen)
    {
        ws->bussi_refused_seen = s.errors;
        return CAVMD_ERR_BAD_PARAMS; // "Bussi thermostat requires non-zero initial momenta."
    }
    return CAVMD_OK;
}

int cavmd_bussi_device_reset(cavmd_workspace* ws, void* stream_)
{
    if (!ws)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->d_bussi.ptr)
        return CAVMD_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    // wait for the last step's publication first so that the host copy can be reset consistently
    cavmd_bussi_device_state unused;
    const int st = cavmd_bussi_device_read(ws, &unused);
    if (st != CAVMD_OK && st != CAVMD_ERR_BAD_PARAMS)
        return st;
    CAVMD_HIP_TRY(hipMemsetAsync(ws->d_bussi.ptr, 0, sizeof(BussiDevice), stream));
    memset(&ws->h_bussi.host->state, 0, sizeof(BussiDevice));
    ws->bussi_refused_seen = 0;
    return CAVMD_OK;
}

int cavmd_profile_enable(cavmd_workspace* ws, int on)
{
    if (!ws)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    if (on && ws->events.empty())
    {
        ws->events.resize(kEventsPerSlot * kProfileSlots);
        ws->slot_mask.assign(kProfileSlots, 0);
        for (size_t i = 0; i < ws->events.size(); ++i)
        {
            hipError_t e = hipEventCreate(&ws->events[i]);
            if (e != hipSuccess)
            {
                for (size_t j = 0; j < i; ++j)
                    (void)hipEventDestroy(ws->events[j]);
                ws->events.clear();
                return (int)e;
            }
        }
    }
    if (!on && ws->pending)
    {
        int st = drain_profile(ws);
        if (st != CAVMD_OK)
            return st;
    }
    ws->profiling = on != 0;
    return CAVMD_OK;
}

int cavmd_profile_read(cavmd_workspace* ws, double ms[3], uint64_t* launches)
{
    if (!ws || !ms || !launches)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    int st = drain_profile(ws);
    if (st != CAVMD_OK)
        return st;
    for (int k = 0; k < 3; ++k)
    {
        ms[k] = ws->acc_ms[k];
        ws->acc_ms[k] = 0.0;
    }
    *launches = ws->acc_launches;
    ws->acc_launches = 0;
    ws->samples.clear();
    return CAVMD_OK;
}

int cavmd_profile_samples(cavmd_workspace* ws, double* out, size_t cap, size_t* n)
{
    if (!ws || !out || !n)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    int st = drain_profile(ws);
    if (st != CAVMD_OK)
        return st;
    const size_t have = ws->samples.size() / 3;
    const size_t take = have < cap ? have : cap;
    const size_t first = have - take;
    for (size_t i = 0; i < 3 * take; ++i)
        out[i] = (double)ws->samples[3 * first + i];
    *n = take;
    return CAVMD_OK;
}

namespace
{
// "result_history": a new ring of `depth` slots.  The stream is drained first (no kernel may still publish into the old
// ring); the last evaluation's block moves to its slot of the new ring, so the synchronous getters keep returning it, and
// every earlier sequence expires.
int resize_history(cavmd_workspace* ws, unsigned depth)
{
    if (stream_capturing(ws->last_stream))
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    if (ws->sequence)
        CAVMD_HIP_TRY(hipStreamSynchronize(ws->last_stream));
    MappedBlock<HostResult> ring;
    CAVMD_HIP_TRY(ring.alloc(depth));
    const uint64_t keep = ws->captured ? ws->captured_from : ws->sequence;
    if (keep)
        memcpy(ring.host + keep % depth, ring_slot(ws, keep), sizeof(HostResult));
    ws->h_ring = std::move(ring); // frees the old ring
    ws->ring_depth = depth;
    ws->history_first = ws->sequence ? ws->sequence : 1;
    return CAVMD_OK;
}

// The plain integer tunables: a name, the member it sets and the values it accepts (lo..hi); cavmd_set_tunable and
// cavmd_get_tunable both walk this table.  Whatever does more than store a checked int is spelled out in the two functions.
struct TunableRow
{
    const char* name;
    int cavmd_workspace::*member;
    int lo, hi;
};
const TunableRow kTunables[] = {
    {"reduce_blocks_per_cu", &cavmd_workspace::reduce_blocks_per_cu, 1, kMaxBlocksPerCU},
    {"map_blocks_per_cu", &cavmd_workspace::map_blocks_per_cu, 1, kMaxBlocksPerCU},
    {"map_nt_store", &cavmd_workspace::map_nt_store, -1, 2},
    {"reduce_nt_load", &cavmd_workspace::reduce_nt_load, -1, 2},
    {"fused_finalize", &cavmd_workspace::fused_finalize, 0, 1},
    {"map_reverse", &cavmd_workspace::map_reverse, -1, 1},
    {"small_system_max_n", &cavmd_workspace::small_system_max_n, 0, 1 << 20},
    {"rho_lane_particle", &cavmd_workspace::rho_lane_particle, -1, 3},
    {"persistent_lds_kb", &cavmd_workspace::persistent_lds_kb, 0, 156},
    {"persistent_balanced", &cavmd_workspace::persistent_balanced, -1, 1},
#ifdef CAVMD_TEST_HOOKS
    {"debug_spin_limit", &cavmd_workspace::debug_spin_limit, 0, INT_MAX},
    {"debug_late_block", &cavmd_workspace::debug_late_block, -1, (int)kMaxPersistGrid - 1},
    {"debug_late_ticks", &cavmd_workspace::debug_late_ticks, 0, 100000000}, // at most one second
    {"debug_silent_block", &cavmd_workspace::debug_silent_block, -1, (int)kMaxPersistGrid - 1},
#endif
};

const TunableRow* find_tunable(const char* name)
{
    for (const TunableRow& row : kTunables)
        if (!strcmp(name, row.name))
            return &row;
    return nullptr;
}
} // namespace

int cavmd_set_tunable(cavmd_workspace* ws, const char* name, int value)
{
    if (!ws || !name)
        return CAVMD_ERR_INVALID_VALUE;
    if (const TunableRow* row = find_tunable(name))
    {
        if (value < row->lo || value > row->hi)
            return CAVMD_ERR_INVALID_VALUE;
        ws->*(row->member) = value;
        return CAVMD_OK;
    }
    if (!strcmp(name, "result_history"))
    {
        if (value < 2 || value > (int)kResultHistoryMax)
            return CAVMD_ERR_INVALID_VALUE;
        return resize_history(ws, (unsigned)value);
    }
    if (!strcmp(name, "persistent"))
    {
        if (value < -1 || value > 1)
            return CAVMD_ERR_INVALID_VALUE;
        ws->persistent = value;
        ws->suspend_until = 0; // the caller's word ends a suspension (the hand-off slabs are wiped before the next single launch)
        ws->suspend_backoff = kSuspendFirst;
        return CAVMD_OK;
    }
    if (!strcmp(name, "reduce_unroll"))
    {
        if (value != -1 && value != 1 && value != 2)
            return CAVMD_ERR_INVALID_VALUE;
        ws->reduce_unroll = value;
        return CAVMD_OK;
    }
#ifdef CAVMD_TEST_HOOKS
    if (!strcmp(name, "debug_suspend_first"))
    {
        if (value < 1)
            return CAVMD_ERR_INVALID_VALUE;
        ws->suspend_backoff = (uint64_t)value;
        return CAVMD_OK;
    }
    if (!strcmp(name, "debug_skip_publish"))
    {
        if (value < 0 || value > 1)
            return CAVMD_ERR_INVALID_VALUE;
        if (value && !ws->h_scratch.host)
        {
            DeviceGuard guard(ws->device);
            CAVMD_HIP_TRY(ws->h_scratch.alloc()); // one owner: there, or empty
        }
        ws->debug_skip_publish = value;
        return CAVMD_OK;
    }
#endif
    if (!strcmp(name, "sync_timeout_seen"))
    {
        // 0 forgets a time-out seen earlier.  In the test-hooks build also a fault-injection hook: raises the flag of the
        // host-visible block as a starved single-launch kernel would -- 1: the evaluation failed, 2: its last block completed it
#ifdef CAVMD_TEST_HOOKS
        if (value < 0 || value > 2)
            return CAVMD_ERR_INVALID_VALUE;
        if (value)
            __atomic_store_n(&ws->h_ctl.host->sync_error, value == 2 ? kSyncRepaired : kSyncFailed, __ATOMIC_RELEASE);
        else
            ws->sync_timeout_seen = false;
#else
        if (value != 0) // raising the flag is a fault-injection hook: libcavmd_hooks.so only
            return CAVMD_ERR_INVALID_VALUE;
        ws->sync_timeout_seen = false;
#endif
        return CAVMD_OK;
    }
    return CAVMD_ERR_INVALID_VALUE;
}

int cavmd_get_tunable(cavmd_workspace* ws, const char* name, int* value)
{
    if (!ws || !name || !value)
        return CAVMD_ERR_INVALID_VALUE;
    if (const TunableRow* row = find_tunable(name))
        *value = ws->*(row->member);
    else if (!strcmp(name, "result_history"))
        *value = (int)ws->ring_depth;
    else if (!strcmp(name, "persistent"))
        *value = ws->persistent;
    else if (!strcmp(name, "reduce_unroll"))
        *value = ws->reduce_unroll;
    else if (!strcmp(name, "sync_timeout_seen"))
        *value = ws->sync_timeout_seen ? 1 : 0;
    else if (!strcmp(name, "persistent_suspended"))
        *value = ws->suspend_until == kSuspendForever ? 2 : (ws->sequence < ws->suspend_until ? 1 : 0);
    else if (!strcmp(name, "rho_last_mapping"))
        *value = ws->rho_last_mapping;
    else if (!strcmp(name, "rho_last_blocks"))
        *value = ws->rho_last_blocks;
#ifdef CAVMD_TEST_HOOKS
    else if (!strcmp(name, "debug_skip_publish"))
        *value = ws->debug_skip_publish;
    else if (!strcmp(name, "test_hooks"))
        *value = 1;
#else
    else if (!strcmp(name, "test_hooks"))
        *value = 0;
#endif
    else
        return CAVMD_ERR_INVALID_VALUE;
    return CAVMD_OK;
}

int cavmd_device_info(cavmd_workspace* ws, int* device, int* compute_units, char* arch_name, size_t arch_name_len)
{
    if (!ws)
        return CAVMD_ERR_INVALID_VALUE;
    if (device)
        *device = ws->device;
    if (compute_units)
        *compute_units = ws->num_cu;
    if (arch_name && arch_name_len)
    {
        strncpy(arch_name, ws->arch, arch_name_len - 1);
        arch_name[arch_name_len - 1] = 0;
    }
    return CAVMD_OK;
}

const char* cavmd_error_string(int status)
{
    switch (status)
    {
    case CAVMD_OK:
        return "success";
    case CAVMD_ERR_INVALID_VALUE:
        return "invalid value (null or misaligned pointer, bad stride or size)";
    case CAVMD_ERR_NO_DEVICE:
        return "no HIP device available (this library has no CPU fallback)";
    case CAVMD_ERR_CAPACITY:
        return "N exceeds the workspace capacity";
    case CAVMD_ERR_BAD_PARAMS:
        return "bad cavity parameters (K == 0 or non-finite)";
    case CAVMD_ERR_NOT_COMPUTED:
        return "no evaluation has been enqueued on this workspace yet";
    case CAVMD_ERR_EXPIRED:
        return "that evaluation's result slot has been reused: read it sooner or raise the \"result_history\" tunable";
    case CAVMD_ERR_SYNC_TIMEOUT:
        return "a single-launch evaluation was starved (its workgroups were not resident together) and could not be completed; "
               "forces of that evaluation are NaN";
    default:
        break;
    }
    if (status > 0)
        return hipGetErrorString((hipError_t)status);
    return "unknown cavmd status";
}

int cavmd_version(void)
{
    return CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR;
}

// ---- a batch of independent small systems in one launch (cavmd_batch_kernel.hpp) ------------------------------------------
// The replica loop of the reference (examples/05_advanced_run.py:1570-1612) on one GPU: B systems, one kernel, one
// workgroup per system.  The table of rows lives on the device from create / set_items on; compute enqueues the kernel and
// nothing else.
} // extern "C"

#include "cavmd_item_table.hpp" // how the tables of the seven objects below live on the host and on the device

namespace
{
constexpr int kBatchBlock = kSmallBlock; // the block size of cavity_small_system_kernel: the two paths share bits
constexpr size_t kBatchRingMaxBytes = (size_t)64 << 20;
static_assert(sizeof(cavmd_batch_item) == 128, "batch item layout");

BatchRow batch_row(const cavmd_batch_item& it)
{
    BatchRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.charge = it.d_charge;
    r.image = reinterpret_cast<const int*>(it.d_image);
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx; r.Ly = it.Ly; r.Lz = it.Lz;
    if (it.N)
        r.prm = derive(&it.params);
    r.N = it.N;
    r.L_typeid = it.L_typeid;
    return r;
}
} // namespace

struct cavmd_batch : ItemTable<cavmd_batch_item, BatchRow> // launched by N descending
{
    unsigned depth = 0;
    DeviceArray<cavmd_result> d_result;  // n blocks, indexed by item
    MappedBlock<HostResult> h_ring;      // depth x n blocks; evaluation s, item i -> (s % depth) * n + i
    uint64_t sequence = 0;
    bool captured = false; // some evaluation was enqueued into a stream capture: the stamps cannot tell replays apart

    cavmd_batch() : ItemTable(cavmd_batch_item_check, [](const cavmd_batch_item& it) { return it.N; }, batch_row) {}

    static constexpr bool tied = false; // the one object cavmd_destroy does not wait for (include/cavmd.h)
    int capacity_status(size_t n_items) const
    {
        return (size_t)depth * n_items * sizeof(HostResult) > kBatchRingMaxBytes ? CAVMD_ERR_CAPACITY : CAVMD_OK;
    }
    hipError_t alloc_own()
    {
        const hipError_t e = d_result.alloc_zeroed(n);
        return e == hipSuccess ? h_ring.alloc((size_t)depth * n) : e;
    }
};

namespace
{
inline const HostResult* batch_slot(const cavmd_batch* b, uint64_t s)
{
    return b->h_ring.host + (s % b->depth) * b->n;
}
} // namespace

extern "C"
{

int cavmd_batch_item_check(const cavmd_batch_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 4; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    // the checks of cavmd_compute_hoomd, in its order; an empty system may leave its arrays out
    if (it->N != 0 && (!it->d_pos || !it->d_charge || !it->d_image || !it->d_force))
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_force & 15) || ((uintptr_t)it->d_charge & 7)
        || ((uintptr_t)it->d_image & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N == 0)
        return CAVMD_OK;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    if (!params_ok(&it->params))
        return CAVMD_ERR_BAD_PARAMS;
    return CAVMD_OK;
}

int cavmd_batch_create(cavmd_workspace* ws, size_t n_items, const cavmd_batch_item* h_items, int history_depth,
                       cavmd_batch** out)
{
    const bool args_ok = history_depth >= 2 && history_depth <= (int)kResultHistoryMax;
    return create_table(ws, n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE,
                        [&](cavmd_batch* b) { b->depth = (unsigned)history_depth; });
}

int cavmd_batch_destroy(cavmd_batch* b)
{
    return destroy_table(b);
}

int cavmd_batch_set_items(cavmd_batch* b, size_t first, size_t count, const cavmd_batch_item* h_items)
{
    return b ? b->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_batch_compute(cavmd_batch* b, void* stream_)
{
    if (!b)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    if (!b->captured && stream_capturing(stream))
        b->captured = true;
    b->sequence += 1;
    HostResult* host = b->h_ring.dev + (b->sequence % b->depth) * b->n;
    const int st = b->launch(stream, cavity_batch_kernel<kBatchBlock>, dim3((unsigned)b->n), dim3(kBatchBlock), 0, b->d_rows.ptr,
                             b->d_order.ptr, b->sequence, b->d_result.ptr, host);
    if (st != CAVMD_OK)
        b->sequence -= 1;
    return st;
}

int cavmd_batch_last_sequence(cavmd_batch* b, uint64_t* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = b->sequence;
    return CAVMD_OK;
}

namespace
{
// Waits for the n stamps of evaluation `sequence` (never for the stream) and leaves b's blocks of it readable.  Each wait ends
// with the stamp, or once the same item's block of a LATER evaluation carries its stamp (the stream runs them in order), or
// with the stream idle; an evaluation that is over without its stamp died on the device.
int batch_wait(cavmd_batch* b, uint64_t sequence)
{
    const HostResult* slot = batch_slot(b, sequence);
    const uint64_t last = b->sequence;
    for (size_t i = 0; i < b->n; ++i)
    {
        const StampWait w = wait_for_stamp(&slot[i].ready, sequence, b->last_stream, [&] {
            for (uint64_t j = sequence + 1; j <= last; ++j)
                if (__atomic_load_n(&batch_slot(b, j)[i].ready, __ATOMIC_ACQUIRE) == j)
                    return true;
            return false;
        });
        if (w.error != hipSuccess)
            return (int)w.error;
        if (!w.arrived)
            return (int)hipErrorLaunchFailure;
    }
    return CAVMD_OK;
}

int batch_range_check(cavmd_batch* b, uint64_t sequence)
{
    if (b->sequence == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    if (b->captured) // replays publish under their frozen sequence: no history to read
        return CAVMD_ERR_INVALID_VALUE;
    if (sequence == 0 || sequence > b->sequence)
        return CAVMD_ERR_INVALID_VALUE;
    if (b->sequence - sequence >= b->depth)
        return CAVMD_ERR_EXPIRED;
    return CAVMD_OK;
}
} // namespace

int cavmd_batch_results_at(cavmd_batch* b, uint64_t sequence, cavmd_result* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    int st = batch_range_check(b, sequence);
    if (st != CAVMD_OK)
        return st;
    DeviceGuard guard(b->device);
    st = batch_wait(b, sequence);
    if (st != CAVMD_OK)
        return st;
    const HostResult* slot = batch_slot(b, sequence);
    for (size_t i = 0; i < b->n; ++i)
        memcpy(out + i, &slot[i].result, sizeof(cavmd_result));
    return CAVMD_OK;
}

int cavmd_batch_energies_at(cavmd_batch* b, uint64_t sequence, double* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    int st = batch_range_check(b, sequence);
    if (st != CAVMD_OK)
        return st;
    DeviceGuard guard(b->device);
    st = batch_wait(b, sequence);
    if (st != CAVMD_OK)
        return st;
    const HostResult* slot = batch_slot(b, sequence);
    for (size_t i = 0; i < b->n; ++i)
        memcpy(out + 3 * i, slot[i].result.energy, 3 * sizeof(double));
    return CAVMD_OK;
}

int cavmd_batch_results_read(cavmd_batch* b, cavmd_result* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    if (b->sequence == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    if (!b->captured)
        return cavmd_batch_results_at(b, b->sequence, out);
    // graph replays: the stamps cannot be trusted (frozen sequence) and the replay stream is unknown -> wait for the device
    // and copy the device blocks, which every replay rewrites
    DeviceGuard guard(b->device);
    CAVMD_HIP_TRY(hipDeviceSynchronize());
    CAVMD_HIP_TRY(hipMemcpy(out, b->d_result.ptr, sizeof(cavmd_result) * b->n, hipMemcpyDeviceToHost));
    return CAVMD_OK;
}

int cavmd_batch_results_device_ptr(cavmd_batch* b, const cavmd_result** out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = b->d_result.ptr;
    return CAVMD_OK;
}

} // extern "C"

// ---- the Bussi thermostat step of a batch of independent small systems in one launch (cavmd_bussi_batch_kernel.hpp) ---------
struct cavmd_bussi_batch : ItemTable<cavmd_bussi_batch_item, BussiBatchRow> // launched by n_members descending
{
    std::vector<uint64_t> refused_seen;        // per item: refusals already reported to the caller
    DeviceArray<BussiDevice> d_state;          // n states, indexed by item
    MappedBlock<HostBussiBatch> h_blocks;      // n blocks, indexed by item
    uint64_t sequence = 0;
    bool captured = false; // some step was enqueued into a stream capture: the stamps cannot tell replays apart

    cavmd_bussi_batch()
        : ItemTable(cavmd_bussi_batch_item_check, [](const cavmd_bussi_batch_item& it) { return it.n_members; },
                    uploaded_as_it_is<cavmd_bussi_batch_item, BussiBatchRow>)
    {
    }

    hipError_t alloc_own()
    {
        refused_seen.assign(n, 0);
        const hipError_t e = d_state.alloc_zeroed(n);
        return e == hipSuccess ? h_blocks.alloc(n) : e;
    }
};

namespace
{
static_assert(sizeof(cavmd_bussi_batch_item) == sizeof(BussiBatchRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_bussi_batch_item, n_members) == offsetof(BussiBatchRow, n)
                  && offsetof(cavmd_bussi_batch_item, dof_translational) == offsetof(BussiBatchRow, dof),
              "thermostat batch item layout");
static_assert(sizeof(cavmd_bussi_batch_input) == sizeof(BussiBatchInput) && offsetof(cavmd_bussi_batch_input, skip) == 32,
              "thermostat batch input layout");
static_assert(sizeof(cavmd_bussi_device_state) == sizeof(BussiDevice), "the device states are read out as they are");
static_assert(CAVMD_BATCH_MAX_ITEM_N <= kBussiBatchMaxTiles * 256 * kBussiBatchUnroll, "one LDS partial per tile");

void bussi_state_out(cavmd_bussi_device_state* out, const BussiDevice& s)
{
    out->reservoir_translational = s.reservoir;
    out->instantaneous_translational = s.instantaneous;
    out->last_alpha = s.alpha;
    out->last_kinetic_energy = s.kinetic;
    out->steps = s.steps;
    out->refused = s.errors;
}
} // namespace

extern "C"
{

int cavmd_bussi_batch_item_check(const cavmd_bussi_batch_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 4; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if (it->n_members != 0 && !it->d_vel)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (!std::isfinite(it->dof_translational) || it->dof_translational < 0.0)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->n_members > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_bussi_batch_input_make(double deltaT, double set_T, double tau, double normal_variate, double gamma_variate,
                                 cavmd_bussi_batch_input* row)
{
    if (!row)
        return CAVMD_ERR_INVALID_VALUE;
    memset(row, 0, sizeof(*row));
    row->normal_variate = normal_variate;
    row->gamma_variate = gamma_variate;
    row->c = (tau != 0.0) ? exp(-deltaT / tau) : 0.0; // the expression of cavmd_bussi_step_device (:186-190)
    row->set_T = set_T;
    row->skip = (deltaT == 0.0) ? 1u : 0u;             // src/BussiReservoirThermostat.h:45-48
    return CAVMD_OK;
}

int cavmd_bussi_batch_create(cavmd_workspace* ws, size_t n_items, const cavmd_bussi_batch_item* h_items,
                             cavmd_bussi_batch** out)
{
    return create_table(ws, n_items, h_items, out, CAVMD_OK, [](cavmd_bussi_batch*) {});
}

int cavmd_bussi_batch_destroy(cavmd_bussi_batch* b)
{
    return destroy_table(b);
}

int cavmd_bussi_batch_set_items(cavmd_bussi_batch* b, size_t first, size_t count, const cavmd_bussi_batch_item* h_items)
{
    return b ? b->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_bussi_batch_step(cavmd_bussi_batch* b, void* stream_, const cavmd_bussi_batch_input* d_inputs)
{
    if (!b || !d_inputs || ((uintptr_t)d_inputs & 7))
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    if (!b->captured && stream_capturing(stream))
        b->captured = true;
    b->sequence += 1;
    const int st = b->launch(stream, bussi_batch_kernel<256>, dim3((unsigned)b->n), dim3(256), 0, b->d_rows.ptr, b->d_order.ptr,
                             reinterpret_cast<const BussiBatchInput*>(d_inputs), b->sequence, b->d_state.ptr, b->h_blocks.dev);
    if (st != CAVMD_OK)
        b->sequence -= 1;
    return st;
}

int cavmd_bussi_batch_last_sequence(cavmd_bussi_batch* b, uint64_t* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = b->sequence;
    return CAVMD_OK;
}

int cavmd_bussi_batch_read(cavmd_bussi_batch* b, cavmd_bussi_device_state* out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    memset(out, 0, sizeof(*out) * b->n);
    if (b->sequence == 0)
        return CAVMD_OK;
    DeviceGuard guard(b->device);
    if (b->captured)
    {
        // graph replays: frozen sequence, unknown replay stream -> wait for the device and copy the device states
        CAVMD_HIP_TRY(hipDeviceSynchronize());
        CAVMD_HIP_TRY(hipMemcpy(out, b->d_state.ptr, sizeof(BussiDevice) * b->n, hipMemcpyDeviceToHost));
    }
    else
    {
        const uint64_t want = b->sequence;
        for (size_t i = 0; i < b->n; ++i)
        {
            const HostBussiBatch* h = b->h_blocks.host + i;
            const StampWait w = wait_for_stamp(&h->ready, want, b->last_stream);
            if (w.error != hipSuccess)
                return (int)w.error;
            if (!w.arrived)
                return (int)hipErrorLaunchFailure; // a launch that never published
            bussi_state_out(out + i, h->state);
        }
    }
    bool refused = false;
    for (size_t i = 0; i < b->n; ++i)
        if (out[i].refused != b->refused_seen[i])
        {
            b->refused_seen[i] = out[i].refused;
            refused = true;
        }
    return refused ? CAVMD_ERR_BAD_PARAMS : CAVMD_OK; // "Bussi thermostat requires non-zero initial momenta."
}

int cavmd_bussi_batch_reset(cavmd_bussi_batch* b, void* stream_)
{
    if (!b)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(b->device);
    // wait for the last step's stamps first so that the host copies can be reset consistently (not while it is being captured)
    if (b->sequence && !b->captured)
    {
        std::vector<cavmd_bussi_device_state> unused(b->n);
        const int st = cavmd_bussi_batch_read(b, unused.data());
        if (st != CAVMD_OK && st != CAVMD_ERR_BAD_PARAMS)
            return st;
    }
    CAVMD_HIP_TRY(hipMemsetAsync(b->d_state.ptr, 0, sizeof(BussiDevice) * b->n, stream));
    for (size_t i = 0; i < b->n; ++i)
        memset(&b->h_blocks.host[i].state, 0, sizeof(BussiDevice));
    std::fill(b->refused_seen.begin(), b->refused_seen.end(), (uint64_t)0);
    return CAVMD_OK;
}

int cavmd_bussi_batch_state_device_ptr(cavmd_bussi_batch* b, const cavmd_bussi_device_state** out)
{
    if (!b || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = reinterpret_cast<const cavmd_bussi_device_state*>(b->d_state.ptr);
    return CAVMD_OK;
}

} // extern "C"

// ---- per-step observables of a batch recorded into a time series in device memory (cavmd_recorder_kernel.hpp) ----------------
// launched by max(N, n_members) descending; kRecCounters words per item: rows, calls, phase, slot
namespace
{
constexpr size_t kRecorderMaxBytes = (size_t)1 << 30; // of one recorder's series (and, for a field recorder, its fields)
}

struct cavmd_recorder : SeriesTable<cavmd_recorder_item, RecorderRow, cavmd_record>
{
    uint64_t period = 1;
    double kB = 0.0;

    cavmd_recorder()
        : SeriesTable(kRecCounters, cavmd_recorder_item_check,
                      [](const cavmd_recorder_item& it) { return std::max(it.N, it.n_members); },
                      uploaded_as_it_is<cavmd_recorder_item, RecorderRow>)
    {
    }

    int capacity_status(size_t n_items) const
    {
        return capacity > kRecorderMaxBytes / sizeof(cavmd_record) / n_items ? CAVMD_ERR_CAPACITY : CAVMD_OK;
    }
    hipError_t alloc_own()
    {
        return alloc_series();
    }
};

namespace
{
static_assert(sizeof(cavmd_record) == 128 && offsetof(cavmd_record, energy) == 16 && offsetof(cavmd_record, cavity_kinetic) == 88,
              "record layout");
static_assert(sizeof(cavmd_recorder_item) == sizeof(RecorderRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_recorder_item, d_result) == offsetof(RecorderRow, res)
                  && offsetof(cavmd_recorder_item, d_vel) == offsetof(RecorderRow, vel2)
                  && offsetof(cavmd_recorder_item, d_net_force) == offsetof(RecorderRow, force2)
                  && offsetof(cavmd_recorder_item, d_members) == offsetof(RecorderRow, members)
                  && offsetof(cavmd_recorder_item, N) == offsetof(RecorderRow, N)
                  && offsetof(cavmd_recorder_item, n_members) == offsetof(RecorderRow, n_members),
              "recorder item layout");
static_assert(CAVMD_BATCH_MAX_ITEM_N <= kRecorderMaxTiles * 256 * kRecorderUnroll, "one LDS partial per tile");
static_assert(kRecRows == 0 && kFldRows == 0, "SeriesTable: the rows-written array is the first of the counters");
} // namespace

extern "C"
{

int cavmd_recorder_item_check(const cavmd_recorder_item* it)
{
    if (!it || !it->d_result)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 3; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_result & 15) || ((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_net_force & 15)
        || ((uintptr_t)it->d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N || it->n_members > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_recorder_item* h_items, size_t capacity,
                          uint64_t period, double kB, cavmd_recorder** out)
{
    const bool args_ok = capacity != 0 && period != 0 && kB > 0.0 && std::isfinite(kB);
    return create_table(ws, n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE, [&](cavmd_recorder* r) {
        r->capacity = capacity;
        r->period = period;
        r->kB = kB;
    });
}

int cavmd_recorder_destroy(cavmd_recorder* r)
{
    return destroy_table(r);
}

int cavmd_recorder_set_items(cavmd_recorder* r, size_t first, size_t count, const cavmd_recorder_item* h_items)
{
    return r ? r->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_record(cavmd_recorder* r, void* stream_)
{
    if (!r)
        return CAVMD_ERR_INVALID_VALUE;
    return r->launch((hipStream_t)stream_, recorder_batch_kernel<256>, dim3((unsigned)r->n), dim3(256), 0, r->d_rows.ptr,
                     r->d_order.ptr, (unsigned)r->n, (uint64_t)r->capacity, r->period, r->kB, r->d_series.ptr, r->d_counters.ptr);
}

int cavmd_recorder_rows(cavmd_recorder* r, void* stream_, uint64_t* out)
{
    return (r && out) ? r->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_read(cavmd_recorder* r, void* stream_, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows,
                        cavmd_record* out)
{
    if (!r || !out || n_items == 0 || n_rows == 0 || first_item >= r->n || n_items > r->n - first_item)
        return CAVMD_ERR_INVALID_VALUE;
    return r->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, out);
}

int cavmd_recorder_reset(cavmd_recorder* r, void* stream_)
{
    return r ? r->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_device_ptr(cavmd_recorder* r, const cavmd_record** records, const uint64_t** rows)
{
    return r ? r->device_ptr(records, rows) : CAVMD_ERR_INVALID_VALUE;
}

} // extern "C"

// ---- density field and F(k,t) of a batch recorded into a time series in device memory (cavmd_field_recorder_kernel.hpp) -------
// launched by N descending; kFldCounters words per item
struct cavmd_field_recorder : SeriesTable<cavmd_field_item, FieldRow, cavmd_field_record>
{
    size_t n_k = 0;
    uint64_t period = 1;
    unsigned max_refs = 1;
    uint64_t interval = 0;
    const double* h_kvec = nullptr;   // the caller's wavevectors: read by create only
    DeviceArray<double> d_kvec;       // n_k x 3
    DeviceArray<uint64_t> d_ref_rows; // n x max_refs: the row each reference was taken at
    DeviceArray<double> d_now;        // n x n_k x 2: the field of the last recorded call
    DeviceArray<double> d_refs;       // n x max_refs x n_k x 2

    cavmd_field_recorder()
        : SeriesTable(kFldCounters, cavmd_field_recorder_item_check, [](const cavmd_field_item& it) { return it.N; },
                      uploaded_as_it_is<cavmd_field_item, FieldRow>)
    {
    }

    // series + fields (the current one and the references) within the recorder's cap
    int capacity_status(size_t n_items) const
    {
        const size_t fields = sizeof(double) * 2 * n_k * ((size_t)max_refs + 1) * n_items;
        return fields > kRecorderMaxBytes || capacity > (kRecorderMaxBytes - fields) / sizeof(cavmd_field_record) / n_items
                   ? CAVMD_ERR_CAPACITY
                   : CAVMD_OK;
    }
    hipError_t alloc_own()
    {
        hipError_t e = d_kvec.upload(h_kvec, 3 * n_k);
        h_kvec = nullptr;
        if (e == hipSuccess)
            e = alloc_series();
        if (e == hipSuccess)
            e = d_ref_rows.alloc_zeroed(n * max_refs);
        if (e == hipSuccess)
            e = d_now.alloc_zeroed(2 * n_k * n);
        return e == hipSuccess ? d_refs.alloc_zeroed(2 * n_k * n * max_refs) : e;
    }
};

namespace
{
static_assert(sizeof(cavmd_field_record) == 160 && offsetof(cavmd_field_record, n_references) == 8
                  && offsetof(cavmd_field_record, took_reference) == 12 && offsetof(cavmd_field_record, rho2) == 16
                  && offsetof(cavmd_field_record, F) == 32,
              "field record layout");
static_assert(sizeof(cavmd_field_item) == sizeof(FieldRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_field_item, d_position) == offsetof(FieldRow, pos)
                  && offsetof(cavmd_field_item, position_stride) == offsetof(FieldRow, stride)
                  && offsetof(cavmd_field_item, N) == offsetof(FieldRow, N),
              "field item layout");
} // namespace

extern "C"
{

int cavmd_field_recorder_item_check(const cavmd_field_item* it)
{
    if (!it || it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 5; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if ((!it->d_position && it->N > 0) || ((uintptr_t)it->d_position & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->position_stride < 24 || (it->position_stride & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_field_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_field_item* h_items, size_t n_k,
                                const double* h_wavevectors, size_t capacity, uint64_t period, uint32_t max_references,
                                uint64_t reference_interval, cavmd_field_recorder** out)
{
    bool args_ok = h_wavevectors && n_k != 0 && n_k <= CAVMD_FIELD_MAX_WAVEVECTORS && capacity != 0 && period != 0
        && max_references != 0 && max_references <= CAVMD_FIELD_MAX_REFERENCES;
    for (size_t i = 0; args_ok && i < 3 * n_k; ++i)
        args_ok = std::isfinite(h_wavevectors[i]);
    return create_table(ws, n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE, [&](cavmd_field_recorder* r) {
        r->n_k = n_k;
        r->h_kvec = h_wavevectors;
        r->capacity = capacity;
        r->period = period;
        r->max_refs = max_references;
        r->interval = reference_interval;
    });
}

int cavmd_field_recorder_destroy(cavmd_field_recorder* r)
{
    return destroy_table(r);
}

int cavmd_field_recorder_set_items(cavmd_field_recorder* r, size_t first, size_t count, const cavmd_field_item* h_items)
{
    return r ? r->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_record(cavmd_field_recorder* r, void* stream_, const uint32_t* d_take_reference)
{
    if (!r || ((uintptr_t)d_take_reference & 3))
        return CAVMD_ERR_INVALID_VALUE;
    return r->launch((hipStream_t)stream_, field_recorder_batch_kernel<256>, dim3((unsigned)r->n), dim3(256), 0, r->d_rows.ptr,
                     r->d_order.ptr, (unsigned)r->n, r->d_kvec.ptr, (unsigned)r->n_k, make_sincos_coef(), (uint64_t)r->capacity,
                     r->period, r->max_refs, r->interval, d_take_reference, r->d_series.ptr, r->d_counters.ptr, r->d_ref_rows.ptr,
                     r->d_now.ptr, r->d_refs.ptr);
}

int cavmd_field_recorder_rows(cavmd_field_recorder* r, void* stream_, uint64_t* out)
{
    return (r && out) ? r->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_read(cavmd_field_recorder* r, void* stream_, size_t first_item, size_t n_items, uint64_t first_row,
                              size_t n_rows, cavmd_field_record* out)
{
    if (!r || !out || n_items == 0 || n_rows == 0 || first_item >= r->n || n_items > r->n - first_item)
        return CAVMD_ERR_INVALID_VALUE;
    return r->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, out);
}

int cavmd_field_recorder_read_fields(cavmd_field_recorder* r, void* stream_, size_t item, double* rho_now, double* rho_refs,
                                     uint64_t* ref_rows, uint32_t* n_refs)
{
    if (!r || !n_refs || item >= r->n)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(r->device);
    const int st = sync_uncaptured((hipStream_t)stream_);
    if (st != CAVMD_OK)
        return st;
    uint64_t rows = 0, refs = 0;
    CAVMD_HIP_TRY(hipMemcpy(&rows, r->d_counters.ptr + (size_t)kFldRows * r->n + item, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rows == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    CAVMD_HIP_TRY(hipMemcpy(&refs, r->d_counters.ptr + (size_t)kFldRefs * r->n + item, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (refs > r->max_refs)
        return CAVMD_ERR_INVALID_VALUE;
    const size_t field_len = 2 * r->n_k;
    if (rho_now)
        CAVMD_HIP_TRY(hipMemcpy(rho_now, r->d_now.ptr + item * field_len, sizeof(double) * field_len, hipMemcpyDeviceToHost));
    if (rho_refs && refs)
        CAVMD_HIP_TRY(hipMemcpy(rho_refs, r->d_refs.ptr + item * r->max_refs * field_len, sizeof(double) * field_len * refs,
                                hipMemcpyDeviceToHost));
    if (ref_rows && refs)
        CAVMD_HIP_TRY(hipMemcpy(ref_rows, r->d_ref_rows.ptr + item * r->max_refs, sizeof(uint64_t) * refs, hipMemcpyDeviceToHost));
    *n_refs = (uint32_t)refs;
    return CAVMD_OK;
}

int cavmd_field_recorder_reset(cavmd_field_recorder* r, void* stream_)
{
    return r ? r->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_device_ptr(cavmd_field_recorder* r, const cavmd_field_record** records, const uint64_t** rows)
{
    return r ? r->device_ptr(records, rows) : CAVMD_ERR_INVALID_VALUE;
}

} // extern "C"

// ---- the velocity-Verlet step of a batch of independent small systems, one launch per half-step (cavmd_verlet_batch_kernel.hpp) --
struct cavmd_verlet : ItemTable<cavmd_verlet_item, VerletRow> // launched by N descending
{
    DeviceArray<VerletState> d_state; // n states, indexed by item

    cavmd_verlet()
        : ItemTable(cavmd_verlet_item_check, [](const cavmd_verlet_item& it) { return it.N; },
                    uploaded_as_it_is<cavmd_verlet_item, VerletRow>)
    {
    }

    hipError_t alloc_own()
    {
        return d_state.alloc_zeroed(n);
    }

    // one launch of n workgroups of one of the three kernels
    template <class Kernel>
    int launch_step(void* stream, Kernel kernel, const cavmd_verlet_input* d_inputs)
    {
        return launch((hipStream_t)stream, kernel, dim3((unsigned)n), dim3(256), 0, d_rows.ptr, d_order.ptr,
                      reinterpret_cast<const VerletInput*>(d_inputs), d_state.ptr);
    }
};

namespace
{
static_assert(sizeof(cavmd_verlet_item) == sizeof(VerletRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_verlet_item, d_pos) == offsetof(VerletRow, pos2)
                  && offsetof(cavmd_verlet_item, d_image) == offsetof(VerletRow, image)
                  && offsetof(cavmd_verlet_item, d_vel) == offsetof(VerletRow, vel2)
                  && offsetof(cavmd_verlet_item, d_accel) == offsetof(VerletRow, accel)
                  && offsetof(cavmd_verlet_item, d_force) == offsetof(VerletRow, force2)
                  && offsetof(cavmd_verlet_item, d_net_force) == offsetof(VerletRow, net2)
                  && offsetof(cavmd_verlet_item, Lx) == offsetof(VerletRow, Lx)
                  && offsetof(cavmd_verlet_item, N) == offsetof(VerletRow, n)
                  && offsetof(cavmd_verlet_item, langevin_index) == offsetof(VerletRow, langevin),
              "integrator item layout");
static_assert(sizeof(cavmd_verlet_input) == sizeof(VerletInput) && offsetof(cavmd_verlet_input, dt) == offsetof(VerletInput, dt)
                  && offsetof(cavmd_verlet_input, langevin_gamma) == offsetof(VerletInput, gamma)
                  && offsetof(cavmd_verlet_input, langevin_coeff) == offsetof(VerletInput, coeff)
                  && offsetof(cavmd_verlet_input, uniform) == offsetof(VerletInput, uniform)
                  && offsetof(cavmd_verlet_input, skip) == offsetof(VerletInput, skip),
              "integrator input layout");
static_assert(sizeof(cavmd_verlet_state) == sizeof(VerletState) && offsetof(cavmd_verlet_state, steps) == offsetof(VerletState, steps)
                  && offsetof(cavmd_verlet_state, out_of_box) == offsetof(VerletState, out_of_box)
                  && offsetof(cavmd_verlet_state, langevin_reservoir) == offsetof(VerletState, reservoir),
              "the integrator states are read out as they are");
static_assert(sizeof(((cavmd_verlet_item*)nullptr)->d_force) / sizeof(void*) == kVerletMaxForces, "force arrays per item");
} // namespace

extern "C"
{

int cavmd_verlet_item_check(const cavmd_verlet_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 3; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_image & 3) || ((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_accel & 7)
        || ((uintptr_t)it->d_net_force & 15))
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < kVerletMaxForces; ++k)
    {
        if ((uintptr_t)it->d_force[k] & 15)
            return CAVMD_ERR_INVALID_VALUE;
        if (k > 0 && it->d_force[k] && !it->d_force[k - 1]) // the list ends at the first NULL
            return CAVMD_ERR_INVALID_VALUE;
    }
    if (it->N != 0 && (!it->d_pos || !it->d_image || !it->d_vel || !it->d_accel || !it->d_force[0]))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->langevin_index < -1 || (it->langevin_index >= 0 && (uint32_t)it->langevin_index >= it->N))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_verlet_input_make(double dt, double gamma, double kT, const double uniform[3], cavmd_verlet_input* row)
{
    if (!row || !uniform)
        return CAVMD_ERR_INVALID_VALUE;
    memset(row, 0, sizeof(*row));
    row->dt = dt;
    row->langevin_gamma = gamma;
    // TwoStepLangevin: coeff = sqrt(6 gamma T / deltaT) [HOOMD upstream, not in checkout]
    row->langevin_coeff = (gamma != 0.0 && dt != 0.0) ? sqrt(6.0 * gamma * kT / dt) : 0.0;
    for (int c = 0; c < 3; ++c)
        row->uniform[c] = uniform[c];
    row->skip = (dt == 0.0) ? 1u : 0u;
    return CAVMD_OK;
}

int cavmd_verlet_create(cavmd_workspace* ws, size_t n_items, const cavmd_verlet_item* h_items, cavmd_verlet** out)
{
    return create_table(ws, n_items, h_items, out, CAVMD_OK, [](cavmd_verlet*) {});
}

int cavmd_verlet_destroy(cavmd_verlet* v)
{
    return destroy_table(v);
}

int cavmd_verlet_set_items(cavmd_verlet* v, size_t first, size_t count, const cavmd_verlet_item* h_items)
{
    return v ? v->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_verlet_accelerations(cavmd_verlet* v, void* stream_)
{
    if (!v)
        return CAVMD_ERR_INVALID_VALUE;
    return v->launch_step(stream_, verlet_step_two_kernel<256, true>, nullptr);
}

int cavmd_verlet_step_one(cavmd_verlet* v, void* stream_, const cavmd_verlet_input* d_inputs)
{
    if (!v || !d_inputs || ((uintptr_t)d_inputs & 7))
        return CAVMD_ERR_INVALID_VALUE;
    return v->launch_step(stream_, verlet_step_one_kernel<256>, d_inputs);
}

int cavmd_verlet_step_two(cavmd_verlet* v, void* stream_, const cavmd_verlet_input* d_inputs)
{
    if (!v || !d_inputs || ((uintptr_t)d_inputs & 7))
        return CAVMD_ERR_INVALID_VALUE;
    return v->launch_step(stream_, verlet_step_two_kernel<256, false>, d_inputs);
}

int cavmd_verlet_read(cavmd_verlet* v, void* stream_, cavmd_verlet_state* out)
{
    if (!v || !out)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(v->device);
    const int st = sync_uncaptured((hipStream_t)stream_);
    if (st != CAVMD_OK)
        return st;
    CAVMD_HIP_TRY(hipMemcpy(out, v->d_state.ptr, sizeof(VerletState) * v->n, hipMemcpyDeviceToHost));
    return CAVMD_OK;
}

int cavmd_verlet_reset(cavmd_verlet* v, void* stream_)
{
    if (!v)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(v->device);
    CAVMD_HIP_TRY(hipMemsetAsync(v->d_state.ptr, 0, sizeof(VerletState) * v->n, (hipStream_t)stream_));
    return CAVMD_OK;
}

int cavmd_verlet_state_device_ptr(cavmd_verlet* v, const cavmd_verlet_state** out)
{
    if (!v || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = reinterpret_cast<const cavmd_verlet_state*>(v->d_state.ptr);
    return CAVMD_OK;
}

} // extern "C"

// ---- harmonic bonds and Lennard-Jones pairs of a batch of independent small systems in ONE launch (cavmd_molecular_batch_kernel.hpp) --
// A LinkedTable (cavmd_item_table.hpp): what is below is the status of an item and how the device tables follow from the items.
namespace
{
constexpr int kMolecularJSplit = CAVMD_MOLECULAR_J_SPLIT;
constexpr unsigned kMolecularRows = kMolecularBlock / kMolecularJSplit;
static_assert(kMolecularJSplit == 1 || kMolecularJSplit == 4 || kMolecularJSplit == 16, "S is one of the measured candidates");
static_assert(sizeof(cavmd_molecular_pair) == sizeof(MolecularPair) && sizeof(cavmd_molecular_params) == sizeof(MolecularParams)
                  && offsetof(cavmd_molecular_pair, lj1) == 0 && offsetof(cavmd_molecular_pair, lj2) == 8
                  && offsetof(cavmd_molecular_pair, lj1_12) == 16 && offsetof(cavmd_molecular_pair, lj2_6) == 24
                  && offsetof(cavmd_molecular_pair, rcutsq) == 32 && offsetof(cavmd_molecular_pair, eshift) == 40
                  && offsetof(cavmd_molecular_params, n_types) == offsetof(MolecularParams, n_types)
                  && offsetof(cavmd_molecular_params, n_bond_types) == offsetof(MolecularParams, n_bond_types)
                  && offsetof(cavmd_molecular_params, pair) == offsetof(MolecularParams, pair)
                  && offsetof(cavmd_molecular_params, bond) == offsetof(MolecularParams, bond),
              "the molecular parameters are uploaded as they are");
static_assert(sizeof(cavmd_molecular_item) == 64 && sizeof(cavmd_molecular_bond) == 12, "molecular item layout");
static_assert(CAVMD_MOLECULAR_MAX_TYPES == kMolecularMaxTypes && CAVMD_MOLECULAR_MAX_BONDS == kMolecularMaxBonds
                  && CAVMD_MOLECULAR_MAX_BOND_TYPES == 8,
              "the header's limits are the kernel's");
static_assert(molecular_lds_bytes(CAVMD_MOLECULAR_MAX_ITEM_N) <= 64 * 1024, "the largest system fits the LDS a kernel gets without opt-in");
static_assert(CAVMD_MOLECULAR_MAX_ITEM_N <= 0xFFFF, "a partner index takes the low 16 bits of a slot");

bool finite_nonnegative(double x)
{
    return isfinite(x) && x >= 0.0;
}

// The status of one item; `prm` NULL: only what can be said without the parameters (bond types and the cut-offs are not
// looked at).  `slots`, if given, receives the item's partner table: four slots a particle, partner | bond type << 16.
int molecular_item_status(const cavmd_molecular_params* prm, const cavmd_molecular_item* it, std::vector<uint32_t>* slots)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_force & 15) || ((uintptr_t)it->h_bonds & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N != 0 && (!it->d_pos || !it->d_force))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->n_bonds != 0 && !it->h_bonds)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_MOLECULAR_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    if (it->N != 0)
    {
        double cut_sq = 0.0;
        if (!box_ok(it->Lx, it->Ly, it->Lz, &cut_sq))
            return CAVMD_ERR_INVALID_VALUE;
        if (prm)
            for (unsigned a = 0; a < prm->n_types; ++a)
                for (unsigned b = 0; b < prm->n_types; ++b)
                    if (prm->pair[a][b].rcutsq > cut_sq)
                        return CAVMD_ERR_INVALID_VALUE;
    }
    const uint32_t n_bond_types = prm ? prm->n_bond_types : CAVMD_MOLECULAR_MAX_BOND_TYPES;
    for (uint32_t k = 0; k < it->n_bonds; ++k)
        if (it->h_bonds[k].type >= n_bond_types)
            return CAVMD_ERR_INVALID_VALUE;
    return partner_slots(it->N, it->h_bonds, it->n_bonds, kMolecularMaxBonds, kMolecularNoPartner,
                         [](uint32_t partner, uint32_t type) { return partner | (type << 16); }, slots);
}

MolecularRow molecular_row(const cavmd_molecular_item& it)
{
    MolecularRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx;
    r.Ly = it.Ly;
    r.Lz = it.Lz;
    r.n = it.N;
    return r;
}

// what set_items replaces together
struct MolecularTables
{
    DeviceArray<uint4> blocks, partners;
    MolecularHeader header;
    unsigned lds_n = 2; // particles the next launch has LDS for
};
} // namespace

// workgroups by N descending; per item its partner table
struct cavmd_molecular final : LinkedTable<cavmd_molecular_item, MolecularRow, std::vector<uint32_t>, MolecularTables>
{
    cavmd_molecular_params params;
    DeviceArray<MolecularParams> d_params;

    cavmd_molecular() : LinkedTable([](const cavmd_molecular_item& it) { return it.N; }, molecular_row) {}

    int item_status(const cavmd_molecular_item* it, std::vector<uint32_t>* slots) const override
    {
        return molecular_item_status(&params, it, slots);
    }

    void strip(cavmd_molecular_item* it) const override
    {
        it->h_bonds = nullptr;
        it->n_bonds = 0;
    }

    hipError_t alloc_own()
    {
        const hipError_t e = LinkedTable::alloc_own();
        return e == hipSuccess ? d_params.upload(&params, 1) : e; // a blocking copy: there before any launch
    }

    hipError_t fill(const std::vector<cavmd_molecular_item>& all, const std::vector<unsigned>& launch,
                    const std::vector<std::vector<uint32_t>>& slots, MolecularTables* t) const override
    {
        std::vector<uint32_t> base(all.size()), pool;
        unsigned largest = 0;
        for (size_t i = 0; i < all.size(); ++i)
        {
            base[i] = pool_append(&pool, slots[i]) / kMolecularMaxBonds;
            largest = std::max(largest, all[i].N);
        }
        std::vector<uint4> table;
        for (unsigned item : launch)
            emit_blocks(&table, item, all[item].N, kMolecularRows, base[item], 0u);
        hipError_t e = t->blocks.upload(table.data(), table.size());
        if (e == hipSuccess)
            e = t->partners.upload(pool.data(), pool.size());
        memset(&t->header, 0, sizeof(t->header));
        t->header.blocks = t->blocks.ptr;
        t->header.partners = t->partners.ptr;
        t->header.n_blocks = (unsigned)table.size();
        t->lds_n = lds_particles(largest);
        return e;
    }
};

extern "C"
{

int cavmd_molecular_pair_make(double epsilon, double sigma, double r_cut, int shift, cavmd_molecular_pair* out)
{
    if (!out || !finite_nonnegative(epsilon) || !finite_nonnegative(sigma) || !finite_nonnegative(r_cut))
        return CAVMD_ERR_INVALID_VALUE;
    cavmd_molecular_pair p;
    memset(&p, 0, sizeof(p));
    const double s2 = sigma * sigma;
    const double s6 = (s2 * s2) * s2;
    p.lj2 = (4.0 * epsilon) * s6;
    p.lj1 = p.lj2 * s6;
    p.lj1_12 = 12.0 * p.lj1;
    p.lj2_6 = 6.0 * p.lj2;
    p.rcutsq = r_cut * r_cut;
    p.eshift = 0.0;
    if (shift && p.rcutsq > 0.0)
    {
        const double r2inv = 1.0 / p.rcutsq;
        const double r6inv = (r2inv * r2inv) * r2inv;
        p.eshift = r6inv * ((p.lj1 * r6inv) - p.lj2);
    }
    if (!isfinite(p.lj1_12) || !isfinite(p.lj2_6) || !isfinite(p.rcutsq) || !isfinite(p.eshift))
        return CAVMD_ERR_INVALID_VALUE;
    *out = p;
    return CAVMD_OK;
}

int cavmd_molecular_params_check(const cavmd_molecular_params* prm)
{
    if (!prm || prm->n_types > CAVMD_MOLECULAR_MAX_TYPES || prm->n_bond_types > CAVMD_MOLECULAR_MAX_BOND_TYPES || prm->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (unsigned a = 0; a < prm->n_types; ++a)
        for (unsigned b = 0; b < prm->n_types; ++b)
        {
            const cavmd_molecular_pair& p = prm->pair[a][b];
            if (!finite_nonnegative(p.lj1) || !finite_nonnegative(p.lj2) || !finite_nonnegative(p.lj1_12) || !finite_nonnegative(p.lj2_6)
                || !finite_nonnegative(p.rcutsq) || !isfinite(p.eshift) || p.reserved[0] != 0 || p.reserved[1] != 0)
                return CAVMD_ERR_INVALID_VALUE;
            if (memcmp(&p, &prm->pair[b][a], sizeof(p)) != 0)
                return CAVMD_ERR_INVALID_VALUE;
        }
    for (unsigned k = 0; k < prm->n_bond_types; ++k)
        if (!finite_nonnegative(prm->bond[k].K) || !finite_nonnegative(prm->bond[k].r0))
            return CAVMD_ERR_INVALID_VALUE;
    return CAVMD_OK;
}

int cavmd_molecular_item_check(const cavmd_molecular_params* prm, const cavmd_molecular_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    const int st = cavmd_molecular_params_check(prm);
    if (st != CAVMD_OK)
        return st;
    return molecular_item_status(prm, it, nullptr);
}

int cavmd_molecular_order(int* rows, int* j_split)
{
    if (rows)
        *rows = (int)kMolecularRows;
    if (j_split)
        *j_split = kMolecularJSplit;
    return CAVMD_OK;
}

int cavmd_molecular_create(cavmd_workspace* ws, const cavmd_molecular_params* prm, size_t n_items, const cavmd_molecular_item* h_items,
                           cavmd_molecular** out)
{
    return create_table(ws, n_items, h_items, out, cavmd_molecular_params_check(prm), [&](cavmd_molecular* m) { m->params = *prm; });
}

int cavmd_molecular_destroy(cavmd_molecular* m)
{
    return destroy_table(m);
}

int cavmd_molecular_set_items(cavmd_molecular* m, size_t first, size_t count, const cavmd_molecular_item* h_items)
{
    return m ? m->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_molecular_compute(cavmd_molecular* m, void* stream_)
{
    if (!m)
        return CAVMD_ERR_INVALID_VALUE;
    const MolecularTables& t = m->tables;
    return m->launch((hipStream_t)stream_, molecular_force_kernel<kMolecularBlock, kMolecularJSplit>,
                     dim3(std::max(t.header.n_blocks, 1u)), dim3(kMolecularBlock), molecular_lds_bytes(t.lds_n), m->d_rows.ptr,
                     m->d_header.ptr, m->d_params.ptr, t.lds_n);
}

} // extern "C"

// ---- Ewald Coulomb forces of a batch of independent small systems in TWO launches (cavmd_coulomb_batch_kernel.hpp) ------------
// A LinkedTable as well: the status of an item with its k-vectors, and how the device tables follow from the items.
namespace
{
constexpr int kCoulombJSplit = CAVMD_COULOMB_J_SPLIT;
constexpr int kCoulombKSplit = CAVMD_COULOMB_K_SPLIT;
constexpr unsigned kCoulombRows = kCoulombBlock / kCoulombJSplit;
constexpr unsigned kCoulombKRows = kCoulombBlock / kCoulombKSplit;
static_assert(kCoulombJSplit == 1 || kCoulombJSplit == 4 || kCoulombJSplit == 16 || kCoulombJSplit == 64, "S is one of the candidates");
static_assert(kCoulombKSplit == 1 || kCoulombKSplit == 4 || kCoulombKSplit == 16 || kCoulombKSplit == 64, "T is one of the candidates");
static_assert(sizeof(cavmd_coulomb_item) == 96, "coulomb item layout");
static_assert(CAVMD_COULOMB_MAX_EXCLUSIONS == kCoulombMaxExclusions, "the header's limit is the kernel's");
static_assert(coulomb_lds_bytes(CAVMD_COULOMB_MAX_ITEM_N) <= 64 * 1024, "the largest system fits the LDS a kernel gets without opt-in");
constexpr double kCoulombPi = 3.141592653589793;
constexpr double kCoulombSqrtPi = 1.7724538509055159;

// The kept k-vectors of an item (whose box and cut-offs have been checked), in the contract's order; stops at `limit` + 1.
// Every loop visits kept vectors and one more per row, so the work is bounded by the limit whatever k_cut is.
void coulomb_k_vectors(const cavmd_coulomb_item& it, size_t limit, std::vector<CoulombK>* out, size_t* count)
{
    const double two_pi = 2.0 * kCoulombPi;
    const double kc2 = it.k_cut * it.k_cut;
    const double V = (it.Lx * it.Ly) * it.Lz;
    const double four_kappa2 = 4.0 * (it.kappa * it.kappa);
    size_t K = 0;
    auto component = [&](long m, double L) { return (two_pi * (double)m) / L; };
    for (long mx = 0;; ++mx)
    {
        const double kx = component(mx, it.Lx);
        const double kxx = kx * kx;
        if (!(kxx <= kc2))
            break;
        if (mx > (long)limit + 1)
        {
            *count = limit + 1;
            return;
        }
        // every (mx, my) in range keeps at least one vector, and so does every mz in range: a search that runs past the limit
        // has already decided the answer
        long My = 0;
        while (true)
        {
            const double ky = component(My + 1, it.Ly);
            if (!(kxx + ky * ky <= kc2))
                break;
            if (++My > (long)limit + 1)
            {
                *count = limit + 1;
                return;
            }
        }
        for (long my = -My; my <= My; ++my)
        {
            if (mx == 0 && my < 0)
                continue;
            const double ky = component(my, it.Ly);
            const double kxy = kxx + ky * ky;
            long Mz = 0;
            while (true)
            {
                const double kz = component(Mz + 1, it.Lz);
                if (!(kxy + kz * kz <= kc2))
                    break;
                if (++Mz > (long)limit + 1)
                {
                    *count = limit + 1;
                    return;
                }
            }
            for (long mz = -Mz; mz <= Mz; ++mz)
            {
                if (mx == 0 && my == 0 && mz <= 0)
                    continue;
                const double kz = component(mz, it.Lz);
                const double k2 = kxy + kz * kz;
                if (!(k2 > 0.0 && k2 <= kc2))
                    continue;
                if (++K > limit)
                {
                    *count = K;
                    return;
                }
                if (out)
                    out->push_back(CoulombK {kx, ky, kz, ((4.0 * kCoulombPi) / V) * exp(-k2 / four_kappa2) / k2});
            }
        }
    }
    *count = K;
}

// the tables derived from one item: its partner slots (four a particle, from the exclusion list) and its k-vectors
struct CoulombDerived
{
    std::vector<uint32_t> slots;
    std::vector<CoulombK> ktab;
};

// The status of one item.  `out`, if given, receives the item's derived tables, `out_K` the number of its k-vectors.
int coulomb_item_status(const cavmd_coulomb_item* it, CoulombDerived* out, size_t* out_K)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_force & 15) || ((uintptr_t)it->d_charge & 7) || ((uintptr_t)it->h_exclusions & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N != 0 && (!it->d_pos || !it->d_force || !it->d_charge))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->n_exclusions != 0 && !it->h_exclusions)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_COULOMB_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    if (it->N != 0)
    {
        double cut_sq = 0.0;
        if (!box_ok(it->Lx, it->Ly, it->Lz, &cut_sq))
            return CAVMD_ERR_INVALID_VALUE;
        if (!(isfinite(it->kappa) && it->kappa > 0.0) || !finite_nonnegative(it->r_cut) || !finite_nonnegative(it->k_cut))
            return CAVMD_ERR_INVALID_VALUE;
        if (it->r_cut * it->r_cut > cut_sq)
            return CAVMD_ERR_INVALID_VALUE;
    }
    const int st = partner_slots(it->N, it->h_exclusions, it->n_exclusions, kCoulombMaxExclusions, kCoulombNoPartner,
                                 [](uint32_t partner, uint32_t) { return partner; }, out ? &out->slots : nullptr);
    if (st != CAVMD_OK)
        return st;
    size_t K = 0;
    if (out)
        out->ktab.clear();
    if (it->N != 0)
    {
        coulomb_k_vectors(*it, CAVMD_COULOMB_MAX_K, out ? &out->ktab : nullptr, &K);
        if (K > CAVMD_COULOMB_MAX_K)
            return CAVMD_ERR_CAPACITY;
    }
    if (out_K)
        *out_K = K;
    return CAVMD_OK;
}

CoulombRow coulomb_row(const cavmd_coulomb_item& it)
{
    CoulombRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.charge = it.d_charge;
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx;
    r.Ly = it.Ly;
    r.Lz = it.Lz;
    r.kappa = it.kappa;
    r.rcutsq = it.r_cut * it.r_cut;
    r.n = it.N;
    if (it.N != 0)
    {
        size_t K = 0;
        coulomb_k_vectors(it, CAVMD_COULOMB_MAX_K, nullptr, &K); // the item has been checked: K <= CAVMD_COULOMB_MAX_K
        r.n_k = (unsigned)K;
        r.self_c = it.kappa / kCoulombSqrtPi;
        r.bg_c = kCoulombPi / ((2.0 * ((it.Lx * it.Ly) * it.Lz)) * (it.kappa * it.kappa));
    }
    return r;
}

// what set_items replaces together
struct CoulombTables
{
    DeviceArray<uint4> k_blocks, blocks, partners;
    DeviceArray<CoulombK> ktab;
    DeviceArray<v2d> structure;
    std::vector<uint32_t> offsets; // per item: its first entry of ktab / structure
    CoulombHeader header;
    unsigned lds_n = 2;
};
} // namespace

// workgroups by N descending
struct cavmd_coulomb final : LinkedTable<cavmd_coulomb_item, CoulombRow, CoulombDerived, CoulombTables>
{
    cavmd_coulomb() : LinkedTable([](const cavmd_coulomb_item& it) { return it.N; }, coulomb_row) {}

    int item_status(const cavmd_coulomb_item* it, CoulombDerived* out) const override
    {
        return coulomb_item_status(it, out, nullptr);
    }

    void strip(cavmd_coulomb_item* it) const override
    {
        it->h_exclusions = nullptr;
        it->n_exclusions = 0;
    }

    hipError_t fill(const std::vector<cavmd_coulomb_item>& all, const std::vector<unsigned>& launch,
                    const std::vector<CoulombDerived>& d, CoulombTables* t) const override
    {
        const size_t B = all.size();
        std::vector<uint32_t> partner_base(B), pool;
        std::vector<CoulombK> kpool;
        t->offsets.assign(B, 0);
        unsigned largest = 0;
        for (size_t i = 0; i < B; ++i)
        {
            partner_base[i] = pool_append(&pool, d[i].slots) / kCoulombMaxExclusions;
            t->offsets[i] = pool_append(&kpool, d[i].ktab);
            kpool.push_back(CoulombK {0.0, 0.0, 0.0, 0.0}); // the slot of {Q, 0}
            largest = std::max(largest, all[i].N);
        }
        std::vector<uint4> k_table, table;
        for (unsigned item : launch)
        {
            if (all[item].N == 0)
                continue;
            emit_blocks(&k_table, item, (unsigned)d[item].ktab.size(), kCoulombKRows, t->offsets[item], 0u);
            emit_blocks(&table, item, all[item].N, kCoulombRows, partner_base[item], t->offsets[item]);
        }
        hipError_t e = t->k_blocks.upload(k_table.data(), k_table.size());
        if (e == hipSuccess)
            e = t->blocks.upload(table.data(), table.size());
        if (e == hipSuccess)
            e = t->ktab.upload(kpool.data(), kpool.size());
        if (e == hipSuccess)
            e = t->structure.alloc_zeroed(kpool.size());
        if (e == hipSuccess)
            e = t->partners.upload(pool.data(), pool.size());
        memset(&t->header, 0, sizeof(t->header));
        t->header.k_blocks = t->k_blocks.ptr;
        t->header.blocks = t->blocks.ptr;
        t->header.partners = t->partners.ptr;
        t->header.ktab = t->ktab.ptr;
        t->header.structure = t->structure.ptr;
        t->header.n_k_blocks = (unsigned)k_table.size();
        t->header.n_blocks = (unsigned)table.size();
        t->lds_n = lds_particles(largest);
        return e;
    }
};

extern "C"
{

int cavmd_coulomb_item_check(const cavmd_coulomb_item* it)
{
    return coulomb_item_status(it, nullptr, nullptr);
}

int cavmd_coulomb_k_count(const cavmd_coulomb_item* it, uint32_t* out_K)
{
    if (!out_K)
        return CAVMD_ERR_INVALID_VALUE;
    size_t K = 0;
    const int st = coulomb_item_status(it, nullptr, &K);
    if (st != CAVMD_OK)
        return st;
    *out_K = (uint32_t)K;
    return CAVMD_OK;
}

int cavmd_coulomb_parameters(double r_cut, double accuracy, double* kappa, double* k_cut)
{
    if (!kappa || !k_cut || !(isfinite(r_cut) && r_cut > 0.0) || !(accuracy > 0.0 && accuracy < 1.0))
        return CAVMD_ERR_INVALID_VALUE;
    const double s = sqrt(-log(accuracy));
    *kappa = s / r_cut;
    *k_cut = (2.0 * *kappa) * s;
    return CAVMD_OK;
}

int cavmd_coulomb_order(int* rows, int* j_split, int* k_rows, int* k_split)
{
    if (rows)
        *rows = (int)kCoulombRows;
    if (j_split)
        *j_split = kCoulombJSplit;
    if (k_rows)
        *k_rows = (int)kCoulombKRows;
    if (k_split)
        *k_split = kCoulombKSplit;
    return CAVMD_OK;
}

int cavmd_coulomb_create(cavmd_workspace* ws, size_t n_items, const cavmd_coulomb_item* h_items, cavmd_coulomb** out)
{
    return create_table(ws, n_items, h_items, out, CAVMD_OK, [](cavmd_coulomb*) {});
}

int cavmd_coulomb_destroy(cavmd_coulomb* c)
{
    return destroy_table(c);
}

int cavmd_coulomb_set_items(cavmd_coulomb* c, size_t first, size_t count, const cavmd_coulomb_item* h_items)
{
    return c ? c->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_coulomb_compute(cavmd_coulomb* c, void* stream_)
{
    if (!c)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    const CoulombTables& t = c->tables;
    const size_t lds = coulomb_lds_bytes(t.lds_n);
    // two launches, each noted once it is in flight: a refused second one leaves the first to be waited for
    const int st = c->launch(stream, coulomb_structure_kernel<kCoulombBlock, kCoulombKSplit>, dim3(std::max(t.header.n_k_blocks, 1u)),
                             dim3(kCoulombBlock), lds, c->d_rows.ptr, c->d_header.ptr, t.lds_n);
    if (st != CAVMD_OK)
        return st;
    return c->launch(stream, coulomb_force_kernel<kCoulombBlock, kCoulombJSplit>, dim3(std::max(t.header.n_blocks, 1u)),
                     dim3(kCoulombBlock), lds, c->d_rows.ptr, c->d_header.ptr, t.lds_n);
}

int cavmd_coulomb_structure_device_ptr(cavmd_coulomb* c, const double** out, const uint32_t** h_offsets)
{
    if (!c || (!out && !h_offsets))
        return CAVMD_ERR_INVALID_VALUE;
    if (out)
        *out = reinterpret_cast<const double*>(c->tables.structure.ptr);
    if (h_offsets)
        *h_offsets = c->tables.offsets.data();
    return CAVMD_OK;
}

} // extern "C"
