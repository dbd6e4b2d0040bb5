// cavmd_capi.hip -- the workspace of include/cavmd.h and the evaluation of the cavity force on it, on top of the kernels in
// cavmd_force_kernels.hpp and cavmd_persistent_kernel.hpp: create and destroy, the dispatcher, the result ring and its
// getters, profiling, tunables.  The rest of the header is in units of their own: cavmd_observables.hip, and seven units
// for the eleven batch objects ('Translation units and the build graph').  Whatever CAVMD_TEST_HOOKS guards is here,
// and only here.
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
#include "cavmd_force_kernels.hpp"
#include "cavmd_persistent_kernel.hpp"
#include "cavmd_workspace.hpp" // struct cavmd_workspace, and what this unit shares with cavmd_observables.hip

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
constexpr size_t kNtStoreMinN = 200000;       // force stores: neutral at 1e5, -3.6 % at 3e5, -4.3 % at 1e6, -5.8 % at 1e7
constexpr size_t kChargeTemporalMaxN = 25000000; // charges stay temporal while the 8 N bytes fit in the 256 MiB Infinity Cache
                                                 // next to the streams: re-measured in round 2 (the round-1 crossover at
                                                 // 5e6 dated from before the scratch-traffic fix): -8 % per evaluation at
                                                 // 6e6 and 1e7, -5 % at 2e7, tie at 5e7 (profiles/r02/ab_two_launch_knobs.txt)
constexpr int kPersistBlock = 256;
constexpr size_t kPersistMaxLds = 156 * 1024; // dynamic LDS of the single-launch kernel (charges of a block's tiles); 160 KiB per CU
constexpr size_t kPersistSharedLds = 76 * 1024; // default ceiling: two such blocks (+ 1.7 KiB static each) fit on one CU, so two concurrent grids stay resident

static_assert(sizeof(cavmd_double4) == 32, "Scalar4 layout");
static_assert(sizeof(cavmd_int3) == 12, "int3 layout");
static_assert(sizeof(cavmd_params) == 32, "params layout");
static_assert(sizeof(cavmd_result) == 192, "result layout");
} // namespace

// the one way from a workspace to what the batch objects may see of it (cavmd_item_table.hpp)
WorkspaceTie* cavmd_workspace_tie(cavmd_workspace* ws)
{
    return ws;
}

namespace
{
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
    // Load policy.  pos and image are new every step and read once per evaluation: non-temporal on every path.  Charges are
    // temporal on every path while 8 N bytes fit the Infinity Cache: the force map reads them again (measured per evaluation:
    // -8 % at N = 6e6 and 1e7, -5 % at 2e7, tie at 5e7; non-temporal above), and they are the same from step to step.  The
    // single launch reads them temporal always, since it ends far below that size (NT_LOAD's default in
    // cavmd_persistent_kernel.hpp; profiles/charge_temporal/README.md); nt_load governs the two-launch reduction only.
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
        st = ls.launch(0, cavity_small_system_kernel<kSmallBlock>, 1u, kSmallBlock, in.pos2, in.charge, in.image, n, L_typeid,
                       Lx, Ly, Lz, dp, ws->sequence, d_result, host_block(ws), force2);
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
        const SyncState sync {ws->d_granules.ptr, ws->d_epoch.ptr,
                              ws->debug_spin_limit > 0 ? (unsigned)ws->debug_spin_limit : kSpinLimit, ws->debug_late_block,
                              (unsigned)ws->debug_late_ticks, ws->debug_silent_block, &ws->h_ctl.dev->sync_error};
        // the kernel's G and the launch's grid are the same number, set here and nowhere else
        const auto launch = [&](auto kernel) {
            const unsigned G = plan.g1;
            return ls.launch_lds(0, plan.lds_bytes, kernel, G, kPersistBlock, in.pos2, in.charge, in.image, sync.epoch, n, G,
                                 L_typeid, plan.lds_slots | (plan.balanced ? kBalancedBit : 0u), Lx, Ly, Lz, dp, rest_of(sync),
                                 ws->sequence, d_result, host_block(ws), force2);
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
            const unsigned G = plan.g1; // the kernel's G and the launch's grid
            return ls.launch(0, &dipole_partials_aos_kernel<decltype(nt)::value, kReduceBlock, decltype(u)::value>, G,
                             kReduceBlock, in.pos2, in.charge, in.image, n, G, L_typeid, Lx, Ly, Lz, part);
        });
    });
    if (st != CAVMD_OK)
        return st;

    ws->sequence += 1;
    if (plan.path == Path::two_launches)
    {
        // ---- launch 2 of 2: every force-map block folds the partials itself, block 0 publishes the result block
        st = with_constant(kStorePolicies, plan.nt_store, [&](auto s) {
            const unsigned G = plan.g2; // the kernel's G and the launch's grid
            return ls.launch(2, &force_map_aos_fused_kernel<kMapBlock, kMapUnroll, decltype(s)::value>, G, kMapBlock, in.pos2,
                             in.charge, in.image, part.d, part.i, n, G, (int)plan.map_reverse, plan.g1, part.stride, L_typeid, Lx,
                             Ly, Lz, dp, ws->sequence, d_result, host_block(ws), force2);
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
        return ls.launch(0, &dipole_partials_kernel<StridedInput, kReduceBlock, decltype(u)::value>, plan.g1, kReduceBlock,
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

} // extern "C"
