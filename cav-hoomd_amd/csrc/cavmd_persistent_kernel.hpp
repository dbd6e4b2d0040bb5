// cavmd_persistent_kernel.hpp -- the whole cavity-force evaluation in ONE launch (1024 < N <~ 2.4e6 by default).
//
//   phase 1   every block streams its tiles (pos 32 + charge 8 + image 12 B per particle) exactly as
//             dipole_partials_kernel does -- same tile assignment, same double-double accumulation, same block tree,
//             hence the same per-block partial, bit for bit -- and parks the charges it read in LDS.
//   hand-off  a two-level all-reduce across the (<= 256) workgroups, walking the same fixed tree as the two-launch
//             path's fold (reduce_partials_and_finalize): thread 0 of every block publishes the block's partial as a
//             record of 8-byte {tag, 32-bit value} granules; the first block of every group of 16 consecutive blocks
//             gathers its group's records, folds them (row_fold16) and publishes the group total; every block then
//             gathers the <= 16 group totals and folds them.  Every block obtains the same bits; no float atomics.
//             The last block publishes cavmd_result.
//   phase 2   every block writes the forces of its own tiles from the charges in LDS (dense 16-byte chunks): up to ~5e6
//             particles the charge array is not read a second time (84 instead of 92 bytes per particle cross the memory
//             bus; beyond that the tiles that do not fit in LDS are re-read) and the second launch with its ramp, drain and
//             re-fold prologue disappears.
//
// Inter-workgroup protocol (cdna_hip_programming.md, Guideline 16, form R2 "the data is the flag"): each granule is ONE
// naturally aligned 8-byte relaxed agent-scope atomic (global_store/load_dwordx2 sc1), carries its own tag and is
// validated individually by the reader, so no release/acquire ordering between granules, no separate flag, no fence and
// no dependence on dispatch order, timing or XCD placement are needed -- only that all blocks of the grid are resident
// together (grid <= CUs, one block per CU fits by construction).  Why two levels: a flat all-gather (every block reads
// every record) makes up to 1024 waves spin on the same 320 lines of the memory side -- measured 4.6 us per hand-off at
// N = 1e6 whichever way the waiting was organised (profiles/r02/microbench_persistent_v1_flat_*.txt); here a waiting block
// polls 20 lines, from ONE wave.  The tag is the epoch word of the workspace, read from DEVICE memory at kernel start and
// advanced by the publishing block once it holds the total (every block has published by then, so every block has read it): a
// captured launch replays correctly, nothing needs zeroing between launches.  Grids of at most 16 blocks skip the first
// level (every block gathers the block records itself).
//
// Starvation: when other grids hold CUs, part of this grid cannot start while the rest waits for it.  Every spin is
// bounded; a block that gives up poisons its tiles with NaN, is counted and LEAVES, which lets the missing blocks start; they
// give up in turn (the count rides along with their polls), and the last one, which knows from the count that every record
// is in place, folds them in the same order and writes every tile itself -- late, but the same bits (bail path below).
// An evaluation whose blocks were not ALL counted on the bail path (some had completed before the first give-up) leaves
// epoch[2] (the poison word) set to its launch nonce: every block of every LATER launch reads it with the tag at kernel
// entry and fails at once and as a whole (NaN forces, kSyncFailed), without touching the records or the give-up count of
// the failed launch -- so launches already queued behind a failure, or replays of a captured graph, end
// loudly whatever the slabs and counters were left like; only the host clears the word (cavmd_capi.hip, sync_state_dirty).
#pragma once

#include "cavmd_force_kernels.hpp"

#pragma clang fp contract(off)

// Diagnostic hook (csrc/microbench_persistent.hip): per-block time stamps at numbered points of the kernel; nothing in the product.
#ifndef CAVMD_PSTAMP
#define CAVMD_PSTAMP(k)
#endif

namespace cavmd
{

constexpr int kGranulesPerRecord = 2 * kNumPartDoubles + kNumPartInts; // 9 doubles as 18 halves + lmin + lcnt
constexpr unsigned kSpinLimit = 1000000; // poll rounds of a bounded wait: ~0.2-0.4 s; a healthy wait is microseconds
constexpr unsigned kRepairRounds = 4096; // the last block of a starved evaluation finds every record in place: no real wait

constexpr int kGroup = 16;           // blocks per first-level group = lanes of a DPP row
constexpr unsigned kMaxPersistGrid = kGroup * kGroup;
constexpr unsigned kGroupCopies = 8; // the group totals are published in 8 copies; block b polls copy b % 8, so a line of
                                     // group records has 32 pollers instead of 256 (a one-to-255 broadcast through one
                                     // line costs ~1 us more than through lines with 32 pollers: scripts/dev/pingpong.hip)
constexpr int kPollSleep = 1;        // s_sleep argument between two poll rounds (copies and sleep swept in
                                     // profiles/r03/handoff_knob_sweep.txt)
// Measured and rejected, no longer in the tree (last present in commit 1906464; DESIGN.md 3.8 has one row each): the odd zero
// chunks written during the hand-off (EARLYZ, profiles/r03/microbench_persistent_early_zero_chunks_*.txt), the hybrid
// partition (profiles/r03/microbench_persistent_hybrid_partition_*.txt) and 512-thread blocks (profiles/r02/ab_block512.txt).

struct SyncState
{
    unsigned long long* granules; // kMaxPersistGrid block records, then kGroupCopies x kGroup group records; a record is
                                  // kGranulesPerRecord granules {tag << 32 | value} = 160 contiguous bytes
    unsigned* epoch;              // epoch[0]: tag of the next evaluation (never 0); epoch[1]: blocks of the running evaluation
                                  // that gave up waiting (0 outside a starved evaluation); epoch[2]: poison -- the nonce of
                                  // the launch some block of which gave up, from its first give-up until its last block has
                                  // put the state back in order (or for good, until the host wipes it, if nobody could)
    unsigned spin_limit;          // poll rounds of a bounded wait (kSpinLimit; tests shorten it)
    int late_block;               // fault injection (FAULT instantiation only): this block starts late_ticks of the 100 MHz
    unsigned late_ticks;          // wall clock late, as if its CU had been held by another grid; -1: none
    int silent_block;             // fault injection (FAULT instantiation only): this block never publishes its record, as if
                                  // it were not resident -> the evaluation cannot be completed; -1: none
    unsigned* sync_error;         // the workspace's starvation flag, a fixed word in mapped host memory (kSyncFailed /
                                  // kSyncRepaired; the host consumes it): outside the per-evaluation result slots
};
// SyncState as the kernel receives it: the epoch pointer travels among the leading arguments (it is needed at entry), the rest
// of the state behind them.
struct SyncRest
{
    unsigned long long* granules;
    unsigned spin_limit;
    int late_block;
    unsigned late_ticks;
    int silent_block;
    unsigned* sync_error;
    __host__ __device__ SyncState with_epoch(unsigned* epoch) const
    {
        return SyncState {granules, epoch, spin_limit, late_block, late_ticks, silent_block, sync_error};
    }
};
inline SyncRest rest_of(const SyncState& st)
{
    return SyncRest {st.granules, st.spin_limit, st.late_block, st.late_ticks, st.silent_block, st.sync_error};
}
// lds_slots and `balanced` share one of the leading dwords (block_range needs `balanced` before the first tile load)
constexpr unsigned kBalancedBit = 1u << 31;
// *SyncState::sync_error, and the low bits of HostResult::failed
constexpr unsigned kSyncFailed = 1u;   // some block gave up and nobody could complete the evaluation: its forces hold NaN
constexpr unsigned kSyncRepaired = 2u; // every block gave up; the last one completed the whole evaluation alone: results valid

__device__ __forceinline__ unsigned long long granule_load(const unsigned long long* g)
{
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lane 0's Accum -> the 20 words of a record in LDS (word 2 i = low half, 2 i + 1 = high half of double i)
// (written as 32-bit words, the type they are read back as: no aliasing between double and unsigned accesses to the same LDS)
__device__ __forceinline__ void record_to_lds(unsigned* s_rec, const Accum& a)
{
    const double d[kNumPartDoubles] = {a.hx, a.lx, a.hy, a.ly, a.hz, a.lz, a.sx, a.sy, a.sz};
#pragma unroll
    for (int i = 0; i < kNumPartDoubles; ++i)
    {
        s_rec[2 * i] = (unsigned)__double2loint(d[i]);
        s_rec[2 * i + 1] = (unsigned)__double2hiint(d[i]);
    }
    s_rec[2 * kNumPartDoubles] = (unsigned)a.lmin;
    s_rec[2 * kNumPartDoubles + 1] = (unsigned)a.lcnt;
}

__device__ __forceinline__ void record_from_lds(const unsigned* w, Accum& o)
{
    o.hx = __hiloint2double((int)w[1], (int)w[0]);   o.lx = __hiloint2double((int)w[3], (int)w[2]);
    o.hy = __hiloint2double((int)w[5], (int)w[4]);   o.ly = __hiloint2double((int)w[7], (int)w[6]);
    o.hz = __hiloint2double((int)w[9], (int)w[8]);   o.lz = __hiloint2double((int)w[11], (int)w[10]);
    o.sx = __hiloint2double((int)w[13], (int)w[12]); o.sy = __hiloint2double((int)w[15], (int)w[14]);
    o.sz = __hiloint2double((int)w[17], (int)w[16]);
    o.lmin = (int)w[18];
    o.lcnt = (int)w[19];
}

// Wave 0 (all 64 lanes active): the Accum held by lane 0 -> record `rec` of `copies` consecutive copies of a slab of
// `slab_records` records.  Lane 0 spreads the 20 words over the lanes through `s_pub` (>= 20 words of LDS that only this
// wave touches; a readfirstlane + select chain for the same job compiled to ~100 instructions, 0.3 us); one wave
// instruction then stores three copies (60 lanes, 160 contiguous bytes per copy).  Twenty separate 8-byte write-through
// stores from a single lane would leave the CU one after the other -- the guide's Pitfall 7 in miniature.
__device__ __forceinline__ void publish_record(unsigned long long* slab, unsigned slab_records, unsigned copies, unsigned rec,
                                               unsigned tag, const Accum& a, unsigned* s_pub)
{
    const unsigned lane = threadIdx.x;
    if (lane == 0)
        record_to_lds(s_pub, a);
    // same wave: LDS operations complete in order, no barrier needed
    const unsigned field = lane % kGranulesPerRecord, copy0 = lane / kGranulesPerRecord; // copy0 = 0, 1, 2 (3: idle lanes)
    const unsigned long long granule = ((unsigned long long)tag << 32) | s_pub[field];
    for (unsigned c = copy0; c < copies && copy0 < 3; c += 3)
        __hip_atomic_store(slab + ((size_t)c * slab_records + rec) * kGranulesPerRecord + field, granule, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0 (all 64 lanes active): wait until records first .. first + count - 1 (count <= 16, contiguous in the slab) carry
// `tag` in every granule, then hand record first + l to lane l (identity Accum for l >= count).  A round is 5 coalesced
// wave loads (count * 160 bytes <= 20 lines); every granule is validated by its own tag; the words reach their lanes
// through a 1280-byte LDS transpose that only this wave touches.  own_slot >= 0: record first + own_slot is this block's
// own -- it is taken from `own` (lane 0's registers) instead of from memory, where the block's store may not have landed.
// Gives up after `max_rounds` rounds (1 = a single look; kSpinLimit = the bounded wait).  Returns whether the records
// were complete (wave-uniform).
__device__ __forceinline__ bool gather_records(const unsigned long long* slab, unsigned first, unsigned count, unsigned tag,
                                               unsigned* s_words, Accum& o, unsigned max_rounds, int own_slot,
                                               const Accum& own, const unsigned* giveups = nullptr)
{
    constexpr int ROUNDS = (kGroup * kGranulesPerRecord + kWave - 1) / kWave; // 5
    const unsigned lane = threadIdx.x;
    const unsigned total = count * kGranulesPerRecord;
    const unsigned long long* g = slab + (size_t)first * kGranulesPerRecord;
    unsigned long long x[ROUNDS];
    for (unsigned spins = 1;; ++spins)
    {
        // all five loads in flight together (clamped index instead of a branch per load: hipcc otherwise waits for each
        // load before it issues the next, five round trips per round); with them, where asked for, the count of blocks that
        // have given up on this evaluation: once one has, nobody may complete on its own any more (see the bail path)
        const unsigned gone = giveups ? __hip_atomic_load(giveups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j)
        {
            const unsigned i = j * kWave + lane;
            x[j] = granule_load(g + (i < total ? i : total - 1));
        }
        bool ok = true;
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j)
        {
            const unsigned i = j * kWave + lane;
            const bool mine = own_slot >= 0 && (i < total ? i : total - 1) / kGranulesPerRecord == (unsigned)own_slot;
            ok = ok && (mine || (unsigned)(x[j] >> 32) == tag);
        }
        if (gone != 0)
            return false;
        if (__all(ok))
            break;
        if (spins >= max_rounds)
            return false;
        __builtin_amdgcn_s_sleep(kPollSleep);
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j)
        if ((unsigned)(j * kWave) + lane < total)
            s_words[j * kWave + lane] = (unsigned)x[j];
    // same wave: LDS operations complete in order, no barrier needed
    if (own_slot >= 0 && lane == 0)
        record_to_lds(s_words + own_slot * kGranulesPerRecord, own);
    if (lane < count)
        record_from_lds(s_words + lane * kGranulesPerRecord, o);
    return true;
}

// The particles of one block: `nfull` full tiles at first, first + step, ... and one ragged tile of `tail_count` particles
// at `tail_base`.  Two partitions of the N particles over the G blocks:
//   strided   tile t belongs to block t % G (exactly dipole_partials_kernel's assignment: the single-launch kernel then
//             produces the two-launch path's partials bit for bit -- what the hand-off's parity test leans on);
//   balanced  block b takes the contiguous 64-particle units [b U / G, (b + 1) U / G), U = ceil(N / 64): every block gets
//             the same number of particles to within 64, instead of differing by a whole 512-particle tile (one tile is
//             13 % of a block's share at N = 1e6).
struct BlockRange
{
    size_t first, step, tail_base;
    unsigned nfull, tail_count;
};
template <unsigned TILE>
__device__ __forceinline__ BlockRange block_range(unsigned N, unsigned G, unsigned b, int balanced)
{
    BlockRange r;
    if (balanced)
    {
        const unsigned long long U = ((unsigned long long)N + kWave - 1) / kWave;
        const size_t s = (size_t)(U * b / G) * kWave;
        size_t e = (size_t)(U * (b + 1) / G) * kWave;
        e = e < N ? e : N;
        const size_t n = e > s ? e - s : 0;
        r.first = s;
        r.step = TILE;
        r.nfull = (unsigned)(n / TILE);
        r.tail_base = s + (size_t)r.nfull * TILE;
        r.tail_count = (unsigned)(n - (size_t)r.nfull * TILE);
    }
    else
    {
        const unsigned full_tiles = N / TILE;
        const TileSchedule s = strided_tiles(N, G, b, TILE);
        r.first = s.first;
        r.step = s.step;
        r.nfull = s.nfull;
        r.tail_base = (size_t)full_tiles * TILE;
        r.tail_count = (b == full_tiles % G) ? (unsigned)(N - r.tail_base) : 0;
    }
    return r;
}

extern __shared__ __attribute__((aligned(16))) double s_dyn_charge[];

// thread 0: park_scalars, plus whether the hand-off failed (s_mi: 3 ints here)
__device__ __forceinline__ void park_scalars(double* s_m, int* s_mi, const Scalars& sc, bool ok)
{
    park_scalars(s_m, s_mi, sc);
    s_mi[2] = !ok;
}

// ---- entry: what a block learns about its launch before it touches a particle ----------------------------------------------
struct LaunchTag
{
    unsigned tag;   // this evaluation's tag: the epoch word
    unsigned nonce; // this launch's own name, never 0
    bool poisoned;  // an earlier evaluation could not be completed: this launch fails as a whole
};
__device__ __forceinline__ LaunchTag read_launch_tag(const SyncState& st, uint64_t sequence)
{
    LaunchTag lt;
    lt.tag = __hip_atomic_load(st.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The poison word holds the NONCE of the launch whose blocks raised it.  A nonce of another launch = an earlier evaluation
    // that nobody could complete: this launch fails as a whole (give_up_and_maybe_repair).  This launch's own nonce = blocks of
    // this very grid have given up while this one could not start: the bail path, not a failure yet.
    // The nonce: address of the launch's AQL dispatch packet (grid-uniform, an SGPR pair; consecutive dispatches of a queue --
    // replays of a captured graph included -- occupy different slots of its ring: 128 or 256 bytes apart on gfx950 / ROCm 7.2,
    // scripts/dev/dispatch_id_probe.hip) mixed with the host's sequence number; never 0.
    lt.nonce = ((unsigned)((uintptr_t)__builtin_amdgcn_dispatch_ptr() >> 6) * 2654435761u ^ (unsigned)sequence * 40503u) | 1u;
    const unsigned poison = __hip_atomic_load(st.epoch + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lt.poisoned = poison != 0u && poison != lt.nonce;
    return lt;
}

// ---- phase 1: partial dipole of this block's tiles (every lane's share; the block tree follows); the charges of its first
// lds_slots tiles are parked in LDS -------------------------------------------------------------------------------------------
// first_issued: see accumulate_full_tiles
template <int BLOCK, int UNROLL, int NT_LOAD, class FirstIssued>
__device__ __forceinline__ Accum block_partial(const AosInputT<NT_LOAD>& in, const BlockRange& rg, double Lx, double Ly, double Lz,
                                               int L_typeid, double* s_charge, unsigned lds_slots, FirstIssued&& first_issued)
{
    constexpr unsigned TILE = BLOCK * UNROLL;
    const unsigned tid = threadIdx.x;
    Accum acc;
    const TileSchedule sch {rg.first, rg.step, rg.nfull};
    const auto park_row = [&](unsigned slot, int u, double c) {
        if (slot < lds_slots)
            s_charge[slot * TILE + u * BLOCK + tid] = c;
    };
    // The one call of the rolling loop, spelled out for the A/B policy: tests/test_rolling_schedule_host.py finds the function the
    // kernels share by this call's text, which therefore names its input type in full.
    static_assert(NT_LOAD == 1 || NT_LOAD == 2, "pos and image are always non-temporal here");
    if constexpr (NT_LOAD == 2)
        accumulate_full_tiles<AosInputT<2>, BLOCK, UNROLL>(in, sch, Lx, Ly, Lz, L_typeid, acc, park_row, first_issued);
    else
        accumulate_full_tiles<AosInputT<1>, BLOCK, UNROLL>(in, sch, Lx, Ly, Lz, L_typeid, acc, park_row, first_issued);
    if (rg.tail_count)
        accumulate_ragged_tile<AosInputT<NT_LOAD>, BLOCK, UNROLL>(in, rg.tail_base, rg.tail_count, Lx, Ly, Lz, L_typeid, acc,
                                                            [&](unsigned o, double c) {
                                                                if (rg.nfull < lds_slots)
                                                                    s_charge[rg.nfull * TILE + o] = c;
                                                            });
    return acc;
}

// records -> total: lane l of wave 0 holds the l-th of <= 16 gathered records (identities beyond); their fixed fold, as
// reduce_partials_and_finalize folds 16 consecutive partials
__device__ __forceinline__ Accum fold_gathered(const Accum& o)
{
    Accum t;
    t.merge(o);
    return row_fold16(t);
}

// ---- hand-off: two-level all-reduce across the workgroups (wave 0; the other waves wait at the kernel's barrier) ------------
// Publishes the block's partial `acc`, gathers and folds.  Gives the total and whether it is complete (wave-uniform); the
// protocol is the one at the top of this file.  Gathering is not one function shared with the repair path: the normal second
// level crosses workgroups (the leader publishes, everyone polls a copy), the repair's stays in one wave's LDS.
struct HandOff
{
    Accum total;
    bool ok;
};
template <bool FAULT>
__device__ __forceinline__ HandOff hand_off(const SyncState& st, unsigned G, unsigned b, const LaunchTag& lt, const Accum& acc,
                                            unsigned* s_words)
{
    const unsigned tag = lt.tag;
    unsigned long long* const block_slab = st.granules;
    unsigned long long* const group_slab = st.granules + (size_t)kMaxPersistGrid * kGranulesPerRecord;
    bool ok = !lt.poisoned;
    bool silent = false;
    if constexpr (FAULT) // tests only: this block never publishes, as if it were not resident
        silent = ((int)b == st.silent_block);
    if (!silent && !lt.poisoned)
        publish_record(block_slab, kMaxPersistGrid, 1, b, tag, acc, s_words);
    Accum o, t;
    if (lt.poisoned)
    {
        // nothing is published, gathered or counted
    }
    else if (G <= (unsigned)kGroup)
    {
        // A grid of at most 16 blocks (N up to ~4000) is ONE group: every block gathers the block records itself, its own
        // from registers -- one hop instead of two, and the same fold (the second level would only add zeros).
        ok = gather_records(block_slab, 0, G, tag, s_words, o, st.spin_limit, (int)b, acc, st.epoch + 1);
        CAVMD_PSTAMP(7);
    }
    else
    {
        if ((b & (kGroup - 1)) == 0)
        {
            // Level 1: the first block of group b / 16 gathers the group's records (its own from registers), folds them
            // and publishes the group total.  (Letting EVERY block take one look at its group on arrival, so that the
            // last arriver folds without waiting to be seen, measured slower: 9.30 vs 9.15 us at N = 1e5, 19.9 vs 19.75 at
            // 1e6 -- 240 extra gathers in flight when the last records land.)
            const unsigned count = min(G - b, (unsigned)kGroup);
            Accum o1, t1;
            ok = gather_records(block_slab, b, count, tag, s_words, o1, st.spin_limit, 0, acc);
            // (a group whose gather timed out publishes nothing: every block then times out on the group totals and
            // the whole evaluation fails loudly, instead of a wrong total spreading with a valid tag)
            if (ok)
            {
                t1.merge(o1); // restates fold_gathered (calling it here reorders the hand-off's instructions)
                t1 = row_fold16(t1);
                publish_record(group_slab, kGroup, kGroupCopies, b / kGroup, tag, t1, s_words);
            }
        }
        CAVMD_PSTAMP(7);
        ok = gather_records(group_slab + (size_t)(b % kGroupCopies) * kGroup * kGranulesPerRecord, 0,
                            (G + kGroup - 1) / kGroup, tag, s_words, o, st.spin_limit, -1, acc, st.epoch + 1)
             && ok;
    }
    t.merge(o); // restates fold_gathered
    HandOff h;
    h.total = row_fold16(t);
    h.ok = ok;
    CAVMD_PSTAMP(3);
    return h;
}

// ---- the slow map, all from global memory: tiles t0, t0 + step, ...; NaN everywhere (poison), or the general rule -- no photon:
// zeros (src/CavityForceCompute.cc:145-156); several L-typed particles: force_chunk_typed ---------------------------------------
template <int BLOCK, int UNROLL, int NT_STORE, int NT_LOAD>
__device__ __forceinline__ void slow_map(const AosInputT<NT_LOAD>& in, unsigned N, double g, int L_typeid, v2d* __restrict__ force2,
                                         unsigned t0, unsigned step, bool poison, const MapScalars& ms)
{
    constexpr unsigned TILE = BLOCK * UNROLL;
    constexpr int MU = 2 * UNROLL;
    const unsigned tid = threadIdx.x;
    const size_t nchunks = 2 * (size_t)N;
    const v2d zero = {0.0, 0.0};
    const double nan = __builtin_nan("");
    const double ng = -g;
    const bool odd = tid & 1;
    for (unsigned t = t0; (size_t)t * TILE < N; t += step)
    {
#pragma unroll
        for (int u = 0; u < MU; ++u)
        {
            const size_t k = (size_t)t * 2 * TILE + (size_t)u * BLOCK + tid;
            if (k >= nchunks)
                continue;
            v2d v = zero;
            if (poison)
                v = (v2d) {nan, nan};
            else if (ms.photon >= 0)
            {
                const size_t p = k >> 1;
                const int ptag = __double2loint(in.pos2[2 * p + 1].y);
                v = force_chunk_typed(ms, ng, in.charge[p], k, odd, 2 * (size_t)ms.photon, ptag, L_typeid);
            }
            store_chunk<NT_STORE>(force2 + k, v);
        }
    }
}

// ---- the bail path: this block gave up waiting, because some block of the grid was not resident (other grids hold the CUs) --
// Loud by default: NaN over the block's own tiles and the failure flag.  Then the block LEAVES, which frees its CU for
// the blocks that have not started.  Those find no group totals (the group leaders have left), give up in turn -- and
// the last one to do so, which knows from the count that every block has published its record, completes the whole
// evaluation alone: same records, same fold, same bits; a millisecond instead of microseconds, once, after which the
// host keeps this workspace on two launches.  If some blocks did get the total while others gave up (a race of
// microseconds after a wait of a third of a second), the count never completes and the evaluation stays failed.
template <int BLOCK, int UNROLL, int NT_STORE, int NT_LOAD>
__device__ __forceinline__ void give_up_and_maybe_repair(const AosInputT<NT_LOAD>& in, unsigned N, double Lx, double Ly, double Lz,
                                                         const DeviceParams& prm, int L_typeid, const SyncState& st,
                                                         uint64_t sequence, cavmd_result* __restrict__ res,
                                                         HostResult* __restrict__ res_host, v2d* __restrict__ force2,
                                                         const LaunchTag& lt, const Accum& acc, const PhotonRow& guess,
                                                         const MapScalars& m, double* s_m, int* s_mi, unsigned* s_words,
                                                         unsigned G)
{
    const unsigned b = blockIdx.x, tid = threadIdx.x;
    const unsigned tag = lt.tag;
    unsigned long long* const block_slab = st.granules;
    __shared__ unsigned s_last;
    slow_map<BLOCK, UNROLL, NT_STORE>(in, N, prm.g, L_typeid, force2, b, G, true, m);
    __threadfence();
    __syncthreads();
    if (tid == 0)
    {
        __hip_atomic_store(st.sync_error, kSyncFailed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // this evaluation's own slot says so too, tagged with its sequence (a repair below publishes the result over it)
        __hip_atomic_store(&res_host->failed, (sequence << 2) | kSyncFailed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (lt.poisoned)
            s_last = 0u; // a launch behind an evaluation nobody could complete: fail as a whole, touch nothing
        else
        {
            // poison first (the counting atomic below orders it): it stays unless ALL blocks end up counted here, i.e.
            // unless the last of them can put records, count and epoch back in order
            __hip_atomic_store(st.epoch + 2, lt.nonce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = __hip_atomic_fetch_add(st.epoch + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == G - 1;
        }
    }
    __syncthreads();
    if (!s_last)
        return;
    __shared__ __attribute__((aligned(8))) unsigned s_groups[kGroup * kGranulesPerRecord];
    if (tid < kWave)
    {
        bool ok = true;
        Accum o;
        if (G <= (unsigned)kGroup)
            ok = gather_records(block_slab, 0, G, tag, s_words, o, kRepairRounds, -1, acc);
        else
        {
            const unsigned ngroups = (G + kGroup - 1) / kGroup;
            for (unsigned g = 0; g < ngroups; ++g)
            {
                Accum o1;
                ok = gather_records(block_slab, g * kGroup, min(G - g * kGroup, (unsigned)kGroup), tag, s_words, o1,
                                    kRepairRounds, -1, acc)
                     && ok;
                const Accum t1 = fold_gathered(o1);
                if (tid == 0)
                    record_to_lds(s_groups + g * kGranulesPerRecord, t1);
            }
            // same wave: LDS operations complete in order, no barrier needed
            if (tid < ngroups)
                record_from_lds(s_groups + tid * kGranulesPerRecord, o);
        }
        const Accum tot = fold_gathered(o);
        const Scalars sc = scalars_from_total<AosInputT<NT_LOAD>>(tot, guess, in, N, Lx, Ly, Lz, prm, true);
        if (tid == 0)
        {
            park_scalars(s_m, s_mi, sc, ok);
            if (ok)
            {
                // the verdict first, the result's ready flag (a release) after it: a host that sees the result sees "repaired"
                __hip_atomic_store(st.sync_error, kSyncRepaired, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                write_result(res, sc, N, G, sequence);
                publish_to_host(res_host, sc, N, G, sequence);
            }
        }
    }
    __syncthreads();
    const MapScalars mr = map_scalars_from_lds(s_m, s_mi);
    if (!s_mi[2]) // over the other blocks' NaN: their stores were fenced before they were counted
        slow_map<BLOCK, UNROLL, NT_STORE>(in, N, prm.g, L_typeid, force2, 0, 1, false, mr);
    if (tid == 0)
    {
        // every block has read the epoch and been counted, none is left in the hand-off: count, epoch and poison are put
        // back in order for the next evaluation (whether or not THIS one could be completed: that is the starvation flag's to say)
        __hip_atomic_store(st.epoch + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st.epoch, tag + 1u ? tag + 1u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st.epoch + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- phase 2: forces of this block's own tiles, charges from LDS: the resident tiles, the tiles beyond the LDS budget and the
// ragged tile; every chunk by force_chunk (one photon exactly: the caller has sent the other cases to slow_map) ----------------
template <int BLOCK, int UNROLL, int NT_STORE, int NT_LOAD>
__device__ __forceinline__ void map_own_tiles(const AosInputT<NT_LOAD>& in, const BlockRange& rg, const MapScalars& m, double g,
                                              v2d* __restrict__ force2, const double* s_charge, unsigned lds_slots)
{
    constexpr unsigned TILE = BLOCK * UNROLL;
    constexpr int MU = 2 * UNROLL; // 16-byte chunk stores per thread and tile
    const unsigned tid = threadIdx.x;
    const double ng = -g;
    const size_t pchunk = 2 * (size_t)m.photon; // photon's first chunk
    const bool odd = tid & 1;                   // BLOCK is even, so the half is fixed per thread
    const v2d zero = {0.0, 0.0};
    auto store_tile = [&](unsigned slot, const double (&c)[MU]) {
        const size_t base = 2 * (rg.first + (size_t)slot * rg.step) + tid;
#pragma unroll
        for (int u = 0; u < MU; ++u)
        {
            const size_t k = base + (size_t)u * BLOCK;
            const double s = ng * c[u]; // restates force_chunk (calling it here costs the UNROLL = 1 kernels 2 VGPRs)
            v2d v = {s * m.Dqx, s * m.Dqy};
            v = odd ? zero : v;
            if ((k | 1) == (pchunk | 1))
                v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
            store_chunk<NT_STORE>(force2 + k, v);
        }
    };
    const unsigned resident = rg.nfull < lds_slots ? rg.nfull : lds_slots;
    for (unsigned slot = 0; slot < resident; ++slot)
    {
        double c[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u)
            c[u] = s_charge[slot * TILE + ((u * BLOCK + tid) >> 1)];
        store_tile(slot, c);
    }
    if (resident < rg.nfull)
    {
        // Tiles beyond the LDS budget: their charges are read a second time (as the two-launch path reads all of them), D
        // tiles per batch and two batches in flight (ping-pong register sets): the loads of the next batch are issued before
        // the stores of the current one, so the wave only ever waits for loads that have had a batch of stores to land.
        constexpr int D = 8;
        auto load_batch = [&](unsigned s0, double (&c)[D][MU]) {
#pragma unroll
            for (int d = 0; d < D; ++d)
            {
                const unsigned slot = s0 + d < rg.nfull ? s0 + d : rg.nfull - 1; // clamped: no branch around the loads
                const size_t p0 = rg.first + (size_t)slot * rg.step;
#pragma unroll
                for (int u = 0; u < MU; ++u)
                {
                    const double* q = in.charge + p0 + ((u * BLOCK + tid) >> 1);
                    c[d][u] = (NT_LOAD == 2) ? __builtin_nontemporal_load(q) : *q; // the policy of AosInputT::load
                }
            }
        };
        auto store_batch = [&](unsigned s0, const double (&c)[D][MU]) {
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (s0 + d < rg.nfull)
                    store_tile(s0 + d, c[d]);
        };
        double A[D][MU], B[D][MU];
        load_batch(resident, A);
        for (unsigned s0 = resident; s0 < rg.nfull; s0 += 2 * D)
        {
            if (s0 + D < rg.nfull)
                load_batch(s0 + D, B);
            store_batch(s0, A);
            if (s0 + 2 * D < rg.nfull)
                load_batch(s0 + 2 * D, A);
            if (s0 + D < rg.nfull)
                store_batch(s0 + D, B);
        }
    }
    if (rg.tail_count)
    {
        const size_t base = 2 * rg.tail_base + tid;
#pragma unroll
        for (int u = 0; u < MU; ++u)
        {
            const unsigned o = (u * BLOCK + tid) >> 1; // particle within the ragged tile
            if (o < rg.tail_count)
            {
                const size_t k = base + (size_t)u * BLOCK;
                const double cc = rg.nfull < lds_slots ? s_charge[rg.nfull * TILE + o] : in.charge[rg.tail_base + o];
                store_chunk<NT_STORE>(force2 + k, force_chunk(m, ng, cc, k, odd, pchunk));
            }
        }
    }
}

// ---- the kernel: entry, phase 1, hand-off, scalars through LDS, then the bail path, the slow map or phase 2 -------------------
// The argument block.  Its first twelve dwords -- the three input pointers, the epoch pointer, N, G, L_typeid and lds_slots
// (with kBalancedBit) -- are everything a block needs up to and including the issue of its first tile rows, and they are plain
// pointers and integers: gfx950 hands them to every wave in user SGPRs at wave start (kernel-argument preload, asked for in
// csrc/Makefile; twelve because the dispatch pointer and the argument-block pointer take four of the sixteen user SGPRs), so
// the first loads wait for no fetch of the argument block.  G is the grid's size: gridDim.x sits in the hidden arguments,
// behind the last explicit one, in a line of its own.  A by-value struct in front (AosInputT, as before) disables the preload.
// NT_LOAD is AosInputT's load policy.  The product instantiates the default only: pos and image non-temporal (new every step),
// charge temporal -- the charges of a run do not change from step to step and 8 N bytes are far below the Infinity Cache
// wherever this kernel runs, so they can be found there in the next evaluation, and in this one by the tiles beyond the LDS
// budget that phase 2 reads again.  2 (charges non-temporal too) is kept for the A/B in csrc/microbench_persistent.hip.
template <int BLOCK, int UNROLL, int NT_STORE, bool FAULT = false, int NT_LOAD = 1>
__global__ __launch_bounds__(BLOCK) void cavity_persistent_kernel(const v2d* __restrict__ pos2, const double* __restrict__ charge,
                                                                  const int* __restrict__ image, unsigned* epoch, unsigned N,
                                                                  unsigned G, int L_typeid, unsigned lds_slots_balanced,
                                                                  double Lx, double Ly, double Lz, DeviceParams prm,
                                                                  SyncRest rest, uint64_t sequence,
                                                                  cavmd_result* __restrict__ res,
                                                                  HostResult* __restrict__ res_host, v2d* __restrict__ force2)
{
    constexpr unsigned TILE = BLOCK * UNROLL; // particles per tile; the same tile is 2 * TILE force chunks
    __shared__ double s_m[5];
    __shared__ int s_mi[3];
    double* s_charge = s_dyn_charge;
    const unsigned b = blockIdx.x, tid = threadIdx.x;
    const AosInputT<NT_LOAD> in {pos2, charge, image};
    const SyncState st = rest.with_epoch(epoch);
    const unsigned lds_slots = lds_slots_balanced & ~kBalancedBit;
    const int balanced = (lds_slots_balanced & kBalancedBit) != 0;

    CAVMD_PSTAMP(0);
    if constexpr (FAULT) // tests only: this block starts late, as if its CU had been held by another grid
    {
        if ((int)b == st.late_block)
        {
            const unsigned long long t0 = wall_clock64();
            while (wall_clock64() - t0 < (unsigned long long)st.late_ticks)
                __builtin_amdgcn_s_sleep(64);
        }
    }
    // this evaluation's tag, and the speculative photon row (the driver appends the photon last): vector loads, issued here so
    // that they are older than every tile load; nothing waits for them before scalars_from_total
    const LaunchTag lt = read_launch_tag(st, sequence);
    const PhotonRow guess = speculative_photon_row(in, N);
    // Everything up to here and block_range came out of the preloaded registers.  The arguments behind them (box lengths first:
    // the first row's arithmetic needs them) are fetched by scalar loads (the compiler issues them a few instructions ahead of the
    // first rows, not at entry) and waited for ONCE, when the first tile rows are on their way: they return in the shadow of those
    // rows' own round trip.  Scalar loads return out of order, so the
    // wait is a full lgkmcnt(0); left to the compiler it sits at the first use, inside the tile loop, and there every row also
    // waits for its own LDS store.
    const auto arguments_landed = [&] { asm volatile("" : : "s"(Lx), "s"(Ly), "s"(Lz)); };

    const BlockRange rg = block_range<TILE>(N, G, b, balanced);
    Accum acc = block_partial<BLOCK, UNROLL>(in, rg, Lx, Ly, Lz, L_typeid, s_charge, lds_slots, arguments_landed);
    CAVMD_PSTAMP(1);
    acc = block_reduce<BLOCK>(acc);
    CAVMD_PSTAMP(2);

    __shared__ __attribute__((aligned(8))) unsigned s_words[kGroup * kGranulesPerRecord];
    if (tid < kWave)
    {
        const HandOff h = hand_off<FAULT>(st, G, b, lt, acc, s_words);
        // The block that publishes cavmd_result (a system-scope release: ~0.6 us before its force stores can start) is the
        // LAST block: it holds the fewest tiles (the ragged tail, or one tile less than the first blocks), so the detour is
        // taken from its slack instead of from the kernel's critical path.
        const bool publisher = (b == G - 1);
        const Scalars sc = scalars_from_total<AosInputT<NT_LOAD>>(h.total, guess, in, N, Lx, Ly, Lz, prm, publisher);
        if (tid == 0)
        {
            park_scalars(s_m, s_mi, sc, h.ok);
            if (publisher && h.ok)
            {
                // every block has published, hence read the epoch: advance it for the next launch (0 is never a tag)
                __hip_atomic_store(st.epoch, lt.tag + 1u ? lt.tag + 1u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                write_result(res, sc, N, G, sequence);
                publish_to_host(res_host, sc, N, G, sequence);
            }
        }
    }
    CAVMD_PSTAMP(4);
    __syncthreads();
    CAVMD_PSTAMP(5);
    const MapScalars m = map_scalars_from_lds(s_m, s_mi);
    const bool bad = s_mi[2];

    if (bad)
    {
        give_up_and_maybe_repair<BLOCK, UNROLL, NT_STORE>(in, N, Lx, Ly, Lz, prm, L_typeid, st, sequence, res, res_host, force2, lt,
                                                          acc, guess, m, s_m, s_mi, s_words, G);
        return;
    }
    if (m.photon < 0 || m.nL > 1)
    {
        slow_map<BLOCK, UNROLL, NT_STORE>(in, N, prm.g, L_typeid, force2, b, G, false, m); // rare, from global memory
        return;
    }
    map_own_tiles<BLOCK, UNROLL, NT_STORE>(in, rg, m, prm.g, force2, s_charge, lds_slots);
    CAVMD_PSTAMP(6);
}

} // namespace cavmd
