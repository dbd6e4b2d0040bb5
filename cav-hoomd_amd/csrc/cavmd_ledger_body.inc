// cavmd_ledger_body.inc -- the body of both ledger_batch_kernel templates (cavmd_ledger_kernel.hpp), included into each.  It is
// the text of a kernel and not a function the two call: as a function, inlined, it changed the code of the kernel that was
// there before the time rule, whose device code stays what it was.  In scope: BLOCK, TIMED (a constant expression), the
// kernel's parameters, and period, time_interval, max_time, last_time.
//
// TIMED: the run clock's rule (include/cavmd.h) decides in step 1 instead of the period, which is 1: due = rows == 0 ||
// t - last_time >= time_interval, not due past max_time (> 0), t = *it->time (never NULL under the rule); a row written sets
// last_time[item] = t, a word beside the counters.
    constexpr int UNROLL = kRecorderUnroll;
    constexpr unsigned TILE = BLOCK * UNROLL;
    __shared__ double s_ke[kRecorderMaxTiles][2];
    __shared__ double s_pot[kLedgerTerms][kRecorderMaxTiles][2];
    __shared__ int s_record;

    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const LedgerItem* __restrict__ it = items + item;
    uint64_t* __restrict__ c_rows = counters + (size_t)kRecRows * n_items + item;
    uint64_t* __restrict__ c_calls = counters + (size_t)kRecCalls * n_items + item;
    uint64_t* __restrict__ c_phase = counters + (size_t)kRecPhase * n_items + item;
    uint64_t* __restrict__ c_slot = counters + (size_t)kRecSlot * n_items + item;

    // 1. does this call record?  Thread 0 alone reads the counters (it is also their only writer) and tells the others.
    //    (restates recorder_batch_kernel's step 1, as field_recorder_batch_kernel does: as a shared function it changed the
    //    register counts of the kernels that called it.)
    uint64_t calls = 0, phase = 0;
    if (threadIdx.x == 0)
    {
        calls = *c_calls + 1;
        if constexpr (TIMED)
        {
            const double t = *it->time;
            const bool due = *c_rows == 0 || t - last_time[item] >= time_interval;
            s_record = due && !(max_time > 0.0 && t > max_time);
        }
        else
        {
            phase = *c_phase + 1;
            s_record = (phase >= period);
        }
    }
    __syncthreads();
    if (!s_record)
    {
        if (threadIdx.x == 0)
        {
            *c_calls = calls;
            if constexpr (!TIMED)
                *c_phase = phase;
        }
        return;
    }

    const v2d* __restrict__ vel2 = it->vel2;
    const unsigned* __restrict__ members = it->members;
    const unsigned N = it->N;
    const unsigned n_ke = vel2 ? it->n_members : 0;
    const unsigned tiles_ke = (n_ke + TILE - 1) / TILE;
    const double* energy[kLedgerTerms];
#pragma unroll
    for (int k = 0; k < kLedgerTerms; ++k)
        energy[k] = it->energy[k];
    const unsigned tiles_pot = energy[0] ? (N + TILE - 1) / TILE : 0; // no term follows an absent one

    // 2a. the group's kinetic energy: the recorder's code, one double-double partial per tile
    for (unsigned t = 0; t < tiles_ke; ++t)
    {
        v2d vxy[UNROLL], vzw[UNROLL];
        sum_tile_load<BLOCK, UNROLL>(vel2, members, n_ke, t, vxy, vzw);
        __builtin_amdgcn_sched_barrier(0);
        tile_partial_to_lds<BLOCK>(recorder_kinetic_terms<UNROLL>(vxy, vzw), s_ke, t);
    }
    // 2b. the potential terms: all loads of a tile (up to 4 terms x 4 entries a lane) are in flight before the first addend.
    //     Plain loads: step two and the thermostat read the same lines.
    for (unsigned t = 0; t < tiles_pot; ++t)
    {
        double w[kLedgerTerms][UNROLL];
#pragma unroll
        for (int k = 0; k < kLedgerTerms; ++k)
            ledger_load_w<BLOCK, UNROLL>(energy[k], N, t, w[k]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < kLedgerTerms; ++k)
            if (energy[k]) // the same for the whole workgroup
                tile_partial_to_lds<BLOCK>(ledger_potential_terms<UNROLL>(w[k]), s_pot[k], t);
    }
    const DD ke = recorder_fold<BLOCK>(s_ke, tiles_ke);
    DD pot[kLedgerTerms];
#pragma unroll
    for (int k = 0; k < kLedgerTerms; ++k)
    {
        pot[k] = DD {0.0, 0.0}; // an absent term: +0
        if (energy[k])
            pot[k] = recorder_fold<BLOCK>(s_pot[k], tiles_pot);
    }

    // 3. the row: copied columns as they are, every derived one by its listed expression
    if (threadIdx.x == 0)
    {
        const cavmd_result* __restrict__ res = it->res;
        const uint64_t n_rows = *c_rows;
        const uint64_t slot = *c_slot;
        cavmd_ledger_row row;
        row.call = calls;
        row.n_terms = 0;
        row.n_reservoirs = 0;
        row.time = it->time ? *it->time : 0.0;
#pragma unroll
        for (int k = 0; k < kLedgerTerms; ++k)
        {
            row.n_terms += energy[k] ? 1u : 0u;
            row.potential[k] = pot[k].hi + pot[k].lo;
        }
        double kinetic_cavity = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            row.cavity[k] = res ? res->energy[k] : 0.0;
        if (res)
        {
            const int p = res->photon_idx;
            double mode[4] = {0.0, 0.0, 0.0, 0.0};
            if (p >= 0 && vel2)
            {
                const v2d pxy = vel2[2 * (size_t)p], pzw = vel2[2 * (size_t)p + 1];
                cavity_mode_numbers(pzw.y, pxy.x, pxy.y, pzw.x, row.cavity[0], kB, mode);
            }
            kinetic_cavity = mode[0];
        }
        row.cavity_potential = (row.cavity[0] + row.cavity[1]) + row.cavity[2];
        row.potential_total = (((row.potential[0] + row.potential[1]) + row.potential[2]) + row.potential[3]) + row.cavity_potential;
        row.kinetic_group = 0.5 * (ke.hi + ke.lo);
        row.kinetic_cavity = kinetic_cavity;
        row.kinetic_total = it->add_cavity_kinetic ? row.kinetic_group + row.kinetic_cavity : row.kinetic_group;
        row.system_total = row.kinetic_total + row.potential_total;
#pragma unroll
        for (int k = 0; k < kLedgerReservoirs; ++k)
        {
            const double* __restrict__ r = it->reservoir[k];
            row.n_reservoirs += r ? 1u : 0u;
            row.reservoir[k] = r ? *r : 0.0;
        }
        row.reservoir_total = ((row.reservoir[0] + row.reservoir[1]) + row.reservoir[2]) + row.reservoir[3];
        row.universe_total = row.system_total + row.reservoir_total;
        const double dof = it->dof;
        row.temperature = dof == 0.0 ? 0.0 : (2.0 * row.kinetic_group) / (dof * kB);
        row.reserved = 0.0;
        // twelve 16-byte stores: the series is allocated by the library, 192 bytes a row
        __builtin_memcpy(__builtin_assume_aligned(series + (size_t)item * capacity + slot, 16), &row, sizeof(row));
        record_counters_store(c_rows, c_calls, c_phase, c_slot, n_rows, slot, capacity, calls);
        if constexpr (TIMED)
            last_time[item] = row.time;
    }
