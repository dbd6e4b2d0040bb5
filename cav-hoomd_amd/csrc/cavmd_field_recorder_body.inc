// cavmd_field_recorder_body.inc -- the body of both field_recorder_batch_kernel templates (cavmd_field_recorder_kernel.hpp),
// included into each.  It is the text of a kernel and not a function the two call, as cavmd_draw_fill_body.inc and
// cavmd_ledger_body.inc are: the kernel that was there before the time rule keeps its device code.  In scope: BLOCK, TIMED (a
// constant expression), the kernel's parameters, and period and rule.
//
// TIMED: the run clock's rule (include/cavmd.h), which thread 0 reads from `rule` in DEVICE memory (FieldRule: the kernel's
// scalar registers are all taken, five more arguments made it spill).  t = the double at time0 + item * time_stride; a row is
// due where rows == 0 or t - last_time >= time_interval (the period is 1); the record's `reserved` double holds t; with
// ref_time_interval > 0 the row-count condition of step 4 is t - last_reference_time >= ref_time_interval.  Behind the rule:
// last_time (n_items doubles), then last_reference_time (n_items), beside the counters.
    constexpr int NW = BLOCK / kWave;
    __shared__ double s_acc[NW][2][kWave];
    __shared__ double s_rho[2 * kFieldMaxK];
    __shared__ double s_F[kFieldMaxRefs + 1]; // [n_refs] holds rho2
    __shared__ uint64_t s_ctl[TIMED ? 6 : 4]; // rows, slot, references, row of the last reference (TIMED: a reference is due by
                                              // time, the clock's bits)
    __shared__ int s_record;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const FieldRow* __restrict__ row = rows + item;
    uint64_t* __restrict__ c_rows = counters + (size_t)kFldRows * n_items + item;
    uint64_t* __restrict__ c_calls = counters + (size_t)kFldCalls * n_items + item;
    uint64_t* __restrict__ c_phase = counters + (size_t)kFldPhase * n_items + item;
    uint64_t* __restrict__ c_slot = counters + (size_t)kFldSlot * n_items + item;
    uint64_t* __restrict__ c_refs = counters + (size_t)kFldRefs * n_items + item;
    uint64_t* __restrict__ c_last = counters + (size_t)kFldLastRef * n_items + item;

    // 1. does this call record?  Thread 0 alone reads the counters (it is also their only writer) and tells the others.
    uint64_t calls = 0, phase = 0;
    if (threadIdx.x == 0)
    {
        calls = *c_calls + 1;
        if constexpr (TIMED) // every decision by the clock is taken here, by the one thread that owns the item's words
        {
            const double* __restrict__ times = reinterpret_cast<const double*>(rule + 1);
            const double now = *reinterpret_cast<const double*>(rule->time0 + (size_t)item * rule->time_stride);
            s_record = *c_rows == 0 || now - times[item] >= rule->time_interval;
            s_ctl[4] = rule->ref_time_interval > 0.0 ? now - times[(size_t)n_items + item] >= rule->ref_time_interval
                                                     : (interval > 0 && *c_rows - *c_last >= interval); // 0: the row count stays
            s_ctl[5] = (uint64_t)__double_as_longlong(now);
        }
        else
        {
            phase = *c_phase + 1;
            s_record = (phase >= period);
        }
        s_ctl[0] = *c_rows;
        s_ctl[1] = *c_slot;
        s_ctl[2] = *c_refs;
        s_ctl[3] = *c_last;
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
    const uint64_t t = s_ctl[0];
    const uint64_t slot = s_ctl[1];
    const unsigned n_refs = (unsigned)s_ctl[2];
    const uint64_t last_ref = s_ctl[3];

    // 2. rho(k): density_partials_kernel's tile loop with "grid" = the four waves of this workgroup
    const char* __restrict__ pos = row->pos;
    const size_t pos_stride = row->stride;
    const unsigned N = row->N;
    const unsigned ntiles = (N + kWave - 1) / kWave;
    const unsigned wave_u = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    const unsigned nchunks = (n_k + kWave - 1) / kWave;
    for (unsigned chunk = 0; chunk < nchunks; ++chunk)
    {
        const unsigned k = chunk * kWave + lane;
        const bool active = k < n_k;
        const double kx = active ? kvec[3 * k + 0] : 0.0;
        const double ky = active ? kvec[3 * k + 1] : 0.0;
        const double kz = active ? kvec[3 * k + 2] : 0.0;
        const double ksum = (fabs(kx) + fabs(ky)) + fabs(kz);
        double re = 0.0, im = 0.0;
        for (unsigned tile = wave_u; tile < ntiles; tile += NW)
        {
            // lane = particle: one coalesced round, used for the tile's coordinate bound and for the rare slow path
            const size_t i = (size_t)tile * kWave + lane;
            double px = 0.0, py = 0.0, pz = 0.0;
            if (i < N)
            {
                const double* p = reinterpret_cast<const double*>(pos + i * pos_stride);
                px = p[0];
                py = p[1];
                pz = p[2];
            }
            const unsigned left = N - tile * kWave;
            const int cnt = left < (unsigned)kWave ? (int)left : kWave; // wave-uniform
            double m = fmax(fmax(fabs(px), fabs(py)), fabs(pz));
            m = fmax(m, dpp_f64<0xB1, 0xF>(m, 0.0));
            m = fmax(m, dpp_f64<0x4E, 0xF>(m, 0.0));
            m = fmax(m, dpp_f64<0x124, 0xF>(m, 0.0));
            m = fmax(m, dpp_f64<0x128, 0xF>(m, 0.0));
            m = fmax(m, __shfl_xor(m, 16, kWave));
            m = fmax(m, __shfl_xor(m, 32, kWave));
            const bool all_finite = !__any(!(fabs(px) < 1.0e300) || !(fabs(py) < 1.0e300) || !(fabs(pz) < 1.0e300));
            if (all_finite && !__any(!(ksum * m < 1.0e8)))
            {
                // fast path: every |k . r| of this tile is below 1e8.  The coordinates come through the scalar cache: the tile
                // address is uniform, and the constant address space tells the compiler what it cannot see through a pointer
                // that was itself loaded from the item table -- this kernel never writes a position.
                const uintptr_t base = (uintptr_t)(pos + (size_t)tile * kWave * pos_stride);
                constexpr int PU = 4;
                int j = 0;
                for (; j + PU <= cnt; j += PU)
                {
                    double x[PU], y[PU], z[PU];
#pragma unroll
                    for (int u = 0; u < PU; ++u)
                    {
                        const FieldConstPtr p = (FieldConstPtr)(base + (size_t)(j + u) * pos_stride);
                        x[u] = p[0];
                        y[u] = p[1];
                        z[u] = p[2];
                    }
#pragma unroll
                    for (int u = 0; u < PU; ++u)
                    {
                        double sn, cs;
                        sincos_reduced(coef, (x[u] * kx + y[u] * ky) + z[u] * kz, sn, cs);
                        re += cs;
                        im += sn;
                    }
                }
                for (; j < cnt; ++j)
                {
                    const FieldConstPtr p0 = (FieldConstPtr)(base + (size_t)j * pos_stride);
                    double s0, c0;
                    sincos_reduced(coef, (p0[0] * kx + p0[1] * ky) + p0[2] * kz, s0, c0);
                    re += c0;
                    im += s0;
                }
            }
            else
            {
                for (int j = 0; j < cnt; ++j)
                {
                    const double x = readlane_f64(px, j), y = readlane_f64(py, j), z = readlane_f64(pz, j);
                    const double kr = (x * kx + y * ky) + z * kz;
                    double sn, cs;
                    if (__any(!(fabs(kr) < 1.0e8))) // wave-uniform; also catches NaN/Inf
                        sincos(kr, &sn, &cs);
                    else
                        sincos_reduced(coef, kr, sn, cs);
                    re += cs;
                    im += sn;
                }
            }
        }
        s_acc[wave][0][lane] = re;
        s_acc[wave][1][lane] = im;
        __syncthreads();
        if (wave == 0)
        {
#pragma unroll
            for (int w = 1; w < NW; ++w) // in wave order, whichever wave arrived first
            {
                re += s_acc[w][0][lane];
                im += s_acc[w][1][lane];
            }
            if (active)
            {
                s_rho[2 * k] = re;
                s_rho[2 * k + 1] = im;
            }
        }
        __syncthreads(); // s_acc is free for the next chunk; after the last one the field is complete in LDS
    }

    // 3. F[r] = (sum over k ascending of (a_r a + b_r b)) / n_k: lane r of wave 0 walks k for reference r, the first lane
    //    of wave 1 does the same with the field itself (rho2).  One rounding per operation, no FMA, the sum starts at +0.
    const size_t field_len = 2 * (size_t)n_k;
    const double inv_count = (double)n_k;
    if (threadIdx.x < n_refs)
    {
        const v2d* __restrict__ ref = reinterpret_cast<const v2d*>(refs + ((size_t)item * max_refs + threadIdx.x) * field_len);
        double acc = 0.0;
#pragma unroll 4
        for (unsigned k = 0; k < n_k; ++k)
        {
            const v2d ab = ref[k];
            acc = acc + (ab.x * s_rho[2 * k] + ab.y * s_rho[2 * k + 1]);
        }
        s_F[threadIdx.x] = acc / inv_count;
    }
    else if (threadIdx.x == (unsigned)kWave)
    {
        double acc = 0.0;
        for (unsigned k = 0; k < n_k; ++k)
            acc = acc + (s_rho[2 * k] * s_rho[2 * k] + s_rho[2 * k + 1] * s_rho[2 * k + 1]);
        s_F[kFieldMaxRefs] = acc / inv_count;
    }
    else if (threadIdx.x < kFieldMaxRefs)
        s_F[threadIdx.x] = 0.0;

    // 4. the field of this call (cavmd_field_recorder_read_fields), and a new reference AFTER the correlation if one is due
    const bool asked = take != nullptr && take[item] != 0;
    bool by_time = false; // TIMED: the interval condition as thread 0 took it, by time or by rows
    if constexpr (TIMED)
        by_time = s_ctl[4] != 0;
    const bool due = n_refs < max_refs
                     && (n_refs == 0 || (TIMED ? by_time : (interval > 0 && t - last_ref >= interval)) || asked);
    double* __restrict__ now = field_now + (size_t)item * field_len;
    for (unsigned i = threadIdx.x; i < field_len; i += BLOCK)
        now[i] = s_rho[i];
    if (due)
    {
        double* __restrict__ dst = refs + ((size_t)item * max_refs + n_refs) * field_len;
        for (unsigned i = threadIdx.x; i < field_len; i += BLOCK)
            dst[i] = s_rho[i];
    }
    __syncthreads();

    // 5. the row with 16-byte stores, then the counters
    if (threadIdx.x == 0)
    {
        v2d* __restrict__ out = reinterpret_cast<v2d*>(series + (size_t)item * capacity + slot);
        const uint64_t word1 = (uint64_t)n_refs | ((uint64_t)(due ? 1u : 0u) << 32);
        const v2d head = {__longlong_as_double((long long)calls), __longlong_as_double((long long)word1)};
        v2d sums = {s_F[kFieldMaxRefs], 0.0};
        if constexpr (TIMED)
            sums.y = __longlong_as_double((long long)s_ctl[5]);
        out[0] = head;
        out[1] = sums;
#pragma unroll
        for (unsigned r = 0; r < kFieldMaxRefs; r += 2)
        {
            const v2d f = {s_F[r], s_F[r + 1]};
            out[2 + r / 2] = f;
        }
        if (due)
        {
            ref_rows[(size_t)item * max_refs + n_refs] = t;
            *c_refs = (uint64_t)n_refs + 1;
            *c_last = t;
            if constexpr (TIMED)
                reinterpret_cast<double*>(rule + 1)[(size_t)n_items + item] = sums.y; // whatever the cause of the reference
        }
        record_counters_store(c_rows, c_calls, c_phase, c_slot, t, slot, capacity, calls);
        if constexpr (TIMED)
            reinterpret_cast<double*>(rule + 1)[item] = sums.y;
    }
