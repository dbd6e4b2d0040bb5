// cavmd_draw_fill_body.inc -- the body of both draw_fill_kernel templates (cavmd_draw_kernel.hpp), included into each.  It is
// the text of a kernel and not a function the two call: as a function, inlined, it changed the register allocation of the
// kernel that was there before end times, whose device code stays what it was.  In scope: BLOCK, END (a constant expression),
// the kernel's parameters, and t_end_all (n_items doubles; not read unless END).
//
// END: the item has an end time, t_end_all[item] (+0: none), held against `elapsed` as the call finds it -- at or past it the
// item is AT REST: both rows are the bytes the two input makers give for dt = 0 with every variate +0 (skip = 1, so both
// half-steps, the bath and the thermostat leave the item alone), no block is consumed and of the state only `finished` is
// written.  A NaN clock compares false and never finishes.
    const unsigned item = blockIdx.x * BLOCK + threadIdx.x;
    if (item >= n_items) // the partly empty last workgroup
        return;
    const DrawRow r = rows[item];
    DrawState st = state_all[item];
    if constexpr (END)
    {
        const double t_end = t_end_all[item];
        if (t_end > 0.0 && st.elapsed >= t_end)
        {
            const double one = __longlong_as_double(1ll);
            if (r.verlet_row)
            {
                double* out = r.verlet_row;
                out[0] = 0.0;
                out[1] = r.gamma;
                out[2] = 0.0;
                out[3] = 0.0;
                out[4] = 0.0;
                out[5] = 0.0;
                out[6] = one;
                out[7] = 0.0;
            }
            if (r.bussi_row)
            {
                double* out = r.bussi_row;
                out[0] = 0.0;
                out[1] = 0.0;
                out[2] = r.tau != 0.0 ? 1.0 : 0.0; // exp(-0 / tau)
                out[3] = r.set_T;
                out[4] = one;
                out[5] = 0.0;
                out[6] = 0.0;
                out[7] = 0.0;
            }
            state_all[item].finished = 1;
            return;
        }
        st.finished = 0;
    }
    const bool adaptive = r.records != nullptr;
    const uint64_t recorded = adaptive ? *r.rows : 0;
    double S = 0.0;
    if (recorded != 0)
        S = r.records[(recorded - 1) % r.capacity].force_mass_sum;

    // ---- the time step ------------------------------------------------------------------------------------------------------
    double dt = r.dt_initial, coeff = r.fixed_coeff, c = r.fixed_c, tolerance = 0.0;
    if (adaptive)
    {
        tolerance = r.tol_target;
        if (r.tol_time_constant != 0.0)
            tolerance = r.tol_target - (r.tol_target - r.tol_initial) * exp(-st.elapsed / r.tol_time_constant);
        if (recorded != 0)
        {
            dt = st.draws != 0 ? st.dt : r.dt_initial; // the last dt used
            if (S > 0.0 && S <= 0x1.fffffffffffffp+1023) // the reference's `if force_mass_sum > 0`, and finite
            {
                dt = sqrt(tolerance / S);
                dt = dt < r.dt_min ? r.dt_min : dt;
                dt = dt > r.dt_max ? r.dt_max : dt;
            }
        }
        coeff = (r.gamma != 0.0 && dt != 0.0) ? sqrt(((6.0 * r.gamma) * r.kT) / dt) : 0.0;
        c = r.tau != 0.0 ? exp(-dt / r.tau) : 0.0;
    }
    const double skip = __longlong_as_double(dt == 0.0 ? 1ll : 0ll);

    // ---- the variates -------------------------------------------------------------------------------------------------------
    const DrawStream s = {(unsigned)st.draws, (unsigned)(st.draws >> 32), item, make_uint2(seed_lo, seed_hi)};
    if (r.verlet_row)
    {
        const uint4 xy = s.block(kDrawPurposeLangevinXY);
        const uint4 z = s.block(kDrawPurposeLangevinZ);
        double* out = r.verlet_row;
        out[0] = dt;
        out[1] = r.gamma;
        out[2] = coeff;
        out[3] = 2.0 * draw_unit(xy.x, xy.y) - 1.0;
        out[4] = 2.0 * draw_unit(xy.z, xy.w) - 1.0;
        out[5] = 2.0 * draw_unit(z.x, z.y) - 1.0;
        out[6] = skip;
        out[7] = 0.0;
    }
    if (r.bussi_row)
    {
        double normal = 0.0, gamma_variate = 0.0;
        if (r.dof != 0.0)
            normal = s.normal(kDrawPurposeNormal);
        if (r.dof > 1.0)
        {
            const double a = (r.dof - 1.0) / 2.0;
            if (a >= 1.0)
                gamma_variate = draw_gamma_ge1(s, a, &st.exhausted);
            else
            {
                const uint4 w = s.block(kDrawPurposeBoost);
                gamma_variate = draw_gamma_ge1(s, a + 1.0, &st.exhausted) * exp(log(draw_log_arg(w.x, w.y)) / a); // u^(1/a)
            }
        }
        double* out = r.bussi_row;
        out[0] = normal;
        out[1] = gamma_variate;
        out[2] = c;
        out[3] = r.set_T;
        out[4] = skip;
        out[5] = 0.0;
        out[6] = 0.0;
        out[7] = 0.0;
    }

    st.draws += 1;
    st.dt = dt;
    st.elapsed = st.elapsed + dt;
    st.tolerance = tolerance;
    state_all[item] = st;
