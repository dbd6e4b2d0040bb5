// cavmd_verlet.hip -- cavmd_verlet of include/cavmd.h: the velocity-Verlet half-steps of a batch of small systems, one launch
// each; and cavmd_draw, which writes the input rows those half-steps (and the thermostat batch) read: seeded variates and the
// step's dt, one launch per step; and cavmd_bath, created from an integrator, whose launch takes the place of the integrator's
// second half-step with a Langevin bath on any set of particles; and cavmd_thermalize, which starts a run: seeded momenta and
// the photon's placement, one launch.  Four of the eleven objects built on an item table (cavmd_item_table.hpp), each a
// StateTable; the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "cavmd.h"
#include "cavmd_verlet_batch_kernel.hpp"
#include "cavmd_mts_verlet_kick_kernel.hpp"
#include "cavmd_draw_kernel.hpp"
#include "cavmd_bath_kernel.hpp"
#include "cavmd_thermalize_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- the velocity-Verlet step of a batch of independent small systems, one launch per half-step (cavmd_verlet_batch_kernel.hpp) --
struct cavmd_verlet : StateTable<cavmd_verlet_item, VerletRow, VerletState> // launched by N descending
{
    WorkspaceTie bath_tie; // the parent's tie of the cavmd_bath objects created from this integrator (cavmd_verlet_destroy)

    cavmd_verlet()
        : StateTable(cavmd_verlet_item_check, [](const cavmd_verlet_item& it) { return it.N; },
                     uploaded_as_it_is<cavmd_verlet_item, VerletRow>)
    {
    }

    // one launch of n workgroups of one of the three kernels
    template <class Kernel>
    int launch_step(void* stream, Kernel kernel, const cavmd_verlet_input* d_inputs)
    {
        return launch((hipStream_t)stream, kernel, dim3((unsigned)n), dim3(256), 0, d_rows.ptr, d_order.ptr,
                      reinterpret_cast<const VerletInput*>(d_inputs), d_state.ptr);
    }

    cavmd_snapshot_header snapshot_shape() const
    {
        return state_shape(CAVMD_SNAPSHOT_VERLET, 0, 0);
    }
};

// ---- the step inputs of a batch drawn on the device, one launch per step (cavmd_draw_kernel.hpp) ------------------------------
// the row of an item: the item, with the fixed-mode columns taken by the two input makers in its reserved words
static DrawRow draw_row(const cavmd_draw_item& it)
{
    static_assert(sizeof(DrawRow) == sizeof(cavmd_draw_item), "a draw row is the item with two words filled in");
    DrawRow r;
    memcpy(&r, &it, sizeof(r));
    const double zero[3] = {0.0, 0.0, 0.0};
    cavmd_verlet_input v;
    cavmd_bussi_batch_input b;
    (void)cavmd_verlet_input_make(it.dt_initial, it.langevin_gamma, it.langevin_kT, zero, &v);
    (void)cavmd_bussi_batch_input_make(it.dt_initial, it.bussi_set_T, it.bussi_tau, 0.0, 0.0, &b);
    r.fixed_coeff = v.langevin_coeff;
    r.fixed_c = b.c;
    return r;
}

struct cavmd_draw : StateTable<cavmd_draw_item, DrawRow, DrawState> // items cost the same: launched in item order
{
    uint64_t seed = 0;
    // the run clock's end times (cavmd_runclock_draw_set_end): none until the first call, which allocates the device array once
    // and for good -- a captured launch reads the values its replay finds there
    std::vector<double> t_end;
    DeviceArray<double> d_t_end;

    cavmd_draw() : StateTable(cavmd_draw_item_check, [](const cavmd_draw_item&) { return 0u; }, draw_row) {}

    // (the seed is a word of the shape: states drawn under another seed do not continue this object's sequence)
    cavmd_snapshot_header snapshot_shape() const
    {
        return state_shape(CAVMD_SNAPSHOT_DRAW, (uint32_t)seed, (uint32_t)(seed >> 32));
    }
};

// ---- a Langevin bath on any set of particles of every item, drawn in step two (cavmd_bath_kernel.hpp) --------------------------
// Item i belongs to item i of the integrator `v`, whose rows, launch order and states the one kernel reads as well; the launch
// goes through the integrator's table, which notes the stream, and is noted here too.
struct cavmd_bath : StateTable<cavmd_bath_item, BathRow, BathState> // tied to v->bath_tie
{
    cavmd_verlet* v = nullptr;

    cavmd_bath()
        : StateTable(cavmd_bath_item_check, [](const cavmd_bath_item& it) { return it.N; },
                     uploaded_as_it_is<cavmd_bath_item, BathRow>)
    {
    }

    cavmd_snapshot_header snapshot_shape() const
    {
        return state_shape(CAVMD_SNAPSHOT_BATH, 0, 0);
    }
};

// ---- the start of a batch: seeded momenta and the photon's placement, one launch (cavmd_thermalize_kernel.hpp) ----------------
struct cavmd_thermalize : StateTable<cavmd_thermalize_item, ThermalizeRow, ThermalizeState> // launched by N descending
{
    cavmd_thermalize()
        : StateTable(cavmd_thermalize_item_check, [](const cavmd_thermalize_item& it) { return it.N; },
                     uploaded_as_it_is<cavmd_thermalize_item, ThermalizeRow>)
    {
    }

    cavmd_snapshot_header snapshot_shape() const
    {
        return state_shape(CAVMD_SNAPSHOT_THERMALIZE, 0, 0);
    }
};

namespace
{
static_assert(offsetof(cavmd_thermalize_item, d_vel) == offsetof(ThermalizeRow, vel2)
                  && offsetof(cavmd_thermalize_item, d_members) == offsetof(ThermalizeRow, members)
                  && offsetof(cavmd_thermalize_item, d_pos) == offsetof(ThermalizeRow, pos2)
                  && offsetof(cavmd_thermalize_item, d_image) == offsetof(ThermalizeRow, image)
                  && offsetof(cavmd_thermalize_item, d_result) == offsetof(ThermalizeRow, res)
                  && offsetof(cavmd_thermalize_item, seed) == offsetof(ThermalizeRow, seed)
                  && offsetof(cavmd_thermalize_item, kT) == offsetof(ThermalizeRow, kT)
                  && offsetof(cavmd_thermalize_item, N) == offsetof(ThermalizeRow, n)
                  && offsetof(cavmd_thermalize_item, n_members) == offsetof(ThermalizeRow, n_members)
                  && offsetof(cavmd_thermalize_item, flags) == offsetof(ThermalizeRow, flags)
                  && offsetof(cavmd_thermalize_item, L) == offsetof(ThermalizeRow, L)
                  && offsetof(cavmd_thermalize_item, params) == offsetof(ThermalizeRow, omegac)
                  && offsetof(cavmd_thermalize_item, params) + offsetof(cavmd_params, couplstr) == offsetof(ThermalizeRow, couplstr)
                  && offsetof(cavmd_thermalize_item, params) + offsetof(cavmd_params, K) == offsetof(ThermalizeRow, K)
                  && sizeof(cavmd_thermalize_item) == sizeof(ThermalizeRow),
              "thermalize item layout");
static_assert(sizeof(cavmd_thermalize_state) == sizeof(ThermalizeState)
                  && offsetof(cavmd_thermalize_state, draws) == offsetof(ThermalizeState, draws)
                  && offsetof(cavmd_thermalize_state, thermalised) == offsetof(ThermalizeState, thermalised)
                  && offsetof(cavmd_thermalize_state, skipped) == offsetof(ThermalizeState, skipped)
                  && offsetof(cavmd_thermalize_state, momentum) == offsetof(ThermalizeState, momentum)
                  && offsetof(cavmd_thermalize_state, photon) == offsetof(ThermalizeState, photon),
              "the thermalize states are read out as they are");
static_assert(CAVMD_THERMALIZE_ZERO_MOMENTUM == kThermalizeZeroMomentum && CAVMD_THERMALIZE_PLACE_PHOTON == kThermalizePlacePhoton
                  && CAVMD_THERMALIZE_FINITE_Q == kThermalizeFiniteQ && CAVMD_THERMALIZE_PHOTON_VELOCITY == kThermalizePhotonVelocity
                  && CAVMD_THERMALIZE_TILE == kThermalizeTile,
              "the flags and the tile the header publishes");
static_assert(offsetof(cavmd_result, photon_idx) == 136 && offsetof(cavmd_result, n_particles) == 144, "the result block's words");
static_assert(offsetof(cavmd_bath_item, d_gamma) == offsetof(BathRow, gamma) && offsetof(cavmd_bath_item, seed) == offsetof(BathRow, seed)
                  && offsetof(cavmd_bath_item, kT) == offsetof(BathRow, kT) && offsetof(cavmd_bath_item, N) == offsetof(BathRow, n)
                  && sizeof(cavmd_bath_item) == sizeof(BathRow),
              "bath item layout");
static_assert(sizeof(cavmd_bath_state) == sizeof(BathState) && offsetof(cavmd_bath_state, draws) == offsetof(BathState, draws)
                  && offsetof(cavmd_bath_state, coupled) == offsetof(BathState, coupled)
                  && offsetof(cavmd_bath_state, reservoir) == offsetof(BathState, reservoir),
              "the bath states are read out as they are");
static_assert(offsetof(cavmd_draw_item, d_verlet_row) == offsetof(DrawRow, verlet_row)
                  && offsetof(cavmd_draw_item, d_bussi_row) == offsetof(DrawRow, bussi_row)
                  && offsetof(cavmd_draw_item, d_records) == offsetof(DrawRow, records)
                  && offsetof(cavmd_draw_item, d_rows) == offsetof(DrawRow, rows)
                  && offsetof(cavmd_draw_item, capacity) == offsetof(DrawRow, capacity)
                  && offsetof(cavmd_draw_item, langevin_gamma) == offsetof(DrawRow, gamma)
                  && offsetof(cavmd_draw_item, langevin_kT) == offsetof(DrawRow, kT)
                  && offsetof(cavmd_draw_item, bussi_set_T) == offsetof(DrawRow, set_T)
                  && offsetof(cavmd_draw_item, bussi_tau) == offsetof(DrawRow, tau)
                  && offsetof(cavmd_draw_item, bussi_dof) == offsetof(DrawRow, dof)
                  && offsetof(cavmd_draw_item, dt_initial) == offsetof(DrawRow, dt_initial)
                  && offsetof(cavmd_draw_item, tolerance_target) == offsetof(DrawRow, tol_target)
                  && offsetof(cavmd_draw_item, tolerance_initial) == offsetof(DrawRow, tol_initial)
                  && offsetof(cavmd_draw_item, tolerance_time_constant) == offsetof(DrawRow, tol_time_constant)
                  && offsetof(cavmd_draw_item, dt_min) == offsetof(DrawRow, dt_min)
                  && offsetof(cavmd_draw_item, dt_max) == offsetof(DrawRow, dt_max)
                  && offsetof(cavmd_draw_item, reserved) == offsetof(DrawRow, fixed_coeff),
              "draw item layout");
static_assert(sizeof(cavmd_draw_state) == sizeof(DrawState) && offsetof(cavmd_draw_state, draws) == offsetof(DrawState, draws)
                  && offsetof(cavmd_draw_state, dt) == offsetof(DrawState, dt)
                  && offsetof(cavmd_draw_state, elapsed) == offsetof(DrawState, elapsed)
                  && offsetof(cavmd_draw_state, tolerance) == offsetof(DrawState, tolerance)
                  && offsetof(cavmd_draw_state, exhausted) == offsetof(DrawState, exhausted)
                  && offsetof(cavmd_draw_state, reserved) == offsetof(DrawState, finished),
              "the draw states are read out as they are");
static_assert(sizeof(cavmd_record) == sizeof(DrawRecord)
                  && offsetof(cavmd_record, force_mass_sum) == offsetof(DrawRecord, force_mass_sum),
              "the record column the adaptive rule reads");
static_assert(offsetof(cavmd_verlet_input, skip) == 48 && offsetof(cavmd_bussi_batch_input, skip) == 32
                  && sizeof(cavmd_bussi_batch_input) == 64,
              "the rows the draw kernel writes word by word");
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
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [](cavmd_verlet* v) { v->bath_tie.device = v->device; });
}

int cavmd_verlet_destroy(cavmd_verlet* v)
{
    // as cavmd_destroy has it for its dependents: nothing is freed while a bath of this integrator lives
    if (v && v->bath_tie.dependents != 0)
        return CAVMD_ERR_INVALID_VALUE;
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

int cavmd_mts_verlet_kick(cavmd_verlet* v, void* stream_, const cavmd_verlet_input* d_inputs, const cavmd_double4* const* d_forces,
                      double weight)
{
    if (!v || !d_inputs || ((uintptr_t)d_inputs & 7) || !d_forces || ((uintptr_t)d_forces & 7) || !isfinite(weight))
        return CAVMD_ERR_INVALID_VALUE;
    return v->launch((hipStream_t)stream_, verlet_kick_kernel<256>, dim3((unsigned)v->n), dim3(256), 0, v->d_rows.ptr, v->d_order.ptr,
                     reinterpret_cast<const VerletInput*>(d_inputs), reinterpret_cast<const v2d* const*>(d_forces), weight);
}

int cavmd_verlet_read(cavmd_verlet* v, void* stream_, cavmd_verlet_state* out)
{
    return v ? v->read((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_verlet_reset(cavmd_verlet* v, void* stream_)
{
    return v ? v->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_verlet_state_device_ptr(cavmd_verlet* v, const cavmd_verlet_state** out)
{
    return v ? v->state_device_ptr(out) : CAVMD_ERR_INVALID_VALUE;
}

// (the one snapshot entry point that belongs to no object: host arithmetic, cavmd_snapshot.hpp)
int cavmd_snapshot_check(const void* blob, size_t bytes, const cavmd_snapshot_header* expected)
{
    return snapshot_check(blob, bytes, expected);
}

int cavmd_snapshot_verlet_bytes(cavmd_verlet* v, size_t* bytes)
{
    return snapshot_bytes(v, bytes);
}

int cavmd_snapshot_verlet_save(cavmd_verlet* v, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(v, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_verlet_load(cavmd_verlet* v, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(v, (hipStream_t)stream_, h_in, bytes);
}

// ---- cavmd_draw ------------------------------------------------------------------------------------------------------------
int cavmd_draw_item_check(const cavmd_draw_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 4; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_verlet_row & 7) || ((uintptr_t)it->d_bussi_row & 7) || ((uintptr_t)it->d_records & 7)
        || ((uintptr_t)it->d_rows & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (!it->d_verlet_row && !it->d_bussi_row)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->d_records && (!it->d_rows || it->capacity == 0))
        return CAVMD_ERR_INVALID_VALUE;
    const double values[] = {it->langevin_gamma,    it->langevin_kT,       it->bussi_set_T, it->bussi_tau,
                             it->bussi_dof,         it->dt_initial,        it->tolerance_target,
                             it->tolerance_initial, it->tolerance_time_constant, it->dt_min, it->dt_max};
    for (double x : values)
        if (!finite_nonnegative(x))
            return CAVMD_ERR_INVALID_VALUE;
    if (it->dt_min > it->dt_max)
        return CAVMD_ERR_INVALID_VALUE;
    return CAVMD_OK;
}

int cavmd_draw_create(cavmd_workspace* ws, uint64_t seed, size_t n_items, const cavmd_draw_item* h_items, cavmd_draw** out)
{
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [seed](cavmd_draw* d) { d->seed = seed; });
}

int cavmd_draw_destroy(cavmd_draw* d)
{
    return destroy_table(d);
}

int cavmd_draw_set_items(cavmd_draw* d, size_t first, size_t count, const cavmd_draw_item* h_items)
{
    return d ? d->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_draw_fill(cavmd_draw* d, void* stream_)
{
    if (!d)
        return CAVMD_ERR_INVALID_VALUE;
    const dim3 grid((unsigned)((d->n + kDrawBlock - 1) / kDrawBlock));
    if (d->d_t_end.ptr) // the variant is chosen here: a launch captured before the first end time stays the old kernel
        return d->launch((hipStream_t)stream_, draw_fill_kernel<kDrawBlock, true>, grid, dim3(kDrawBlock), 0, d->d_rows.ptr,
                         (unsigned)d->n, (unsigned)d->seed, (unsigned)(d->seed >> 32), d->d_state.ptr,
                         (const double*)d->d_t_end.ptr);
    return d->launch((hipStream_t)stream_, draw_fill_kernel<kDrawBlock>, grid, dim3(kDrawBlock), 0, d->d_rows.ptr, (unsigned)d->n,
                     (unsigned)d->seed, (unsigned)(d->seed >> 32), d->d_state.ptr);
}

int cavmd_draw_read(cavmd_draw* d, void* stream_, cavmd_draw_state* out)
{
    return d ? d->read((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_draw_reset(cavmd_draw* d, void* stream_)
{
    return d ? d->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_draw_state_device_ptr(cavmd_draw* d, const cavmd_draw_state** out)
{
    return d ? d->state_device_ptr(out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_draw_bytes(cavmd_draw* d, size_t* bytes)
{
    return snapshot_bytes(d, bytes);
}

int cavmd_snapshot_draw_save(cavmd_draw* d, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(d, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_draw_load(cavmd_draw* d, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(d, (hipStream_t)stream_, h_in, bytes);
}

// ---- the run clock of cavmd_draw: an end time per item, and how many items rest behind theirs ----------------------------------
int cavmd_runclock_draw_set_end(cavmd_draw* d, size_t first, size_t count, const double* h_t_end)
{
    if (!d || !h_t_end || count == 0 || first >= d->n || count > d->n - first)
        return CAVMD_ERR_INVALID_VALUE;
    for (size_t i = 0; i < count; ++i)
        if (!finite_nonnegative(h_t_end[i]))
            return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(d->device);
    const int st = d->wait_idle(); // as set_items: refused while the last stream is being captured
    if (st != CAVMD_OK)
        return st;
    std::vector<double> all(d->t_end);
    all.resize(d->n, 0.0);
    for (size_t i = 0; i < count; ++i)
        all[first + i] = h_t_end[i] + 0.0; // -0 is +0: none
    // The flags first: whether one of these items rests is decided again by the next launch, and until then it does not count
    // as finished.  Should the copy of the end times fail after this one went through, end times and host stay as they were and
    // the next launch sets the flags again by the old end times: nothing is left half-changed.
    const std::vector<uint64_t> zero(count, 0);
    CAVMD_HIP_TRY(hipMemcpy2D(&d->d_state.ptr[first].finished, sizeof(DrawState), zero.data(), sizeof(uint64_t), sizeof(uint64_t),
                              count, hipMemcpyHostToDevice));
    if (!d->d_t_end.ptr)
        CAVMD_HIP_TRY(d->d_t_end.upload(all.data(), d->n));
    else
        CAVMD_HIP_TRY(hipMemcpy(d->d_t_end.ptr + first, all.data() + first, sizeof(double) * count, hipMemcpyHostToDevice));
    d->t_end.swap(all); // only now: a failed copy leaves the host's view as it was
    return CAVMD_OK;
}

int cavmd_runclock_draw_finished(cavmd_draw* d, void* stream_, uint64_t* n_finished)
{
    if (!d || !n_finished)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(d->device);
    int st = d->wait_idle(); // the stream of the last fill, as every call of this section; then the caller's
    if (st == CAVMD_OK)
        st = sync_uncaptured((hipStream_t)stream_);
    if (st != CAVMD_OK)
        return st;
    std::vector<uint64_t> flags(d->n);
    CAVMD_HIP_TRY(hipMemcpy2D(flags.data(), sizeof(uint64_t), &d->d_state.ptr->finished, sizeof(DrawState), sizeof(uint64_t), d->n,
                              hipMemcpyDeviceToHost));
    uint64_t count = 0;
    for (uint64_t f : flags)
        count += f != 0;
    *n_finished = count;
    return CAVMD_OK;
}

// ---- cavmd_bath ------------------------------------------------------------------------------------------------------------
int cavmd_bath_item_check(const cavmd_bath_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 4; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if ((uintptr_t)it->d_gamma & 7)
        return CAVMD_ERR_INVALID_VALUE;
    if ((it->d_gamma == nullptr) != (it->N == 0))
        return CAVMD_ERR_INVALID_VALUE;
    if (!finite_nonnegative(it->kT))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

// as create_table has it, with the integrator's bath_tie as the parent's: the bath counts among the integrator's dependents
int cavmd_bath_create(cavmd_verlet* v, size_t n_items, const cavmd_bath_item* h_items, cavmd_bath** out)
{
    return create_table(v ? &v->bath_tie : nullptr, n_items, h_items, out,
                        v && n_items == v->n ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE, [v](cavmd_bath* b) { b->v = v; });
}

int cavmd_bath_destroy(cavmd_bath* b)
{
    return destroy_table(b);
}

int cavmd_bath_set_items(cavmd_bath* b, size_t first, size_t count, const cavmd_bath_item* h_items)
{
    return b ? b->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_bath_step_two(cavmd_bath* b, void* stream_, const cavmd_verlet_input* d_inputs)
{
    if (!b || !d_inputs || ((uintptr_t)d_inputs & 7))
        return CAVMD_ERR_INVALID_VALUE;
    cavmd_verlet* v = b->v;
    const int st = v->launch((hipStream_t)stream_, verlet_step_two_bath_kernel<256>, dim3((unsigned)v->n), dim3(256), 0, v->d_rows.ptr,
                             v->d_order.ptr, reinterpret_cast<const VerletInput*>(d_inputs), v->d_state.ptr, b->d_rows.ptr,
                             b->d_state.ptr);
    if (st == CAVMD_OK) // the integrator has noted the stream; so does the bath, for its own set_items and destroy
    {
        b->last_stream = (hipStream_t)stream_;
        b->enqueued = true;
    }
    return st;
}

int cavmd_bath_read(cavmd_bath* b, void* stream_, cavmd_bath_state* out)
{
    return b ? b->read((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_bath_reset(cavmd_bath* b, void* stream_)
{
    return b ? b->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_bath_state_device_ptr(cavmd_bath* b, const cavmd_bath_state** out)
{
    return b ? b->state_device_ptr(out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_bath_bytes(cavmd_bath* b, size_t* bytes)
{
    return snapshot_bytes(b, bytes);
}

int cavmd_snapshot_bath_save(cavmd_bath* b, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(b, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_bath_load(cavmd_bath* b, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(b, (hipStream_t)stream_, h_in, bytes);
}

// ---- cavmd_thermalize ------------------------------------------------------------------------------------------------------
int cavmd_thermalize_item_check(const cavmd_thermalize_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 4; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    constexpr uint32_t known = CAVMD_THERMALIZE_ZERO_MOMENTUM | CAVMD_THERMALIZE_PLACE_PHOTON | CAVMD_THERMALIZE_FINITE_Q
                               | CAVMD_THERMALIZE_PHOTON_VELOCITY;
    if (it->flags & ~known)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_members & 3) || ((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_image & 3)
        || ((uintptr_t)it->d_result & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N != 0 && !it->d_vel)
        return CAVMD_ERR_INVALID_VALUE;
    if (!it->d_members && it->n_members != 0)
        return CAVMD_ERR_INVALID_VALUE;
    const double values[] = {it->kT,           it->L[0],          it->L[1],    it->L[2],
                             it->params.omegac, it->params.couplstr, it->params.K, it->params.phmass};
    for (double x : values)
        if (!finite_nonnegative(x))
            return CAVMD_ERR_INVALID_VALUE;
    if ((it->flags & CAVMD_THERMALIZE_FINITE_Q) && !it->d_result)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->flags & CAVMD_THERMALIZE_PLACE_PHOTON)
    {
        if (!it->d_pos || !it->d_image || !it->d_result)
            return CAVMD_ERR_INVALID_VALUE;
        // the placement divides by every edge and by K
        if (it->L[0] == 0.0 || it->L[1] == 0.0 || it->L[2] == 0.0 || it->params.K == 0.0)
            return CAVMD_ERR_INVALID_VALUE;
    }
    if (it->N > CAVMD_BATCH_MAX_ITEM_N || it->n_members > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_thermalize_create(cavmd_workspace* ws, size_t n_items, const cavmd_thermalize_item* h_items, cavmd_thermalize** out)
{
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [](cavmd_thermalize*) {});
}

int cavmd_thermalize_destroy(cavmd_thermalize* t)
{
    return destroy_table(t);
}

int cavmd_thermalize_set_items(cavmd_thermalize* t, size_t first, size_t count, const cavmd_thermalize_item* h_items)
{
    return t ? t->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_thermalize_run(cavmd_thermalize* t, void* stream_)
{
    if (!t)
        return CAVMD_ERR_INVALID_VALUE;
    return t->launch((hipStream_t)stream_, thermalize_batch_kernel<256>, dim3((unsigned)t->n), dim3(256), 0, t->d_rows.ptr,
                     t->d_order.ptr, t->d_state.ptr);
}

int cavmd_thermalize_read(cavmd_thermalize* t, void* stream_, cavmd_thermalize_state* out)
{
    return t ? t->read((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_thermalize_reset(cavmd_thermalize* t, void* stream_)
{
    return t ? t->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_thermalize_state_device_ptr(cavmd_thermalize* t, const cavmd_thermalize_state** out)
{
    return t ? t->state_device_ptr(out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_thermalize_bytes(cavmd_thermalize* t, size_t* bytes)
{
    return snapshot_bytes(t, bytes);
}

int cavmd_snapshot_thermalize_save(cavmd_thermalize* t, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(t, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_thermalize_load(cavmd_thermalize* t, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(t, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"
