// cavmd_verlet.hip -- cavmd_verlet of include/cavmd.h: the velocity-Verlet half-steps of a batch of small systems, one launch each.
// One of the seven objects built on an item table (cavmd_item_table.hpp); the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "cavmd.h"
#include "cavmd_verlet_batch_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

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
