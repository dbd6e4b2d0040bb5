// cavmd_bussi_batch.hip -- cavmd_bussi_batch of include/cavmd.h: the thermostat step of a batch of small systems in one launch.
// One of the objects built on an item table (cavmd_item_table.hpp), a StateTable; the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cavmd.h"
#include "cavmd_bussi_batch_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- the Bussi thermostat step of a batch of independent small systems in one launch (cavmd_bussi_batch_kernel.hpp) ---------
// A StateTable for its n device states (d_state) and their snapshot; its read and reset are the entry points' own, which go
// through the host blocks the kernel publishes to.
struct cavmd_bussi_batch : StateTable<cavmd_bussi_batch_item, BussiBatchRow, BussiDevice> // launched by n_members descending
{
    std::vector<uint64_t> refused_seen;        // per item: refusals already reported to the caller
    MappedBlock<HostBussiBatch> h_blocks;      // n blocks, indexed by item
    uint64_t sequence = 0;
    bool captured = false; // some step was enqueued into a stream capture: the stamps cannot tell replays apart
    bool loaded = false;   // a snapshot was loaded: the states mean something before the first step

    cavmd_bussi_batch()
        : StateTable(cavmd_bussi_batch_item_check, [](const cavmd_bussi_batch_item& it) { return it.n_members; },
                     uploaded_as_it_is<cavmd_bussi_batch_item, BussiBatchRow>)
    {
    }

    hipError_t alloc_own()
    {
        refused_seen.assign(n, 0);
        const hipError_t e = StateTable::alloc_own();
        return e == hipSuccess ? h_blocks.alloc(n) : e;
    }

    cavmd_snapshot_header snapshot_shape() const
    {
        return state_shape(CAVMD_SNAPSHOT_BUSSI_BATCH, 0, 0);
    }

    // the host's copies follow the loaded states (nothing is in flight: snapshot_load has waited): the blocks that a read
    // outside a capture answers from, and the refusals counted in them, which count as reported
    void snapshot_loaded(const char* const* sections)
    {
        for (size_t i = 0; i < n; ++i)
        {
            memcpy(&h_blocks.host[i].state, sections[0] + i * sizeof(BussiDevice), sizeof(BussiDevice));
            refused_seen[i] = h_blocks.host[i].state.errors;
        }
        loaded = true;
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
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [](cavmd_bussi_batch*) {});
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
    if (b->sequence == 0 && !b->loaded)
        return CAVMD_OK;
    DeviceGuard guard(b->device);
    if (b->captured || b->sequence == 0) // (no step since a load: the loaded states, as the device holds them)
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

int cavmd_snapshot_bussi_batch_bytes(cavmd_bussi_batch* b, size_t* bytes)
{
    return snapshot_bytes(b, bytes);
}

int cavmd_snapshot_bussi_batch_save(cavmd_bussi_batch* b, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(b, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_bussi_batch_load(cavmd_bussi_batch* b, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(b, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"
