// cavmd_batch.hip -- cavmd_batch of include/cavmd.h: the cavity force of a batch of small systems in one launch.
// One of the eleven objects built on an item table (cavmd_item_table.hpp); the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "cavmd.h"
#include "cavmd_batch_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- a batch of independent small systems in one launch (cavmd_batch_kernel.hpp) ------------------------------------------
// The replica loop of the reference (examples/05_advanced_run.py:1570-1612) on one GPU: B systems, one kernel, one
// workgroup per system.  The table of rows lives on the device from create / set_items on; compute enqueues the kernel and
// nothing else.
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
    return create_table(tie_of(ws), n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE,
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
