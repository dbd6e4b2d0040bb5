// cavmd_batch.hip -- cavmd_batch of include/cavmd.h: the cavity force of a batch of small systems in one launch; and
// cavmd_shared_cavity, the same force with the dipole summed over the systems of a cavity, in two launches.
// One of the eleven objects built on an item table (cavmd_item_table.hpp); the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "cavmd.h"
#include "cavmd_batch_kernel.hpp"
#include "cavmd_item_table.hpp"
#include "cavmd_shared_cavity_kernel.hpp"

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

// ---- several systems of a batch coupled to one shared cavity mode, two launches (cavmd_shared_cavity_kernel.hpp) -----------------
// A LinkedTable (cavmd_item_table.hpp): the tables derived from the items are the cavities and their member lists.  What is
// below is the status of a row, the status of a whole table (the rules that cross rows) and how the device tables follow.
namespace
{
static_assert(sizeof(cavmd_shared_cavity_item) == 128, "shared-cavity item layout");
static_assert(CAVMD_SHARED_CAVITY_MAX_MEMBERS == kSharedCavityMaxMembers, "the header's limit is the kernel's");

int shared_cavity_item_status(const cavmd_shared_cavity_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    // a batch item but for its last 32 bytes: the per-row rules are cavmd_batch_item_check's
    cavmd_batch_item b;
    static_assert(sizeof(b) == sizeof(*it), "the two items differ in their last 32 bytes only");
    memcpy(&b, it, sizeof(b));
    memset(b.reserved, 0, sizeof(b.reserved));
    if (it->reserved0 != 0 || it->reserved[0] != 0 || it->reserved[1] != 0 || it->reserved[2] != 0)
        return CAVMD_ERR_INVALID_VALUE;
    return cavmd_batch_item_check(&b);
}

// Host view of the cavities of a checked table: members[c] = the items of cavity c, ascending.
struct SharedCavityLayout
{
    std::vector<std::vector<unsigned>> members;
    std::vector<unsigned> carrier;
};

// The status of a whole table: every row, then the rules that cross rows.  `out` NULL: the status alone.
int shared_cavity_table_status(size_t n_items, const cavmd_shared_cavity_item* items, SharedCavityLayout* out)
{
    if (!items || n_items == 0 || n_items > CAVMD_BATCH_MAX_ITEMS)
        return CAVMD_ERR_INVALID_VALUE;
    for (size_t i = 0; i < n_items; ++i)
    {
        const int st = shared_cavity_item_status(items + i);
        if (st != CAVMD_OK)
            return st;
    }
    // ids dense in 0 .. n_cavities - 1: none beyond the number of items, none in between without a member
    size_t n_cavities = 0;
    for (size_t i = 0; i < n_items; ++i)
    {
        if (items[i].cavity >= n_items)
            return CAVMD_ERR_INVALID_VALUE;
        n_cavities = std::max(n_cavities, (size_t)items[i].cavity + 1);
    }
    SharedCavityLayout l;
    l.members.resize(n_cavities);
    for (size_t i = 0; i < n_items; ++i)
        l.members[items[i].cavity].push_back((unsigned)i);
    l.carrier.assign(n_cavities, 0u);
    for (size_t c = 0; c < n_cavities; ++c)
        if (l.members[c].empty())
            return CAVMD_ERR_INVALID_VALUE;
    for (size_t c = 0; c < n_cavities; ++c)
        if (l.members[c].size() > CAVMD_SHARED_CAVITY_MAX_MEMBERS)
            return CAVMD_ERR_CAPACITY;
    for (size_t c = 0; c < n_cavities; ++c)
    {
        unsigned carriers = 0;
        for (unsigned i : l.members[c])
            if (items[i].L_typeid >= 0)
            {
                l.carrier[c] = i;
                carriers += 1;
            }
        if (carriers != 1)
            return CAVMD_ERR_INVALID_VALUE;
    }
    for (size_t c = 0; c < n_cavities; ++c)
        for (unsigned i : l.members[c])
            if (memcmp(&items[i].params, &items[l.members[c][0]].params, sizeof(cavmd_params)) != 0)
                return CAVMD_ERR_BAD_PARAMS;
    if (out)
        *out = std::move(l);
    return CAVMD_OK;
}

SharedCavityRow shared_cavity_row(const cavmd_shared_cavity_item& it)
{
    SharedCavityRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.charge = it.d_charge;
    r.image = reinterpret_cast<const int*>(it.d_image);
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx; r.Ly = it.Ly; r.Lz = it.Lz;
    r.N = it.N;
    r.L_typeid = it.L_typeid;
    r.cavity = it.cavity;
    return r;
}

struct SharedCavityNothing // (no table is derived from one item alone)
{
};

// what set_items replaces together
struct SharedCavityTables
{
    DeviceArray<SharedCavity> cavities;
    DeviceArray<unsigned> members;
    SharedCavityHeader header;
    std::vector<unsigned> carrier; // host: item index of each cavity's carrier
};
} // namespace

struct cavmd_shared_cavity final : LinkedTable<cavmd_shared_cavity_item, SharedCavityRow, SharedCavityNothing, SharedCavityTables>
{
    DeviceArray<cavmd_result> d_result;       // n blocks, indexed by item
    DeviceArray<SharedCavityRecord> d_record; // n records, indexed by item: launch 1 writes, launch 2 reads
    DeviceArray<double> d_cell_dipole;        // n x 4
    uint64_t sequence = 0;

    cavmd_shared_cavity() : LinkedTable([](const cavmd_shared_cavity_item& it) { return it.N; }, shared_cavity_row) {}

    int item_status(const cavmd_shared_cavity_item* it, SharedCavityNothing*) const override
    {
        return shared_cavity_item_status(it);
    }

    void strip(cavmd_shared_cavity_item*) const override {}

    // (hides LinkedTable's: a table passes as a whole)
    int check_new(const cavmd_shared_cavity_item* h_items, size_t n_items)
    {
        const int st = LinkedTable::check_new(h_items, n_items);
        return st == CAVMD_OK ? shared_cavity_table_status(n_items, h_items, nullptr) : st;
    }

    hipError_t alloc_own()
    {
        hipError_t e = LinkedTable::alloc_own();
        if (e == hipSuccess)
            e = d_result.alloc_zeroed(n);
        if (e == hipSuccess)
            e = d_record.alloc_zeroed(n);
        return e == hipSuccess ? d_cell_dipole.alloc_zeroed(4 * n) : e;
    }

    // (hides LinkedTable's: the table after substitution passes as a whole, or nothing changes)
    int set_items(size_t first, size_t count, const cavmd_shared_cavity_item* h_items)
    {
        if (!within(first, count, h_items))
            return CAVMD_ERR_INVALID_VALUE;
        std::vector<cavmd_shared_cavity_item> all(items);
        std::copy(h_items, h_items + count, all.begin() + first);
        const int st = shared_cavity_table_status(all.size(), all.data(), nullptr);
        return st == CAVMD_OK ? LinkedTable::set_items(first, count, h_items) : st;
    }

    hipError_t fill(const std::vector<cavmd_shared_cavity_item>& all, const std::vector<unsigned>&, const std::vector<SharedCavityNothing>&,
                    SharedCavityTables* t) const override
    {
        SharedCavityLayout l;
        if (shared_cavity_table_status(all.size(), all.data(), &l) != CAVMD_OK) // (checked before: check_new, set_items)
            return hipErrorInvalidValue;
        std::vector<SharedCavity> cavities(l.members.size());
        std::vector<unsigned> pool;
        for (size_t c = 0; c < l.members.size(); ++c)
        {
            SharedCavity& cav = cavities[c];
            memset(&cav, 0, sizeof(cav));
            const cavmd_params& p = all[l.members[c][0]].params;
            if (params_ok(&p)) // (unchecked only where every member is empty: nothing reads them)
                cav.prm = derive(&p);
            cav.count = (unsigned)l.members[c].size();
            cav.first = pool_append(&pool, l.members[c]);
            cav.carrier = l.carrier[c];
        }
        hipError_t e = t->cavities.upload(cavities.data(), cavities.size());
        if (e == hipSuccess)
            e = t->members.upload(pool.data(), pool.size());
        memset(&t->header, 0, sizeof(t->header));
        t->header.cavities = t->cavities.ptr;
        t->header.members = t->members.ptr;
        t->header.n_cavities = (unsigned)cavities.size();
        t->carrier = l.carrier;
        return e;
    }
};

extern "C"
{

int cavmd_shared_cavity_item_check(const cavmd_shared_cavity_item* it)
{
    return shared_cavity_item_status(it);
}

int cavmd_shared_cavity_table_check(size_t n_items, const cavmd_shared_cavity_item* h_items, uint32_t* n_cavities)
{
    SharedCavityLayout l;
    const int st = shared_cavity_table_status(n_items, h_items, &l);
    if (st == CAVMD_OK && n_cavities)
        *n_cavities = (uint32_t)l.members.size();
    return st;
}

int cavmd_shared_cavity_create(cavmd_workspace* ws, size_t n_items, const cavmd_shared_cavity_item* h_items, cavmd_shared_cavity** out)
{
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [](cavmd_shared_cavity*) {});
}

int cavmd_shared_cavity_destroy(cavmd_shared_cavity* c)
{
    return destroy_table(c);
}

int cavmd_shared_cavity_set_items(cavmd_shared_cavity* c, size_t first, size_t count, const cavmd_shared_cavity_item* h_items)
{
    return c ? c->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_shared_cavity_compute(cavmd_shared_cavity* c, void* stream_)
{
    if (!c)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    int st = c->launch(stream, shared_cavity_dipole_kernel<kSharedCavityBlock>, dim3((unsigned)c->n), dim3(kSharedCavityBlock), 0,
                       c->d_rows.ptr, c->d_order.ptr, c->d_record.ptr, c->d_cell_dipole.ptr);
    if (st != CAVMD_OK)
        return st;
    // the kernel boundary on the stream orders launch 1 before launch 2: the only synchronisation between workgroups
    st = c->launch(stream, shared_cavity_force_kernel<kSharedCavityBlock>, dim3((unsigned)c->n), dim3(kSharedCavityBlock), 0,
                   c->d_rows.ptr, c->d_order.ptr, c->d_header.ptr, c->d_record.ptr, c->sequence + 1, c->d_result.ptr);
    if (st == CAVMD_OK)
        c->sequence += 1;
    return st;
}

int cavmd_shared_cavity_last_sequence(cavmd_shared_cavity* c, uint64_t* out)
{
    if (!c || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = c->sequence;
    return CAVMD_OK;
}

int cavmd_shared_cavity_results_read(cavmd_shared_cavity* c, void* stream_, cavmd_result* out)
{
    if (!c || !out)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(c->device);
    const int st = sync_uncaptured((hipStream_t)stream_);
    if (st != CAVMD_OK)
        return st;
    if (c->sequence == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    CAVMD_HIP_TRY(hipMemcpy(out, c->d_result.ptr, sizeof(cavmd_result) * c->n, hipMemcpyDeviceToHost));
    return CAVMD_OK;
}

int cavmd_shared_cavity_results_device_ptr(cavmd_shared_cavity* c, const cavmd_result** out)
{
    if (!c || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = c->d_result.ptr;
    return CAVMD_OK;
}

int cavmd_shared_cavity_cell_dipoles_device_ptr(cavmd_shared_cavity* c, const double** out)
{
    if (!c || !out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = c->d_cell_dipole.ptr;
    return CAVMD_OK;
}

int cavmd_shared_cavity_count(cavmd_shared_cavity* c, uint32_t* n_cavities)
{
    if (!c || !n_cavities)
        return CAVMD_ERR_INVALID_VALUE;
    *n_cavities = (uint32_t)c->tables.carrier.size();
    return CAVMD_OK;
}

int cavmd_shared_cavity_carrier(cavmd_shared_cavity* c, uint32_t cavity, uint32_t* item)
{
    if (!c || !item || cavity >= c->tables.carrier.size())
        return CAVMD_ERR_INVALID_VALUE;
    *item = c->tables.carrier[cavity];
    return CAVMD_OK;
}

} // extern "C"
