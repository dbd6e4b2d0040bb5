// cavmd_recorder.hip -- cavmd_recorder of include/cavmd.h: per-step observables of a batch appended to a series in device memory;
// cavmd_ledger, the energy ledger, which has the recorder's shape and calls its kinetic-energy code; and cavmd_trajectory, whose
// records are frames of positions, velocities and images (three objects in one unit, as cavmd_verlet.hip holds four).  Three of
// the twelve objects built on an item table (cavmd_item_table.hpp), each a SeriesTable; what the first two share beyond that is
// PeriodicSeries, below.  The workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "cavmd.h"
#include "cavmd_recorder_kernel.hpp"
#include "cavmd_ledger_kernel.hpp"
#include "cavmd_trajectory_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

namespace
{
// The shape the recorder and the ledger share: items with N particles and n_members group members, uploaded as they are and
// launched by max(N, n_members) descending; kRecCounters words per item (rows, calls, phase, slot); on every period-th call
// an item appends one Record, whose temperatures are taken with kB.
template <class Item, class Row, class Record>
struct PeriodicSeries : SeriesTable<Item, Row, Record>
{
    uint64_t period = 1;
    double kB = 0.0;

    explicit PeriodicSeries(int (*check_)(const Item*))
        : SeriesTable<Item, Row, Record>(
              kRecCounters, check_, [](const Item& it) { return std::max(it.N, it.n_members); }, uploaded_as_it_is<Item, Row>)
    {
    }

    int capacity_status(size_t n_items) const
    {
        return this->capacity > kRecorderMaxBytes / sizeof(Record) / n_items ? CAVMD_ERR_CAPACITY : CAVMD_OK;
    }
    hipError_t alloc_own()
    {
        return this->alloc_series();
    }

    // one launch of n workgroups of the object's kernel
    template <class Kernel>
    int record(void* stream, Kernel kernel)
    {
        return this->launch((hipStream_t)stream, kernel, dim3((unsigned)this->n), dim3(256), 0, this->d_rows.ptr,
                            this->d_order.ptr, (unsigned)this->n, (uint64_t)this->capacity, period, kB, this->d_series.ptr,
                            this->d_counters.ptr);
    }
};

template <class Table, class Item>
int create_periodic(cavmd_workspace* ws, size_t n_items, const Item* h_items, size_t capacity, uint64_t period, double kB,
                    Table** out)
{
    const bool args_ok = capacity != 0 && period != 0 && kB > 0.0 && std::isfinite(kB);
    return create_table(tie_of(ws), n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE, [&](Table* t) {
        t->capacity = capacity;
        t->period = period;
        t->kB = kB;
    });
}
} // namespace

// ---- per-step observables of a batch recorded into a time series in device memory (cavmd_recorder_kernel.hpp) ----------------
struct cavmd_recorder : PeriodicSeries<cavmd_recorder_item, RecorderRow, cavmd_record>
{
    cavmd_recorder() : PeriodicSeries(cavmd_recorder_item_check) {}

    cavmd_snapshot_header snapshot_shape() const
    {
        return series_shape(CAVMD_SNAPSHOT_RECORDER, 0, 0);
    }
};

namespace
{
static_assert(sizeof(cavmd_record) == 128 && offsetof(cavmd_record, energy) == 16 && offsetof(cavmd_record, cavity_kinetic) == 88,
              "record layout");
static_assert(sizeof(cavmd_recorder_item) == sizeof(RecorderRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_recorder_item, d_result) == offsetof(RecorderRow, res)
                  && offsetof(cavmd_recorder_item, d_vel) == offsetof(RecorderRow, vel2)
                  && offsetof(cavmd_recorder_item, d_net_force) == offsetof(RecorderRow, force2)
                  && offsetof(cavmd_recorder_item, d_members) == offsetof(RecorderRow, members)
                  && offsetof(cavmd_recorder_item, N) == offsetof(RecorderRow, N)
                  && offsetof(cavmd_recorder_item, n_members) == offsetof(RecorderRow, n_members),
              "recorder item layout");
static_assert(CAVMD_BATCH_MAX_ITEM_N <= kRecorderMaxTiles * 256 * kRecorderUnroll, "one LDS partial per tile");
static_assert(kRecRows == 0, "SeriesTable: the rows-written array is the first of the counters");
} // namespace

extern "C"
{

int cavmd_recorder_item_check(const cavmd_recorder_item* it)
{
    if (!it || !it->d_result)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 3; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_result & 15) || ((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_net_force & 15)
        || ((uintptr_t)it->d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N || it->n_members > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_recorder_item* h_items, size_t capacity,
                          uint64_t period, double kB, cavmd_recorder** out)
{
    return create_periodic(ws, n_items, h_items, capacity, period, kB, out);
}

int cavmd_recorder_destroy(cavmd_recorder* r)
{
    return destroy_table(r);
}

int cavmd_recorder_set_items(cavmd_recorder* r, size_t first, size_t count, const cavmd_recorder_item* h_items)
{
    return r ? r->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_record(cavmd_recorder* r, void* stream_)
{
    return r ? r->record(stream_, recorder_batch_kernel<256>) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_rows(cavmd_recorder* r, void* stream_, uint64_t* out)
{
    return (r && out) ? r->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_read(cavmd_recorder* r, void* stream_, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows,
                        cavmd_record* out)
{
    return r ? r->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_reset(cavmd_recorder* r, void* stream_)
{
    return r ? r->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_recorder_device_ptr(cavmd_recorder* r, const cavmd_record** records, const uint64_t** rows)
{
    return r ? r->device_ptr(records, rows) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_recorder_bytes(cavmd_recorder* r, size_t* bytes)
{
    return snapshot_bytes(r, bytes);
}

int cavmd_snapshot_recorder_save(cavmd_recorder* r, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(r, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_recorder_load(cavmd_recorder* r, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(r, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"

// ---- the energy ledger of a batch: every term of the conserved energy per step (cavmd_ledger_kernel.hpp) ----------------------
struct cavmd_ledger : PeriodicSeries<cavmd_ledger_item, LedgerItem, cavmd_ledger_row> // the recorder's shape
{
    using Base = PeriodicSeries<cavmd_ledger_item, LedgerItem, cavmd_ledger_row>;
    // the run clock's time rule (cavmd_runclock_ledger_set_rule); time_interval 0: off
    double time_interval = 0.0, max_time = 0.0;
    DeviceArray<double> d_last_time; // n words beside the counters, zero from the first rule on; written under the rule alone

    cavmd_ledger() : PeriodicSeries(cavmd_ledger_item_check) {}

    // a blob taken under the rule says so in word 0 and carries last_time behind the ring
    cavmd_snapshot_header snapshot_shape() const
    {
        return series_shape(CAVMD_SNAPSHOT_LEDGER, time_interval > 0.0 ? 1 : 0, 0);
    }
    size_t snapshot_arrays(const void** arrays) const
    {
        const size_t count = Base::snapshot_arrays(arrays);
        if (time_interval == 0.0)
            return count;
        arrays[count] = d_last_time.ptr;
        return count + 1;
    }

    // (hides ItemTable's: under the rule an item needs its clock)
    int set_items(size_t first, size_t count, const cavmd_ledger_item* h_items)
    {
        if (time_interval > 0.0 && within(first, count, h_items))
            for (size_t i = 0; i < count; ++i)
                if (!h_items[i].d_time)
                    return CAVMD_ERR_INVALID_VALUE;
        return Base::set_items(first, count, h_items);
    }

    int reset(hipStream_t stream)
    {
        const int st = Base::reset(stream);
        if (st != CAVMD_OK || !d_last_time.ptr)
            return st;
        DeviceGuard guard(device);
        CAVMD_HIP_TRY(hipMemsetAsync(d_last_time.ptr, 0, sizeof(double) * n, stream));
        return CAVMD_OK;
    }
};

namespace
{
static_assert(sizeof(cavmd_ledger_row) == 192 && offsetof(cavmd_ledger_row, potential) == 24
                  && offsetof(cavmd_ledger_row, reservoir) == 128 && offsetof(cavmd_ledger_row, reserved) == 184,
              "ledger row layout");
static_assert(sizeof(cavmd_ledger_item) == sizeof(LedgerItem), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_ledger_item, d_result) == offsetof(LedgerItem, res)
                  && offsetof(cavmd_ledger_item, d_vel) == offsetof(LedgerItem, vel2)
                  && offsetof(cavmd_ledger_item, d_members) == offsetof(LedgerItem, members)
                  && offsetof(cavmd_ledger_item, n_members) == offsetof(LedgerItem, n_members)
                  && offsetof(cavmd_ledger_item, N) == offsetof(LedgerItem, N)
                  && offsetof(cavmd_ledger_item, d_energy) == offsetof(LedgerItem, energy)
                  && offsetof(cavmd_ledger_item, d_reservoir) == offsetof(LedgerItem, reservoir)
                  && offsetof(cavmd_ledger_item, d_time) == offsetof(LedgerItem, time)
                  && offsetof(cavmd_ledger_item, dof) == offsetof(LedgerItem, dof)
                  && offsetof(cavmd_ledger_item, add_cavity_kinetic) == offsetof(LedgerItem, add_cavity_kinetic),
              "ledger item layout");
static_assert(sizeof(((cavmd_ledger_item*)0)->d_energy) == sizeof(void*) * kLedgerTerms
                  && sizeof(((cavmd_ledger_item*)0)->d_reservoir) == sizeof(void*) * kLedgerReservoirs,
              "four terms, four reservoirs");
} // namespace

extern "C"
{

int cavmd_ledger_item_check(const cavmd_ledger_item* it)
{
    if (!it || it->reserved0 != 0 || it->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_result & 15) || ((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_members & 3)
        || ((uintptr_t)it->d_time & 7))
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < kLedgerTerms; ++k)
        if (((uintptr_t)it->d_energy[k] & 15) || (k > 0 && it->d_energy[k] && !it->d_energy[k - 1]))
            return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < kLedgerReservoirs; ++k)
        if (((uintptr_t)it->d_reservoir[k] & 7) || (k > 0 && it->d_reservoir[k] && !it->d_reservoir[k - 1]))
            return CAVMD_ERR_INVALID_VALUE;
    if (!finite_nonnegative(it->dof) || it->add_cavity_kinetic > 1)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N || it->n_members > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_ledger_create(cavmd_workspace* ws, size_t n_items, const cavmd_ledger_item* h_items, size_t capacity, uint64_t period,
                        double kB, cavmd_ledger** out)
{
    return create_periodic(ws, n_items, h_items, capacity, period, kB, out);
}

int cavmd_ledger_destroy(cavmd_ledger* l)
{
    return destroy_table(l);
}

int cavmd_ledger_set_items(cavmd_ledger* l, size_t first, size_t count, const cavmd_ledger_item* h_items)
{
    return l ? l->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_ledger_record(cavmd_ledger* l, void* stream_)
{
    if (!l)
        return CAVMD_ERR_INVALID_VALUE;
    if (l->time_interval > 0.0) // the variant and the rule's values are launch arguments: frozen in a captured launch
        return l->launch((hipStream_t)stream_, ledger_batch_kernel<256, true>, dim3((unsigned)l->n), dim3(256), 0, l->d_rows.ptr,
                         l->d_order.ptr, (unsigned)l->n, (uint64_t)l->capacity, l->kB, l->d_series.ptr, l->d_counters.ptr,
                         l->time_interval, l->max_time, l->d_last_time.ptr);
    return l->record(stream_, ledger_batch_kernel<256>);
}

// the run clock of cavmd_ledger (include/cavmd.h, "the run clock")
int cavmd_runclock_ledger_set_rule(cavmd_ledger* l, double time_interval, double max_time)
{
    if (!l || !finite_nonnegative(time_interval) || !finite_nonnegative(max_time) || (time_interval == 0.0 && max_time != 0.0))
        return CAVMD_ERR_INVALID_VALUE;
    if (time_interval > 0.0)
    {
        if (l->period != 1)
            return CAVMD_ERR_INVALID_VALUE;
        for (const cavmd_ledger_item& it : l->items)
            if (!it.d_time)
                return CAVMD_ERR_INVALID_VALUE;
    }
    DeviceGuard guard(l->device);
    const int st = l->wait_idle(); // as set_items: refused while the last stream is being captured
    if (st != CAVMD_OK)
        return st;
    if (time_interval > 0.0 && !l->d_last_time.ptr)
    {
        const std::vector<double> zero(l->n, 0.0);
        CAVMD_HIP_TRY(l->d_last_time.upload(zero.data(), l->n)); // a copy that has returned: no stream launches ahead of it
    }
    l->time_interval = time_interval + 0.0;
    l->max_time = max_time + 0.0;
    return CAVMD_OK;
}

int cavmd_ledger_rows(cavmd_ledger* l, void* stream_, uint64_t* out)
{
    return (l && out) ? l->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_ledger_read(cavmd_ledger* l, void* stream_, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows,
                      cavmd_ledger_row* out)
{
    return l ? l->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_ledger_reset(cavmd_ledger* l, void* stream_)
{
    return l ? l->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_ledger_device_ptr(cavmd_ledger* l, const cavmd_ledger_row** series, const uint64_t** rows)
{
    return l ? l->device_ptr(series, rows) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_ledger_bytes(cavmd_ledger* l, size_t* bytes)
{
    return snapshot_bytes(l, bytes);
}

int cavmd_snapshot_ledger_save(cavmd_ledger* l, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(l, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_ledger_load(cavmd_ledger* l, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(l, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"

// ---- trajectory frames of a batch: positions, velocities and images per due call (cavmd_trajectory_kernel.hpp) ----------------
struct cavmd_trajectory : SeriesTable<cavmd_trajectory_item, TrajectoryRow, unsigned char> // a record is a frame of layout.frame_bytes
{
    using Base = SeriesTable<cavmd_trajectory_item, TrajectoryRow, unsigned char>;
    struct cavmd_trajectory_layout layout = {};
    uint64_t period = 1;
    double time_interval = 0.0;

    cavmd_trajectory()
        : Base(kTrajCounters, cavmd_trajectory_item_check, [](const cavmd_trajectory_item& it) { return (unsigned)it.N; },
               uploaded_as_it_is<cavmd_trajectory_item, TrajectoryRow>)
    {
    }

    // what the object asks of an item beyond cavmd_trajectory_item_check
    int check_own(const cavmd_trajectory_item* h_items, size_t count) const
    {
        const int st = check_items(h_items, count, check);
        if (st != CAVMD_OK)
            return st;
        for (size_t i = 0; i < count; ++i)
            if (h_items[i].N > layout.max_N)
                return CAVMD_ERR_CAPACITY;
        for (size_t i = 0; i < count; ++i)
            if (time_interval > 0.0 && !h_items[i].d_time)
                return CAVMD_ERR_INVALID_VALUE;
        return CAVMD_OK;
    }

    // create_table's hooks
    int check_new(const cavmd_trajectory_item* h_items, size_t n_items)
    {
        return check_own(h_items, n_items);
    }
    int capacity_status(size_t n_items) const
    {
        return capacity > CAVMD_TRAJECTORY_MAX_BYTES / layout.frame_bytes / n_items ? CAVMD_ERR_CAPACITY : CAVMD_OK;
    }

    cavmd_snapshot_header snapshot_shape() const
    {
        return series_shape(CAVMD_SNAPSHOT_TRAJECTORY, layout.max_N, layout.format);
    }
    hipError_t alloc_own()
    {
        record_bytes = (size_t)layout.frame_bytes;
        return alloc_series();
    }

    // (hides ItemTable's: an item is also held against the object's max_N and rule)
    int set_items(size_t first, size_t count, const cavmd_trajectory_item* h_items)
    {
        if (!within(first, count, h_items))
            return CAVMD_ERR_INVALID_VALUE;
        const int st = check_own(h_items, count);
        return st == CAVMD_OK ? Base::set_items(first, count, h_items) : st;
    }

    template <class Kernel>
    int record(void* stream, Kernel kernel, const uint32_t* d_take_frame)
    {
        const TrajectoryFrame frame {layout.frame_bytes, layout.velocity_offset, layout.image_offset};
        return launch((hipStream_t)stream, kernel, dim3((unsigned)n), dim3(256), 0, d_rows.ptr, d_order.ptr, (unsigned)n,
                      (uint64_t)capacity, period, time_interval, frame, d_take_frame, d_series.ptr, d_counters.ptr);
    }
};

namespace
{
static_assert(sizeof(cavmd_trajectory_item) == sizeof(TrajectoryRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_trajectory_item, d_pos) == offsetof(TrajectoryRow, pos2)
                  && offsetof(cavmd_trajectory_item, d_image) == offsetof(TrajectoryRow, image)
                  && offsetof(cavmd_trajectory_item, d_vel) == offsetof(TrajectoryRow, vel2)
                  && offsetof(cavmd_trajectory_item, d_time) == offsetof(TrajectoryRow, time)
                  && offsetof(cavmd_trajectory_item, Lx) == offsetof(TrajectoryRow, L)
                  && offsetof(cavmd_trajectory_item, N) == offsetof(TrajectoryRow, N),
              "trajectory item layout");
static_assert(sizeof(cavmd_trajectory_header) == sizeof(TrajectoryHeader) && sizeof(cavmd_trajectory_header) == kTrajHeaderBytes
                  && offsetof(cavmd_trajectory_header, call) == offsetof(TrajectoryHeader, call)
                  && offsetof(cavmd_trajectory_header, row) == offsetof(TrajectoryHeader, row)
                  && offsetof(cavmd_trajectory_header, time) == offsetof(TrajectoryHeader, time)
                  && offsetof(cavmd_trajectory_header, N) == offsetof(TrajectoryHeader, N)
                  && offsetof(cavmd_trajectory_header, flags) == offsetof(TrajectoryHeader, flags)
                  && offsetof(cavmd_trajectory_header, box) == offsetof(TrajectoryHeader, box)
                  && offsetof(cavmd_trajectory_header, reserved) == offsetof(TrajectoryHeader, reserved),
              "trajectory header layout");
static_assert(sizeof(struct cavmd_trajectory_layout) == 48, "trajectory layout");
static_assert(kTrajRows == 0, "SeriesTable: the rows-written array is the first of the counters");

inline uint64_t pad16(uint64_t x)
{
    return (x + 15u) & ~(uint64_t)15u;
}
} // namespace

extern "C"
{

int cavmd_trajectory_item_check(const cavmd_trajectory_item* it)
{
    if (!it || it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_vel & 15) || ((uintptr_t)it->d_image & 3) || ((uintptr_t)it->d_time & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > 0)
    {
        double cut_sq;
        if (!it->d_pos || !it->d_image || !box_ok(it->Lx, it->Ly, it->Lz, &cut_sq))
            return CAVMD_ERR_INVALID_VALUE;
    }
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_trajectory_layout(uint32_t max_N, uint32_t format, struct cavmd_trajectory_layout* out)
{
    if (!out || max_N < 1 || max_N > CAVMD_BATCH_MAX_ITEM_N || (format != CAVMD_TRAJECTORY_F64 && format != CAVMD_TRAJECTORY_F32))
        return CAVMD_ERR_INVALID_VALUE;
    const uint32_t e = format == CAVMD_TRAJECTORY_F64 ? 8 : 4;
    const uint64_t section = pad16((uint64_t)3 * max_N * e);
    out->position_offset = kTrajHeaderBytes;
    out->velocity_offset = out->position_offset + section;
    out->image_offset = out->velocity_offset + section;
    out->frame_bytes = out->image_offset + pad16((uint64_t)12 * max_N);
    out->max_N = max_N;
    out->format = format;
    out->element_bytes = e;
    out->reserved = 0;
    return CAVMD_OK;
}

int cavmd_trajectory_create(cavmd_workspace* ws, size_t n_items, const cavmd_trajectory_item* h_items, uint32_t max_N,
                            uint32_t format, size_t capacity, uint64_t period, double time_interval, cavmd_trajectory** out)
{
    struct cavmd_trajectory_layout layout;
    const bool args_ok = cavmd_trajectory_layout(max_N, format, &layout) == CAVMD_OK && capacity != 0 && period != 0
                         && finite_nonnegative(time_interval) && !(time_interval > 0.0 && period != 1);
    return create_table(tie_of(ws), n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE, [&](cavmd_trajectory* t) {
        t->layout = layout;
        t->capacity = capacity;
        t->period = period;
        t->time_interval = time_interval;
    });
}

int cavmd_trajectory_destroy(cavmd_trajectory* t)
{
    return destroy_table(t);
}

int cavmd_trajectory_set_items(cavmd_trajectory* t, size_t first, size_t count, const cavmd_trajectory_item* h_items)
{
    return t ? t->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_trajectory_record(cavmd_trajectory* t, void* stream_, const uint32_t* d_take_frame)
{
    if (!t || ((uintptr_t)d_take_frame & 3))
        return CAVMD_ERR_INVALID_VALUE;
    return t->layout.format == CAVMD_TRAJECTORY_F64
               ? t->record(stream_, trajectory_batch_kernel<256, CAVMD_TRAJECTORY_F64>, d_take_frame)
               : t->record(stream_, trajectory_batch_kernel<256, CAVMD_TRAJECTORY_F32>, d_take_frame);
}

int cavmd_trajectory_rows(cavmd_trajectory* t, void* stream_, uint64_t* out)
{
    return (t && out) ? t->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_trajectory_read(cavmd_trajectory* t, void* stream_, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows,
                          void* out)
{
    return t ? t->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, (unsigned char*)out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_trajectory_reset(cavmd_trajectory* t, void* stream_)
{
    return t ? t->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_trajectory_device_ptr(cavmd_trajectory* t, const void** series, const uint64_t** rows)
{
    if (!t || (!series && !rows))
        return CAVMD_ERR_INVALID_VALUE;
    const unsigned char* p = nullptr;
    const int st = t->device_ptr(series ? &p : nullptr, rows);
    if (st == CAVMD_OK && series)
        *series = p;
    return st;
}

int cavmd_snapshot_trajectory_bytes(cavmd_trajectory* t, size_t* bytes)
{
    return snapshot_bytes(t, bytes);
}

int cavmd_snapshot_trajectory_save(cavmd_trajectory* t, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(t, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_trajectory_load(cavmd_trajectory* t, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(t, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"
