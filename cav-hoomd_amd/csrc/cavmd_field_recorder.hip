// cavmd_field_recorder.hip -- cavmd_field_recorder of include/cavmd.h: density field and F(k,t) of a batch appended to a series
// in device memory.  One of the eleven objects built on an item table (cavmd_item_table.hpp), a SeriesTable; the workspace is an
// incomplete type here.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "cavmd.h"
#include "cavmd_field_recorder_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- density field and F(k,t) of a batch recorded into a time series in device memory (cavmd_field_recorder_kernel.hpp) -------
// launched by N descending; kFldCounters words per item
struct cavmd_field_recorder : SeriesTable<cavmd_field_item, FieldRow, cavmd_field_record>
{
    size_t n_k = 0;
    uint64_t period = 1;
    unsigned max_refs = 1;
    uint64_t interval = 0;
    const double* h_kvec = nullptr;   // the caller's wavevectors: read by create only
    DeviceArray<double> d_kvec;       // n_k x 3
    DeviceArray<uint64_t> d_ref_rows; // n x max_refs: the row each reference was taken at
    DeviceArray<double> d_now;        // n x n_k x 2: the field of the last recorded call
    DeviceArray<double> d_refs;       // n x max_refs x n_k x 2
    // the run clock's time rule (cavmd_runclock_field_set_rule); time_interval 0: off.  The values the kernel reads are in d_rule.
    double time_interval = 0.0;
    DeviceArray<double> d_rule;       // a FieldRule, then last_time (n) and last_reference_time (n): beside the counters, the
                                      // time words zero from the first rule on
    double* times() const { return d_rule.ptr + sizeof(FieldRule) / sizeof(double); }

    cavmd_field_recorder()
        : SeriesTable(kFldCounters, cavmd_field_recorder_item_check, [](const cavmd_field_item& it) { return it.N; },
                      uploaded_as_it_is<cavmd_field_item, FieldRow>)
    {
    }

    // series + fields (the current one and the references) within the recorder's cap
    int capacity_status(size_t n_items) const
    {
        const size_t fields = sizeof(double) * 2 * n_k * ((size_t)max_refs + 1) * n_items;
        return fields > kRecorderMaxBytes || capacity > (kRecorderMaxBytes - fields) / sizeof(cavmd_field_record) / n_items
                   ? CAVMD_ERR_CAPACITY
                   : CAVMD_OK;
    }
    hipError_t alloc_own()
    {
        hipError_t e = d_kvec.upload(h_kvec, 3 * n_k);
        h_kvec = nullptr;
        if (e == hipSuccess)
            e = alloc_series();
        if (e == hipSuccess)
            e = d_ref_rows.alloc_zeroed(n * max_refs);
        if (e == hipSuccess)
            e = d_now.alloc_zeroed(2 * n_k * n);
        return e == hipSuccess ? d_refs.alloc_zeroed(2 * n_k * n * max_refs) : e;
    }

    // the series' two arrays, then what the object keeps beyond them (the wavevectors are create's, not state)
    cavmd_snapshot_header snapshot_shape() const
    {
        // a blob taken under the rule says so above the reference count and carries the two time arrays as a sixth section
        return series_shape(CAVMD_SNAPSHOT_FIELD_RECORDER, (uint32_t)n_k,
                            max_refs | (time_interval > 0.0 ? cavmd::kSnapshotFieldTimed : 0u));
    }
    size_t snapshot_arrays(const void** arrays) const
    {
        const size_t first = SeriesTable::snapshot_arrays(arrays);
        arrays[first] = d_ref_rows.ptr;
        arrays[first + 1] = d_now.ptr;
        arrays[first + 2] = d_refs.ptr;
        if (time_interval == 0.0)
            return first + 3;
        arrays[first + 3] = times();
        return first + 4;
    }

    int reset(hipStream_t stream)
    {
        const int st = SeriesTable::reset(stream);
        if (st != CAVMD_OK || !d_rule.ptr)
            return st;
        DeviceGuard guard(device);
        CAVMD_HIP_TRY(hipMemsetAsync(times(), 0, sizeof(double) * 2 * n, stream));
        return CAVMD_OK;
    }
};

namespace
{
static_assert(sizeof(cavmd_field_record) == 160 && offsetof(cavmd_field_record, n_references) == 8
                  && offsetof(cavmd_field_record, took_reference) == 12 && offsetof(cavmd_field_record, rho2) == 16
                  && offsetof(cavmd_field_record, F) == 32,
              "field record layout");
static_assert(sizeof(cavmd_field_item) == sizeof(FieldRow), "the item table is uploaded as it is");
static_assert(offsetof(cavmd_field_item, d_position) == offsetof(FieldRow, pos)
                  && offsetof(cavmd_field_item, position_stride) == offsetof(FieldRow, stride)
                  && offsetof(cavmd_field_item, N) == offsetof(FieldRow, N),
              "field item layout");
static_assert(kFldRows == 0, "SeriesTable: the rows-written array is the first of the counters");
} // namespace

extern "C"
{

int cavmd_field_recorder_item_check(const cavmd_field_item* it)
{
    if (!it || it->reserved0 != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (int k = 0; k < 5; ++k)
        if (it->reserved[k] != 0)
            return CAVMD_ERR_INVALID_VALUE;
    if ((!it->d_position && it->N > 0) || ((uintptr_t)it->d_position & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->position_stride < 24 || (it->position_stride & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_BATCH_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    return CAVMD_OK;
}

int cavmd_field_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_field_item* h_items, size_t n_k,
                                const double* h_wavevectors, size_t capacity, uint64_t period, uint32_t max_references,
                                uint64_t reference_interval, cavmd_field_recorder** out)
{
    bool args_ok = h_wavevectors && n_k != 0 && n_k <= CAVMD_FIELD_MAX_WAVEVECTORS && capacity != 0 && period != 0
        && max_references != 0 && max_references <= CAVMD_FIELD_MAX_REFERENCES;
    for (size_t i = 0; args_ok && i < 3 * n_k; ++i)
        args_ok = std::isfinite(h_wavevectors[i]);
    return create_table(tie_of(ws), n_items, h_items, out, args_ok ? CAVMD_OK : CAVMD_ERR_INVALID_VALUE,
                        [&](cavmd_field_recorder* r) {
                            r->n_k = n_k;
                            r->h_kvec = h_wavevectors;
                            r->capacity = capacity;
                            r->period = period;
                            r->max_refs = max_references;
                            r->interval = reference_interval;
                        });
}

int cavmd_field_recorder_destroy(cavmd_field_recorder* r)
{
    return destroy_table(r);
}

int cavmd_field_recorder_set_items(cavmd_field_recorder* r, size_t first, size_t count, const cavmd_field_item* h_items)
{
    return r ? r->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_record(cavmd_field_recorder* r, void* stream_, const uint32_t* d_take_reference)
{
    if (!r || ((uintptr_t)d_take_reference & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (r->time_interval > 0.0) // the variant and the rule's values are launch arguments: frozen in a captured launch
        return r->launch((hipStream_t)stream_, field_recorder_batch_kernel<256, true>, dim3((unsigned)r->n), dim3(256), 0,
                         r->d_rows.ptr, r->d_order.ptr, (unsigned)r->n, r->d_kvec.ptr, (unsigned)r->n_k, make_sincos_coef(),
                         (uint64_t)r->capacity, r->max_refs, r->interval, d_take_reference, r->d_series.ptr, r->d_counters.ptr,
                         r->d_ref_rows.ptr, r->d_now.ptr, r->d_refs.ptr, reinterpret_cast<FieldRule*>(r->d_rule.ptr));
    return r->launch((hipStream_t)stream_, field_recorder_batch_kernel<256>, dim3((unsigned)r->n), dim3(256), 0, r->d_rows.ptr,
                     r->d_order.ptr, (unsigned)r->n, r->d_kvec.ptr, (unsigned)r->n_k, make_sincos_coef(), (uint64_t)r->capacity,
                     r->period, r->max_refs, r->interval, d_take_reference, r->d_series.ptr, r->d_counters.ptr, r->d_ref_rows.ptr,
                     r->d_now.ptr, r->d_refs.ptr);
}

// the run clock of cavmd_field_recorder (include/cavmd.h, "the run clock")
int cavmd_runclock_field_set_rule(cavmd_field_recorder* r, const double* d_time0, uint64_t stride_bytes, double time_interval,
                                  double reference_time_interval)
{
    if (!r || !finite_nonnegative(time_interval) || !finite_nonnegative(reference_time_interval)
        || (time_interval == 0.0 && reference_time_interval != 0.0))
        return CAVMD_ERR_INVALID_VALUE;
    if (time_interval > 0.0
        && (!d_time0 || ((uintptr_t)d_time0 & 7) || stride_bytes < 8 || (stride_bytes & 7) || r->period != 1))
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(r->device);
    const int st = r->wait_idle(); // as set_items: refused while the last stream is being captured
    if (st != CAVMD_OK)
        return st;
    if (time_interval > 0.0)
    {
        const FieldRule rule {reinterpret_cast<const char*>(d_time0), stride_bytes, time_interval + 0.0, reference_time_interval + 0.0};
        if (!r->d_rule.ptr)
        {
            std::vector<double> block(sizeof(rule) / sizeof(double) + 2 * r->n, 0.0);
            memcpy(block.data(), &rule, sizeof(rule));
            CAVMD_HIP_TRY(r->d_rule.upload(block.data(), block.size())); // a copy that has returned: no stream launches ahead of it
        }
        else
            CAVMD_HIP_TRY(hipMemcpy(r->d_rule.ptr, &rule, sizeof(rule), hipMemcpyHostToDevice));
    }
    r->time_interval = time_interval + 0.0;
    return CAVMD_OK;
}

int cavmd_field_recorder_rows(cavmd_field_recorder* r, void* stream_, uint64_t* out)
{
    return (r && out) ? r->rows((hipStream_t)stream_, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_read(cavmd_field_recorder* r, void* stream_, size_t first_item, size_t n_items, uint64_t first_row,
                              size_t n_rows, cavmd_field_record* out)
{
    return r ? r->read((hipStream_t)stream_, first_item, n_items, first_row, n_rows, out) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_read_fields(cavmd_field_recorder* r, void* stream_, size_t item, double* rho_now, double* rho_refs,
                                     uint64_t* ref_rows, uint32_t* n_refs)
{
    if (!r || !n_refs || item >= r->n)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(r->device);
    const int st = sync_uncaptured((hipStream_t)stream_);
    if (st != CAVMD_OK)
        return st;
    uint64_t rows = 0, refs = 0;
    CAVMD_HIP_TRY(hipMemcpy(&rows, r->d_counters.ptr + (size_t)kFldRows * r->n + item, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rows == 0)
        return CAVMD_ERR_NOT_COMPUTED;
    CAVMD_HIP_TRY(hipMemcpy(&refs, r->d_counters.ptr + (size_t)kFldRefs * r->n + item, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (refs > r->max_refs)
        return CAVMD_ERR_INVALID_VALUE;
    const size_t field_len = 2 * r->n_k;
    if (rho_now)
        CAVMD_HIP_TRY(hipMemcpy(rho_now, r->d_now.ptr + item * field_len, sizeof(double) * field_len, hipMemcpyDeviceToHost));
    if (rho_refs && refs)
        CAVMD_HIP_TRY(hipMemcpy(rho_refs, r->d_refs.ptr + item * r->max_refs * field_len, sizeof(double) * field_len * refs,
                                hipMemcpyDeviceToHost));
    if (ref_rows && refs)
        CAVMD_HIP_TRY(hipMemcpy(ref_rows, r->d_ref_rows.ptr + item * r->max_refs, sizeof(uint64_t) * refs, hipMemcpyDeviceToHost));
    *n_refs = (uint32_t)refs;
    return CAVMD_OK;
}

int cavmd_field_recorder_reset(cavmd_field_recorder* r, void* stream_)
{
    return r ? r->reset((hipStream_t)stream_) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_field_recorder_device_ptr(cavmd_field_recorder* r, const cavmd_field_record** records, const uint64_t** rows)
{
    return r ? r->device_ptr(records, rows) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_snapshot_field_recorder_bytes(cavmd_field_recorder* r, size_t* bytes)
{
    return snapshot_bytes(r, bytes);
}

int cavmd_snapshot_field_recorder_save(cavmd_field_recorder* r, void* stream_, void* h_out, size_t bytes)
{
    return snapshot_save(r, (hipStream_t)stream_, h_out, bytes);
}

int cavmd_snapshot_field_recorder_load(cavmd_field_recorder* r, void* stream_, const void* h_in, size_t bytes)
{
    return snapshot_load(r, (hipStream_t)stream_, h_in, bytes);
}

} // extern "C"
