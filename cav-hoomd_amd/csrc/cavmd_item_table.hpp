// Host-only: what the "batch of small systems in one launch" objects of cavmd_capi.hip share -- how a table of items lives on
// the host and on the device (ItemTable) and, for the two recorders, the per-item ring of records behind it (SeriesTable).
// cavmd_capi.hip includes this once, after its DeviceGuard and CAVMD_HIP_TRY, which the code below uses.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cavmd.h"
#include "cavmd_host_support.hpp" // stream_capturing

namespace
{
// waits for what was enqueued on `stream`; a capturing stream cannot be waited for
int sync_uncaptured(hipStream_t stream)
{
    if (stream_capturing(stream))
        return CAVMD_ERR_INVALID_VALUE;
    CAVMD_HIP_TRY(hipStreamSynchronize(stream));
    return CAVMD_OK;
}

// Launch order: items by key(item) descending, ties in item order (the hardware starts workgroups in blockIdx order, so the
// long systems of a ragged batch go first and the short ones fill in behind them).
template <class Item>
std::vector<unsigned> launch_order(const std::vector<Item>& items, unsigned (*key)(const Item&))
{
    // counting would do; B <= 65536 and this is set-up time
    std::vector<unsigned> order(items.size());
    for (size_t i = 0; i < items.size(); ++i)
        order[i] = (unsigned)i;
    std::stable_sort(order.begin(), order.end(), [&](unsigned x, unsigned y) { return key(items[x]) > key(items[y]); });
    return order;
}

// the first status that is not CAVMD_OK among `count` items, in item order
template <class Item>
int check_items(const Item* h_items, size_t count, int (*check)(const Item*))
{
    for (size_t i = 0; i < count; ++i)
    {
        const int st = check(h_items + i);
        if (st != CAVMD_OK)
            return st;
    }
    return CAVMD_OK;
}

// the conversion of a table whose items are uploaded as they are (the object static_asserts that the two layouts agree)
template <class Item, class Row>
Row uploaded_as_it_is(const Item& it)
{
    static_assert(sizeof(Row) == sizeof(Item), "the item table is uploaded as it is");
    Row r;
    memcpy(&r, &it, sizeof(r));
    return r;
}

// A table of n items: the host copy, the launch order, and both on the device from upload() on.  An object derives from it
// and names, once, the status of one item, the size key the launch order sorts by and the row the kernel reads for an item.
template <class Item, class Row>
struct ItemTable
{
    int (*const check)(const Item*);
    unsigned (*const key)(const Item&);
    Row (*const to_row)(const Item&);
    int device = -1;
    size_t n = 0;
    std::vector<Item> items;     // host copy of the table, as the caller gave it
    std::vector<unsigned> order; // items by key descending, stable
    Row* d_rows = nullptr;
    unsigned* d_order = nullptr;
    hipStream_t last_stream = nullptr;
    bool enqueued = false; // some launch was enqueued: last_stream means something

    ItemTable(int (*check_)(const Item*), unsigned (*key_)(const Item&), Row (*to_row_)(const Item&))
        : check(check_), key(key_), to_row(to_row_)
    {
    }

    void adopt(int device_, const Item* h_items, size_t n_items)
    {
        device = device_;
        n = n_items;
        items.assign(h_items, h_items + n_items);
        order = launch_order(items, key);
    }

    // allocates and fills d_rows, then d_order (the caller holds the DeviceGuard and frees through quiesce_and_free)
    hipError_t upload()
    {
        std::vector<Row> rows(n);
        for (size_t i = 0; i < n; ++i)
            rows[i] = to_row(items[i]);
        hipError_t e = hipMalloc((void**)&d_rows, sizeof(Row) * n);
        if (e == hipSuccess)
            e = hipMemcpy(d_rows, rows.data(), sizeof(Row) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMalloc((void**)&d_order, sizeof(unsigned) * n);
        if (e == hipSuccess)
            e = hipMemcpy(d_order, order.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice);
        return e;
    }

    // after a launch on `stream` went through
    void enqueued_on(hipStream_t stream)
    {
        last_stream = stream;
        enqueued = true;
    }

    int set_items(size_t first, size_t count, const Item* h_items)
    {
        if (!h_items || count == 0 || first >= n || count > n - first)
            return CAVMD_ERR_INVALID_VALUE;
        const int st = check_items(h_items, count, check);
        if (st != CAVMD_OK)
            return st;
        DeviceGuard guard(device);
        if (enqueued)
        {
            if (stream_capturing(last_stream))
                return CAVMD_ERR_INVALID_VALUE;
            CAVMD_HIP_TRY(hipStreamSynchronize(last_stream)); // launches in flight read the rows this call rewrites
        }
        // the new table and order are built aside and committed only after both copies went through: a failed copy leaves the
        // host's view and (up to the rows already overwritten by a copy that died half-way) the device's as they were
        std::vector<Item> new_items(items);
        std::vector<Row> rows(count);
        for (size_t i = 0; i < count; ++i)
        {
            new_items[first + i] = h_items[i];
            rows[i] = to_row(h_items[i]);
        }
        const std::vector<unsigned> new_order = launch_order(new_items, key);
        CAVMD_HIP_TRY(hipMemcpy(d_order, new_order.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice));
        const hipError_t e = hipMemcpy(d_rows + first, rows.data(), sizeof(Row) * count, hipMemcpyHostToDevice);
        if (e != hipSuccess)
        {
            (void)hipMemcpy(d_order, order.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice); // the old order back
            return (int)e;
        }
        items.swap(new_items);
        order = new_order;
        return CAVMD_OK;
    }

    // the launches in flight read the table and write the object's results: let them finish (a capturing stream cannot be
    // waited for), then free the table (the caller holds the DeviceGuard)
    void quiesce_and_free()
    {
        if (enqueued && !stream_capturing(last_stream))
            (void)hipStreamSynchronize(last_stream);
        if (d_rows)
            (void)hipFree(d_rows);
        if (d_order)
            (void)hipFree(d_order);
    }
};

// An item table whose launches append Records to a time series in device memory: per item a ring of `capacity` records and
// `n_counters` words, the words kept as n_counters arrays of n with the rows-written array first.
template <class Item, class Row, class Record>
struct SeriesTable : ItemTable<Item, Row>
{
    const unsigned n_counters;
    size_t capacity = 0;
    Record* d_series = nullptr;     // n x capacity records, item-major
    uint64_t* d_counters = nullptr; // n_counters arrays of n words

    SeriesTable(unsigned n_counters_, int (*check_)(const Item*), unsigned (*key_)(const Item&), Row (*to_row_)(const Item&))
        : ItemTable<Item, Row>(check_, key_, to_row_), n_counters(n_counters_)
    {
    }

    // allocates and zeroes the series, then the counters
    hipError_t alloc_series()
    {
        const size_t series_bytes = sizeof(Record) * this->n * capacity;
        const size_t counter_bytes = sizeof(uint64_t) * n_counters * this->n;
        hipError_t e = hipMalloc((void**)&d_series, series_bytes);
        if (e == hipSuccess)
            e = hipMemset(d_series, 0, series_bytes);
        if (e == hipSuccess)
            e = hipMalloc((void**)&d_counters, counter_bytes);
        if (e == hipSuccess)
            e = hipMemset(d_counters, 0, counter_bytes);
        return e;
    }

    void free_series()
    {
        if (d_series)
            (void)hipFree(d_series);
        if (d_counters)
            (void)hipFree(d_counters);
    }

    int rows(hipStream_t stream, uint64_t* out)
    {
        DeviceGuard guard(this->device);
        const int st = sync_uncaptured(stream);
        if (st != CAVMD_OK)
            return st;
        CAVMD_HIP_TRY(hipMemcpy(out, d_counters, sizeof(uint64_t) * this->n, hipMemcpyDeviceToHost));
        return CAVMD_OK;
    }

    // the caller has checked that the items lie within the table and that n_items and n_rows are not 0
    int read(hipStream_t stream, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows, Record* out)
    {
        DeviceGuard guard(this->device);
        const int st = sync_uncaptured(stream);
        if (st != CAVMD_OK)
            return st;
        std::vector<uint64_t> written(n_items);
        CAVMD_HIP_TRY(hipMemcpy(written.data(), d_counters + first_item, sizeof(uint64_t) * n_items, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n_items; ++k)
        {
            if (written[k] == 0)
                return CAVMD_ERR_NOT_COMPUTED;
            if (first_row >= written[k] || n_rows > written[k] - first_row)
                return CAVMD_ERR_INVALID_VALUE;
            if (written[k] > capacity && first_row < written[k] - capacity)
                return CAVMD_ERR_EXPIRED;
        }
        // row j of an item sits in slot j % capacity of that item's stretch: at most two runs of slots, each fetched for all
        // the items with one strided copy
        const size_t rec = sizeof(Record);
        const size_t slot0 = (size_t)(first_row % capacity);
        const size_t run0 = std::min(n_rows, capacity - slot0);
        const Record* src = d_series + first_item * capacity;
        CAVMD_HIP_TRY(hipMemcpy2D(out, n_rows * rec, src + slot0, capacity * rec, run0 * rec, n_items, hipMemcpyDeviceToHost));
        if (run0 < n_rows)
            CAVMD_HIP_TRY(hipMemcpy2D(out + run0, n_rows * rec, src, capacity * rec, (n_rows - run0) * rec, n_items,
                                      hipMemcpyDeviceToHost));
        return CAVMD_OK;
    }

    int reset(hipStream_t stream)
    {
        DeviceGuard guard(this->device);
        CAVMD_HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(uint64_t) * n_counters * this->n, stream));
        return CAVMD_OK;
    }

    int device_ptr(const Record** records, const uint64_t** rows_written)
    {
        if (!records && !rows_written)
            return CAVMD_ERR_INVALID_VALUE;
        if (records)
            *records = d_series;
        if (rows_written)
            *rows_written = d_counters;
        return CAVMD_OK;
    }
};
} // namespace
