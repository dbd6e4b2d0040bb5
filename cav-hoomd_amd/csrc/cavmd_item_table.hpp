// Host-only: what the thirteen "batch of small systems" objects share.  They live in seven units: cavmd_batch.hip (the batch
// and the shared cavity), cavmd_bussi_batch.hip, cavmd_recorder.hip (the recorder, the ledger, which has its shape, and the trajectory),
// cavmd_field_recorder.hip, cavmd_verlet.hip (the integrator, the draw object that writes its input rows, the bath that
// supplies its second half-step and the thermalize object that starts a run), cavmd_molecular.hip and cavmd_coulomb.hip.
// ItemTable is how a table of items lives on the host and on the device; create_table makes an object and ties it to its
// parent, ItemTable::launch launches it and destroy_table releases it.  Three flavours state what more an object keeps:
// SeriesTable, a ring of records per item (the two recorders, the ledger and the trajectory); StateTable, one state per
// item (the integrator, the draw object, the bath, the thermalize object and the thermostat batch); LinkedTable, tables derived
// from the items that the kernels find through a header at a fixed device address and that set_items replaces together (the
// two force batches and the shared cavity).  What a SeriesTable or a StateTable holds on the device can be saved to a host blob and loaded back
// (snapshot_bytes / snapshot_save / snapshot_load below, on the arithmetic of cavmd_snapshot.hpp).
// Those units see cavmd_workspace as an incomplete type: what they need of one is its WorkspaceTie.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "cavmd.h"
#include "cavmd_host_support.hpp" // DeviceGuard, hip_status, CAVMD_HIP_TRY, stream_capturing, DeviceArray
#include "cavmd_snapshot.hpp"     // the blob's header, its sections and snapshot_check (host arithmetic, no HIP)

// What an object built on an item table needs of the parent it was created from: the device, and the count of live objects
// that the parent's destroy refuses on.  The parent is a workspace, or for a bath its integrator (cavmd_verlet::bath_tie).
// cavmd_workspace_tie (cavmd_capi.hip) hands out the workspace's; it is called when an object is created and never on a
// launch path.
struct WorkspaceTie
{
    int device = -1;
    unsigned dependents = 0; // live objects created from this parent (ItemTable::attach)
};
__attribute__((visibility("hidden"))) WorkspaceTie* cavmd_workspace_tie(cavmd_workspace* ws);

// the tie create_table takes from an entry point that is given a workspace
inline WorkspaceTie* tie_of(cavmd_workspace* ws)
{
    return ws ? cavmd_workspace_tie(ws) : nullptr;
}

namespace
{
constexpr size_t kRecorderMaxBytes = (size_t)1 << 30; // of one recorder's series (and, for a field recorder, its fields)

// waits for what was enqueued on `stream`; a capturing stream cannot be waited for
inline int sync_uncaptured(hipStream_t stream)
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
    WorkspaceTie* tie = nullptr;   // of the parent this object was attached to: the parent's destroy refuses while it lives
    std::vector<Item> items;       // host copy of the table, as the caller gave it
    std::vector<unsigned> order;   // items by key descending, stable
    cavmd::DeviceArray<Row> d_rows;
    cavmd::DeviceArray<unsigned> d_order;
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

    // What create_table asks of an object; one that has more to say hides these.
    static constexpr bool tied = true; // attached to the parent it was created from
    int check_new(const Item* h_items, size_t n_items)
    {
        return check_items(h_items, n_items, check);
    }
    int capacity_status(size_t) const // called after the items passed: CAVMD_ERR_CAPACITY for a ring or series too large
    {
        return CAVMD_OK;
    }
    hipError_t alloc_own() // the object's buffers beyond rows and order (the caller holds the DeviceGuard)
    {
        return hipSuccess;
    }

    // allocates and fills d_rows, then d_order (the caller holds the DeviceGuard)
    hipError_t upload()
    {
        std::vector<Row> rows(n);
        for (size_t i = 0; i < n; ++i)
            rows[i] = to_row(items[i]);
        const hipError_t e = d_rows.upload(rows.data(), n);
        return e == hipSuccess ? d_order.upload(order.data(), n) : e;
    }

    // a complete object is tied to the parent it was created from
    void attach(WorkspaceTie* w)
    {
        tie = w;
        tie->dependents += 1;
    }

    void detach()
    {
        if (tie)
            tie->dependents -= 1;
        tie = nullptr;
    }

    // THE launch of the objects built on an item table: under the guard of the table's device, with the launch error as the
    // status; a launch that went through is noted, so that wait_idle() waits for its stream
    template <class Kernel, class... Args>
    int launch(hipStream_t stream, Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, Args... args)
    {
        DeviceGuard guard(device);
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
        const int st = hip_status(hipGetLastError());
        if (st == CAVMD_OK)
        {
            last_stream = stream;
            enqueued = true;
        }
        return st;
    }

    // THE wait for the launches in flight, which read the table and write the object's results (the caller holds the
    // DeviceGuard); a stream that is being captured cannot be waited for
    int wait_idle()
    {
        return enqueued ? sync_uncaptured(last_stream) : CAVMD_OK;
    }

    bool within(size_t first, size_t count, const Item* h_items) const
    {
        return h_items && count != 0 && first < n && count <= n - first;
    }

    // A replacement of items [first, first + count) goes in three steps, so that an object with more to replace than rows can
    // put its own device writes between them: stage() waits for the launches in flight (or refuses) and builds the new table
    // and order aside, write() copies order and rows to the device, commit() makes the host agree.
    struct Staged
    {
        std::vector<Item> items;
        std::vector<unsigned> order;
        std::vector<Row> rows; // of the replaced items
    };

    int stage(size_t first, size_t count, const Item* h_items, Staged* s)
    {
        const int st = wait_idle();
        if (st != CAVMD_OK)
            return st;
        s->items = items;
        s->rows.resize(count);
        for (size_t i = 0; i < count; ++i)
        {
            s->items[first + i] = h_items[i];
            s->rows[i] = to_row(h_items[i]);
        }
        s->order = launch_order(s->items, key);
        return CAVMD_OK;
    }

    // a failed copy leaves the device's table as it was, up to the rows already overwritten by a copy that died half-way
    int write(size_t first, const Staged& s)
    {
        CAVMD_HIP_TRY(hipMemcpy(d_order.ptr, s.order.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice));
        const hipError_t e = hipMemcpy(d_rows.ptr + first, s.rows.data(), sizeof(Row) * s.rows.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess)
            (void)hipMemcpy(d_order.ptr, order.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice); // the old order back
        return hip_status(e);
    }

    void commit(Staged&& s)
    {
        items.swap(s.items);
        order.swap(s.order);
    }

    int set_items(size_t first, size_t count, const Item* h_items)
    {
        if (!within(first, count, h_items))
            return CAVMD_ERR_INVALID_VALUE;
        int st = check_items(h_items, count, check);
        if (st != CAVMD_OK)
            return st;
        DeviceGuard guard(device);
        Staged s;
        st = stage(first, count, h_items, &s);
        if (st == CAVMD_OK)
            st = write(first, s);
        if (st == CAVMD_OK)
            commit(std::move(s)); // only now: a failed copy leaves the host's view as it was
        return st;
    }

    // before the object goes: let the launches in flight finish (the caller holds the DeviceGuard; a capturing stream cannot
    // be waited for, and then nothing of it runs)
    void quiesce()
    {
        (void)wait_idle();
    }

    // what snapshot_load asks of an object once the device holds the blob's sections (`sections`: where each begins in the
    // blob); one whose host keeps something derived from them hides this
    void snapshot_loaded(const char* const*)
    {
    }
};

// The end of every object built on an item table: guard, quiesce, detach, delete -- the buffers go with their owners.
template <class Table>
int destroy_table(Table* t)
{
    if (!t)
        return CAVMD_OK;
    DeviceGuard guard(t->device);
    t->quiesce();
    t->detach();
    delete t;
    return CAVMD_OK;
}

// The beginning of every object built on an item table, for `args`, the status of the entry point's own arguments, and
// `init`, which sets the object's own fields from them.  In this order: the arguments, the items, the capacity rule; then the
// table and the object's buffers on the device, ONE device synchronise (the zeroing memsets are done before any stream of
// the caller's, a non-blocking one included, launches), the tie to the parent.  Any failure destroys what was built.
// `tie` is the parent's: an entry point that takes a workspace passes tie_of(ws).
template <class Table, class Item, class Init>
int create_table(WorkspaceTie* tie, size_t n_items, const Item* h_items, Table** out, int args, Init init)
{
    if (!out)
        return CAVMD_ERR_INVALID_VALUE;
    *out = nullptr;
    if (!tie || !h_items || n_items == 0 || n_items > CAVMD_BATCH_MAX_ITEMS)
        return CAVMD_ERR_INVALID_VALUE;
    if (args != CAVMD_OK)
        return args;
    Table* t = new (std::nothrow) Table();
    if (!t)
        return (int)hipErrorOutOfMemory;
    t->device = tie->device; // whoever destroys the object holds the guard of this device
    init(t);
    int st = t->check_new(h_items, n_items);
    if (st == CAVMD_OK)
        st = t->capacity_status(n_items);
    if (st == CAVMD_OK)
    {
        t->adopt(tie->device, h_items, n_items);
        DeviceGuard guard(t->device);
        hipError_t e = t->upload();
        if (e == hipSuccess)
            e = t->alloc_own();
        if (e == hipSuccess)
            e = hipDeviceSynchronize();
        st = hip_status(e);
    }
    if (st != CAVMD_OK)
    {
        destroy_table(t);
        return st;
    }
    if (Table::tied)
        t->attach(tie);
    *out = t;
    return CAVMD_OK;
}

// ---- save and restore (include/cavmd.h; the blob's arithmetic is cavmd_snapshot.hpp's) ------------------------------------------
// Written once for every flavour.  An object names its shape, snapshot_shape() -- a flavour's state_shape / series_shape with
// the object's kind and words -- and the flavour (or the object, if it has more) its device arrays in the blob's order,
// snapshot_arrays(); the sizes follow from the shape alone.
template <class Table>
int snapshot_bytes(Table* t, size_t* bytes)
{
    if (!t || !bytes)
        return CAVMD_ERR_INVALID_VALUE;
    *bytes = (size_t)t->snapshot_shape().bytes;
    return CAVMD_OK;
}

template <class Table>
int snapshot_save(Table* t, hipStream_t stream, void* h_out, size_t bytes)
{
    if (!t || !h_out)
        return CAVMD_ERR_INVALID_VALUE;
    const cavmd_snapshot_header h = t->snapshot_shape();
    if ((uint64_t)bytes != h.bytes)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(t->device);
    const int st = sync_uncaptured(stream);
    if (st != CAVMD_OK)
        return st;
    uint64_t sizes[cavmd::kSnapshotMaxSections];
    const void* arrays[cavmd::kSnapshotMaxSections];
    const size_t count = cavmd::snapshot_sections(h, sizes);
    if (t->snapshot_arrays(arrays) != count)
        return CAVMD_ERR_INVALID_VALUE;
    char* out = static_cast<char*>(h_out);
    memcpy(out, &h, sizeof(h));
    size_t at = sizeof(h);
    for (size_t k = 0; k < count; ++k)
    {
        const size_t padded = (size_t)cavmd::snapshot_pad16(sizes[k]);
        CAVMD_HIP_TRY(hipMemcpy(out + at, arrays[k], (size_t)sizes[k], hipMemcpyDeviceToHost));
        memset(out + at + sizes[k], 0, padded - (size_t)sizes[k]);
        at += padded;
    }
    return CAVMD_OK;
}

template <class Table>
int snapshot_load(Table* t, hipStream_t stream, const void* h_in, size_t bytes)
{
    if (!t || !h_in || stream_capturing(stream))
        return CAVMD_ERR_INVALID_VALUE;
    const cavmd_snapshot_header h = t->snapshot_shape();
    int st = cavmd::snapshot_check(h_in, bytes, &h);
    if (st != CAVMD_OK)
        return st;
    uint64_t sizes[cavmd::kSnapshotMaxSections];
    const void* arrays[cavmd::kSnapshotMaxSections];
    const size_t count = cavmd::snapshot_sections(h, sizes);
    if (t->snapshot_arrays(arrays) != count)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(t->device);
    // the launches in flight: the object's own (set_items' wait), and what the caller replays on `stream`
    st = t->wait_idle();
    if (st == CAVMD_OK)
        st = sync_uncaptured(stream);
    if (st != CAVMD_OK)
        return st;
    const char* in = static_cast<const char*>(h_in);
    const char* sections[cavmd::kSnapshotMaxSections];
    size_t at = sizeof(h);
    for (size_t k = 0; k < count; ++k)
    {
        sections[k] = in + at;
        CAVMD_HIP_TRY(hipMemcpy(const_cast<void*>(arrays[k]), sections[k], (size_t)sizes[k], hipMemcpyHostToDevice));
        at += (size_t)cavmd::snapshot_pad16(sizes[k]);
    }
    t->snapshot_loaded(sections); // (hipMemcpy has returned: the copies are complete, whichever stream launches next)
    return CAVMD_OK;
}

// An item table whose launches append Records to a time series in device memory: per item a ring of `capacity` records and
// `n_counters` words, the words kept as n_counters arrays of n with the rows-written array first.  A record is `record_bytes`
// long: sizeof(Record), or for an object whose record size is a run-time value (the trajectory's frames, Record = unsigned
// char) what the object sets before alloc_series.
template <class Item, class Row, class Record>
struct SeriesTable : ItemTable<Item, Row>
{
    const unsigned n_counters;
    size_t capacity = 0;
    size_t record_bytes = sizeof(Record);    // a multiple of sizeof(Record)
    cavmd::DeviceArray<Record> d_series;     // n x capacity records, item-major
    cavmd::DeviceArray<uint64_t> d_counters; // n_counters arrays of n words

    SeriesTable(unsigned n_counters_, int (*check_)(const Item*), unsigned (*key_)(const Item&), Row (*to_row_)(const Item&))
        : ItemTable<Item, Row>(check_, key_, to_row_), n_counters(n_counters_)
    {
    }

    // allocates and zeroes the series, then the counters
    hipError_t alloc_series()
    {
        const hipError_t e = d_series.alloc_zeroed(this->n * capacity * (record_bytes / sizeof(Record)));
        return e == hipSuccess ? d_counters.alloc_zeroed((size_t)n_counters * this->n) : e;
    }

    int rows(hipStream_t stream, uint64_t* out)
    {
        DeviceGuard guard(this->device);
        const int st = sync_uncaptured(stream);
        if (st != CAVMD_OK)
            return st;
        CAVMD_HIP_TRY(hipMemcpy(out, d_counters.ptr, sizeof(uint64_t) * this->n, hipMemcpyDeviceToHost));
        return CAVMD_OK;
    }

    int read(hipStream_t stream, size_t first_item, size_t n_items, uint64_t first_row, size_t n_rows, Record* out)
    {
        if (!out || n_items == 0 || n_rows == 0 || first_item >= this->n || n_items > this->n - first_item)
            return CAVMD_ERR_INVALID_VALUE;
        DeviceGuard guard(this->device);
        const int st = sync_uncaptured(stream);
        if (st != CAVMD_OK)
            return st;
        std::vector<uint64_t> written(n_items);
        CAVMD_HIP_TRY(hipMemcpy(written.data(), d_counters.ptr + first_item, sizeof(uint64_t) * n_items, hipMemcpyDeviceToHost));
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
        const size_t rec = record_bytes;
        const size_t slot0 = (size_t)(first_row % capacity);
        const size_t run0 = std::min(n_rows, capacity - slot0);
        const char* src = reinterpret_cast<const char*>(d_series.ptr) + first_item * capacity * rec;
        char* dst = reinterpret_cast<char*>(out);
        CAVMD_HIP_TRY(hipMemcpy2D(dst, n_rows * rec, src + slot0 * rec, capacity * rec, run0 * rec, n_items, hipMemcpyDeviceToHost));
        if (run0 < n_rows)
            CAVMD_HIP_TRY(hipMemcpy2D(dst + run0 * rec, n_rows * rec, src, capacity * rec, (n_rows - run0) * rec, n_items,
                                      hipMemcpyDeviceToHost));
        return CAVMD_OK;
    }

    int reset(hipStream_t stream)
    {
        DeviceGuard guard(this->device);
        CAVMD_HIP_TRY(hipMemsetAsync(d_counters.ptr, 0, sizeof(uint64_t) * n_counters * this->n, stream));
        return CAVMD_OK;
    }

    // the shape of the object's snapshot, and its arrays in the blob's order: the counters, then the whole ring
    cavmd_snapshot_header series_shape(uint32_t kind, uint32_t word0, uint32_t word1) const
    {
        return cavmd::snapshot_header_make(kind, this->n, capacity, record_bytes, n_counters, word0, word1);
    }
    size_t snapshot_arrays(const void** arrays) const
    {
        arrays[0] = d_counters.ptr;
        arrays[1] = d_series.ptr;
        return 2;
    }

    int device_ptr(const Record** records, const uint64_t** rows_written)
    {
        if (!records && !rows_written)
            return CAVMD_ERR_INVALID_VALUE;
        if (records)
            *records = d_series.ptr;
        if (rows_written)
            *rows_written = d_counters.ptr;
        return CAVMD_OK;
    }
};

// An item table with one State per item in device memory, zeroed at creation, which the launches update.  PublicState is the
// ABI struct the entry point names; the object static_asserts that its layout is State's.
template <class Item, class Row, class State>
struct StateTable : ItemTable<Item, Row>
{
    cavmd::DeviceArray<State> d_state; // n states, indexed by item

    using ItemTable<Item, Row>::ItemTable;

    hipError_t alloc_own()
    {
        return d_state.alloc_zeroed(this->n);
    }

    template <class PublicState>
    int read(hipStream_t stream, PublicState* out)
    {
        static_assert(sizeof(PublicState) == sizeof(State), "the states are read out as they are");
        if (!out)
            return CAVMD_ERR_INVALID_VALUE;
        DeviceGuard guard(this->device);
        const int st = sync_uncaptured(stream);
        if (st != CAVMD_OK)
            return st;
        CAVMD_HIP_TRY(hipMemcpy(out, d_state.ptr, sizeof(State) * this->n, hipMemcpyDeviceToHost));
        return CAVMD_OK;
    }

    int reset(hipStream_t stream)
    {
        DeviceGuard guard(this->device);
        CAVMD_HIP_TRY(hipMemsetAsync(d_state.ptr, 0, sizeof(State) * this->n, stream));
        return CAVMD_OK;
    }

    // the shape of the object's snapshot, and its one array
    cavmd_snapshot_header state_shape(uint32_t kind, uint32_t word0, uint32_t word1) const
    {
        return cavmd::snapshot_header_make(kind, this->n, 0, sizeof(State), 0, word0, word1);
    }
    size_t snapshot_arrays(const void** arrays) const
    {
        arrays[0] = d_state.ptr;
        return 1;
    }

    template <class PublicState>
    int state_device_ptr(const PublicState** out)
    {
        if (!out)
            return CAVMD_ERR_INVALID_VALUE;
        *out = reinterpret_cast<const PublicState*>(d_state.ptr);
        return CAVMD_OK;
    }
};

// ---- derived tables behind a header ----------------------------------------------------------------------------------------
// The helpers of the objects whose kernels read, besides the rows, tables the library derives from each item.

inline bool finite_nonnegative(double x)
{
    return isfinite(x) && x >= 0.0;
}

// a periodic box: three finite positive edges; *cut_sq = (half the shortest edge)^2, the largest squared cut-off under which
// the minimum image is the only image in range
inline bool box_ok(double Lx, double Ly, double Lz, double* cut_sq)
{
    const double L[3] = {Lx, Ly, Lz};
    for (double l : L)
        if (!(isfinite(l) && l > 0.0))
            return false;
    const double h = std::min(L[0], std::min(L[1], L[2])) * 0.5;
    *cut_sq = h * h;
    return true;
}

// The partner slots of N particles from a host pair list: `cap` slots a particle, `empty` where there is no partner, filled
// from slot 0 in list order with word(partner, type of the pair).  Refuses an index >= N, a pair of a particle with itself and
// a particle's (cap + 1)-th partner.  `slots` NULL: the status alone.
inline int partner_slots(uint32_t N, const cavmd_molecular_bond* pairs, uint32_t n_pairs, unsigned cap, uint32_t empty,
                  uint32_t (*word)(uint32_t partner, uint32_t type), std::vector<uint32_t>* slots)
{
    std::vector<uint8_t> count(N, 0);
    if (slots)
        slots->assign((size_t)N * cap, empty);
    for (uint32_t k = 0; k < n_pairs; ++k)
    {
        const cavmd_molecular_bond& p = pairs[k];
        if (p.a >= N || p.b >= N || p.a == p.b)
            return CAVMD_ERR_INVALID_VALUE;
        if (count[p.a] >= cap || count[p.b] >= cap)
            return CAVMD_ERR_INVALID_VALUE;
        if (slots)
        {
            (*slots)[(size_t)p.a * cap + count[p.a]] = word(p.b, p.type);
            (*slots)[(size_t)p.b * cap + count[p.b]] = word(p.a, p.type);
        }
        count[p.a] += 1;
        count[p.b] += 1;
    }
    return CAVMD_OK;
}

// appends an item's part to the pool of all items; returns where it starts
template <class T>
uint32_t pool_append(std::vector<T>* pool, const std::vector<T>& part)
{
    const size_t base = pool->size();
    pool->insert(pool->end(), part.begin(), part.end());
    return (uint32_t)base;
}

// one entry per workgroup of an item with `count` particles (or k-vectors), `rows` of them a workgroup: {item, first, z, w}
inline void emit_blocks(std::vector<uint4>* table, unsigned item, unsigned count, unsigned rows, unsigned z, unsigned w)
{
    for (unsigned first = 0; first < count; first += rows)
        table->push_back(make_uint4(item, first, z, w));
}

// particles a launch gets LDS for: the largest N of the table, rounded up to even, at least 2
inline unsigned lds_particles(unsigned largest)
{
    return std::max(2u, (largest + 1u) & ~1u);
}

// An item table with, per item, host tables derived from it (Derived: partner slots, k-vectors) and, pooled over the items,
// device tables (Tables: the arrays, their `header` and `lds_n`) that the kernels find through a header at a device address
// that never changes -- so a launch captured before set_items follows the new tables.  The object names what is its own: the
// status of one item, what of an item is not kept, and how the device tables follow from items, launch order and derived
// tables.  Creation, replacement and the moment the old arrays are freed are here, once.
template <class Item, class Row, class Derived, class Tables>
struct LinkedTable : ItemTable<Item, Row>
{
    using Base = ItemTable<Item, Row>;
    cavmd::DeviceArray<decltype(Tables::header)> d_header; // never reallocated
    Tables tables;                                  // replaced as a whole
    std::vector<Derived> derived;                   // per item (the caller's lists are not kept)

    // (no `check`: the items of this table pass item_status instead)
    LinkedTable(unsigned (*key_)(const Item&), Row (*to_row_)(const Item&)) : Base(nullptr, key_, to_row_) {}

    // the status of one item, writing its derived tables into `out` unless that is NULL
    virtual int item_status(const Item* it, Derived* out) const = 0;
    // takes the caller's host lists out of an item that is kept
    virtual void strip(Item* it) const = 0;
    // fills fresh device arrays and t->header, t->lds_n for `all` items launched in the order `launch`
    virtual hipError_t fill(const std::vector<Item>& all, const std::vector<unsigned>& launch, const std::vector<Derived>& d,
                            Tables* t) const = 0;

    int check_into(const Item* h_items, size_t count, Derived* out) const
    {
        for (size_t i = 0; i < count; ++i)
        {
            const int st = item_status(h_items + i, out + i);
            if (st != CAVMD_OK)
                return st;
        }
        return CAVMD_OK;
    }

    hipError_t copy_header(const Tables& t)
    {
        return hipMemcpy(d_header.ptr, &t.header, sizeof(t.header), hipMemcpyHostToDevice);
    }

    // create_table's hooks (hiding ItemTable's): the items pass item_status, which fills `derived`; what is kept of them has
    // the caller's lists taken out; header and tables follow rows and order
    int check_new(const Item* h_items, size_t n_items)
    {
        derived.resize(n_items);
        return check_into(h_items, n_items, derived.data());
    }

    void adopt(int device_, const Item* h_items, size_t n_items)
    {
        Base::adopt(device_, h_items, n_items);
        for (Item& it : this->items)
            strip(&it);
    }

    hipError_t alloc_own()
    {
        hipError_t e = d_header.alloc_zeroed(1);
        if (e == hipSuccess)
            e = fill(this->items, this->order, derived, &tables);
        return e == hipSuccess ? copy_header(tables) : e;
    }

    // (hides ItemTable's: the rows are only a part of what is replaced here)
    int set_items(size_t first, size_t count, const Item* h_items)
    {
        if (!this->within(first, count, h_items))
            return CAVMD_ERR_INVALID_VALUE;
        std::vector<Derived> new_derived(derived);
        int st = check_into(h_items, count, new_derived.data() + first);
        if (st != CAVMD_OK)
            return st;
        std::vector<Item> kept(h_items, h_items + count);
        for (Item& it : kept)
            strip(&it);
        DeviceGuard guard(this->device);
        typename Base::Staged s;
        st = this->stage(first, count, kept.data(), &s); // refuses during a capture: nothing below may run in one
        if (st != CAVMD_OK)
            return st;
        // device writes: the new tables into fresh arrays, then order and rows, then the header that points to the tables
        Tables t;
        CAVMD_HIP_TRY(fill(s.items, s.order, new_derived, &t));
        st = this->write(first, s);
        if (st != CAVMD_OK)
            return st;
        CAVMD_HIP_TRY(copy_header(t));
        // The one commit of the host's state, after the last device copy went through.  A copy that failed above returned with
        // the host's view as it was; on the device a failed header copy leaves the new order and rows next to the old header
        // and its (still allocated) old tables, until a set_items over the same items goes through.
        this->commit(std::move(s));
        derived.swap(new_derived);
        tables = std::move(t); // the old arrays are freed here: nothing in flight reads them (stage() has waited)
        return CAVMD_OK;
    }
};
} // namespace
