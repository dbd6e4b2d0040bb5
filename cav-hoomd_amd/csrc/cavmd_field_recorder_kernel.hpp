// cavmd_field_recorder_kernel.hpp -- the density field rho(k) of a batch of independent small systems and its correlation with
// each system's stored reference fields, F_r(t) = mean_k Re(rho_r(k) conj rho(k, t)), in ONE launch, one workgroup per system,
// appended to a time series in DEVICE memory: the fourth kernel of the batched step next to cavmd_batch_kernel.hpp (forces),
// cavmd_recorder_kernel.hpp (per-step observables) and cavmd_bussi_batch_kernel.hpp (thermostat).
//
// What the reference's FieldAutocorrelationTracker (src/cavitymd/analysis.py:260-418) does every step for every replica --
// compute_density_field for 50 wavevectors, compute_field_autocorr against up to 10 stored references, and now and then a new
// reference (act, :380-414: correlate with all active references FIRST, then maybe add one) -- is one 160-byte row here.  Write
// position, reference count and the row of the last reference live in device memory, so a graph replay appends a NEW row and
// takes references when they are due exactly like an eager call.  Workgroups never wait for each other; the item's workgroup
// is the only writer of its counters, its series and its reference fields (no atomics).
//
// Mapping: LANE = WAVEVECTOR, density_partials_kernel's, folded into one workgroup: wavevectors in chunks of 64 looped inside
// the workgroup, wave w walks the 64-particle tiles w, w + 4, ... in ascending order and inside a tile the particles in
// ascending order (coordinates through scalar loads from the uniform tile address on the fast path), two plain fp64
// accumulators per lane, and the four waves meet in LDS where wave 0 adds them in WAVE order.  The sum order is therefore a
// function of (N, n_k) alone.  Term arithmetic, sincos_reduced and the per-tile choice between the fast path and the device
// library's sincos are density_partials_kernel's own (the device functions are used by inclusion).
#pragma once

#include "cavmd_observable_kernels.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr unsigned kFieldMaxK = CAVMD_FIELD_MAX_WAVEVECTORS;
constexpr unsigned kFieldMaxRefs = CAVMD_FIELD_MAX_REFERENCES;

typedef const __attribute__((address_space(4))) double* FieldConstPtr; // read-only for the kernel's duration: scalar loads

// One system as the kernel reads it: the layout of cavmd_field_item (the table is uploaded as it is).
struct FieldRow
{
    const char* pos;
    uint64_t stride;
    unsigned N;
    unsigned pad0;
    uint64_t pad[5];
};
static_assert(sizeof(FieldRow) == 64, "one field-recorder row = 64 bytes");

// Six words per item, kept as six arrays of n_items (rows first: that array is what cavmd_field_recorder_device_ptr hands
// out).  phase and slot are calls % period and rows % capacity, carried along so that the kernel never divides.
enum FieldCounter
{
    kFldRows = 0,
    kFldCalls = 1,
    kFldPhase = 2,
    kFldSlot = 3,
    kFldRefs = 4,    // references stored
    kFldLastRef = 5, // row at which the last one was taken
    kFldCounters = 6
};

// The run clock's rule as the TIMED kernel finds it in device memory, written by cavmd_runclock_field_set_rule; behind it
// last_time (n_items doubles) and last_reference_time (n_items doubles), which the kernel writes.
struct FieldRule
{
    const char* time0;    // item i's clock is the double at time0 + i * time_stride
    uint64_t time_stride; // bytes
    double time_interval, ref_time_interval;
};
static_assert(sizeof(FieldRule) == 32, "the time words behind the rule are 8-byte aligned");

// blockIdx.x -> order[blockIdx.x] (items by N descending, sorted on the host) -> the row, fetched once per workgroup.
// Counters, series and fields are indexed by ITEM, never by block.
// field_now: [item][n_k][2], refs: [item][max_refs][n_k][2], ref_rows: [item][max_refs].
// Both kernels have one body, cavmd_field_recorder_body.inc.  The first is the kernel of an object without a time rule, as it
// was before there was one; the second is launched while cavmd_runclock_field_set_rule has a rule on.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void field_recorder_batch_kernel(
    const FieldRow* __restrict__ rows, const unsigned* __restrict__ order, unsigned n_items, const double* __restrict__ kvec,
    unsigned n_k, SinCosCoef coef, uint64_t capacity, uint64_t period, unsigned max_refs, uint64_t interval,
    const unsigned* __restrict__ take, cavmd_field_record* __restrict__ series, uint64_t* __restrict__ counters,
    uint64_t* __restrict__ ref_rows, double* __restrict__ field_now, double* __restrict__ refs)
{
    constexpr bool TIMED = false;
    FieldRule* const rule = nullptr;
#include "cavmd_field_recorder_body.inc"
}

template <int BLOCK, bool TIMED>
__global__ __launch_bounds__(BLOCK) void field_recorder_batch_kernel(
    const FieldRow* __restrict__ rows, const unsigned* __restrict__ order, unsigned n_items, const double* __restrict__ kvec,
    unsigned n_k, SinCosCoef coef, uint64_t capacity, unsigned max_refs, uint64_t interval, const unsigned* __restrict__ take,
    cavmd_field_record* __restrict__ series, uint64_t* __restrict__ counters, uint64_t* __restrict__ ref_rows,
    double* __restrict__ field_now, double* __restrict__ refs, FieldRule* __restrict__ rule)
{
    constexpr uint64_t period = 1;
#include "cavmd_field_recorder_body.inc"
}
} // namespace cavmd
