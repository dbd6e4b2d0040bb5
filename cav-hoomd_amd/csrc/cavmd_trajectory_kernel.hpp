// cavmd_trajectory_kernel.hpp -- trajectory frames of a batch of independent small systems in ONE launch, one workgroup per
// system, appended to a ring of frames in DEVICE memory: the counterpart of the driver's hoomd.write.GSD
// (examples/05_advanced_run.py:1231-1246), which saves positions, images and velocities every --gsd-output-period-ps with the
// initial frame first.  The structure is ledger_batch_kernel's (the path from blockIdx to the row, thread 0 as the only reader
// and writer of the item's counters, the decision handed over through LDS, the ring); what differs is the record, a frame
// whose size is a run-time value (cavmd_trajectory_layout), and the rule of a call, which can go by the device clock.
//
// The rule of one call, per item (thread 0):
//   1. calls += 1; forced = d_take_frame && d_take_frame[item] != 0 (the word is only read);
//   2. time_interval == 0:  phase += 1; due = phase >= period                     (the recorder's rule)
//      time_interval  > 0:  t = *d_time; due = rows == 0 || t - last_time >= time_interval
//      -- _should_create_new_reference of src/cavitymd/analysis.py:366-378 (one subtraction, one comparison, so a NaN time
//      is never due by it) with the first frame written at once, as the driver's write_at_start;
//   3. due || forced: the frame goes to slot rows % capacity, last_time = *d_time (or 0), phase = 0, rows += 1;
//      otherwise only calls (and, by the step rule, phase) move and nothing else of the item is read.
//
// A frame: a 64-byte header, then three sections of packed rows x, y, z per particle -- positions and velocities as doubles
// (FORMAT 0, exact copies) or as (float)x (FORMAT 1, GSD's chunk types: round to nearest even, subnormal results kept, beyond
// the float range +-inf, NaN stays NaN), images as int32.  pos.w (the type tag) and vel.w (the mass) are never copied.
//
// A pass covers BLOCK particles.  Every lane issues all loads of its particle first (two 16-byte loads of pos, two of vel,
// the three image words; plain loads: step one reads the same lines next), converts and places x, y, z in LDS; behind one
// barrier the lanes write the pass's stretch of each section as consecutive 16-byte chunks (BLOCK * 24 and BLOCK * 12 bytes
// are multiples of 16 and the section bases are 16-byte aligned), so a store instruction of a wave covers 1 KiB of contiguous
// memory: the force map's chunk rule.  Lanes past N place zeros, which become the zero bytes between the end of the 3 N
// components and the section's next 16-byte boundary; nothing further of the slot is written.
#pragma once

#include "cavmd_observable_kernels.hpp"

namespace cavmd
{
// One system as the kernel reads it: the layout of cavmd_trajectory_item (the table is uploaded as it is).
struct TrajectoryRow
{
    const v2d* pos2;
    const int* image;
    const v2d* vel2;
    const double* time;
    double L[3];
    unsigned N;
    unsigned pad0;
};
static_assert(sizeof(TrajectoryRow) == 64, "one trajectory item = 64 bytes");

// Five words per item, kept as five arrays of n_items (rows first, as the recorder's): the recorder's four and the bits of the
// time of the item's last frame.
enum TrajectoryCounter
{
    kTrajRows = 0,
    kTrajCalls = 1,
    kTrajPhase = 2,
    kTrajSlot = 3,
    kTrajLastTime = 4,
    kTrajCounters = 5
};

constexpr unsigned kTrajFlagForced = 1u;     // cavmd_trajectory_header.flags
constexpr unsigned kTrajFlagVelocities = 2u;
constexpr unsigned kTrajHeaderBytes = 64;

// what the kernel needs of a cavmd_trajectory_layout
struct TrajectoryFrame
{
    uint64_t frame_bytes;
    uint64_t velocity_offset;
    uint64_t image_offset;
};

// the layout of cavmd_trajectory_header
struct TrajectoryHeader
{
    uint64_t call;
    uint64_t row;
    double time;
    unsigned N;
    unsigned flags;
    double box[3];
    uint64_t reserved;
};
static_assert(sizeof(TrajectoryHeader) == kTrajHeaderBytes, "one frame header = 64 bytes");

template <int FORMAT>
struct TrajectoryElement
{
    using type = double;
};
template <>
struct TrajectoryElement<1>
{
    using type = float;
};

// chunks [0, n_chunks) of 16 bytes from LDS to consecutive 16-byte chunks of global memory
template <int BLOCK>
__device__ __forceinline__ void trajectory_store_chunks(unsigned char* __restrict__ dst, const uint4* __restrict__ lds,
                                                        unsigned n_chunks)
{
    uint4* __restrict__ out = reinterpret_cast<uint4*>(__builtin_assume_aligned(dst, 16));
    for (unsigned c = threadIdx.x; c < n_chunks; c += BLOCK)
        out[c] = lds[c];
}

// blockIdx.x -> order[blockIdx.x] (items by N descending, sorted on the host) -> the item, fetched once per workgroup.
// Counters and series are indexed by ITEM, never by block.
template <int BLOCK, int FORMAT>
__global__ __launch_bounds__(BLOCK) void trajectory_batch_kernel(const TrajectoryRow* __restrict__ items,
                                                                 const unsigned* __restrict__ order, unsigned n_items,
                                                                 uint64_t capacity, uint64_t period, double time_interval,
                                                                 TrajectoryFrame frame, const unsigned* __restrict__ take_frame,
                                                                 unsigned char* __restrict__ series,
                                                                 uint64_t* __restrict__ counters)
{
    using Element = typename TrajectoryElement<FORMAT>::type;
    constexpr unsigned E = sizeof(Element);
    static_assert((BLOCK * 3 * E) % 16 == 0 && (BLOCK * 12) % 16 == 0, "a pass's stretch of a section is whole chunks");
    __shared__ __attribute__((aligned(16))) Element s_pos[BLOCK * 3];
    __shared__ __attribute__((aligned(16))) Element s_vel[BLOCK * 3];
    __shared__ __attribute__((aligned(16))) int s_img[BLOCK * 3];
    __shared__ unsigned s_record;
    __shared__ uint64_t s_slot;

    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const TrajectoryRow* __restrict__ it = items + item;
    uint64_t* __restrict__ c_rows = counters + (size_t)kTrajRows * n_items + item;
    uint64_t* __restrict__ c_calls = counters + (size_t)kTrajCalls * n_items + item;
    uint64_t* __restrict__ c_phase = counters + (size_t)kTrajPhase * n_items + item;
    uint64_t* __restrict__ c_slot = counters + (size_t)kTrajSlot * n_items + item;
    uint64_t* __restrict__ c_last = counters + (size_t)kTrajLastTime * n_items + item;

    // 1. does this call write a frame?  Thread 0 alone reads the counters (it is also their only writer) and tells the others.
    uint64_t calls = 0, phase = 0, n_rows = 0;
    double now = 0.0;
    if (threadIdx.x == 0)
    {
        calls = *c_calls + 1;
        const bool forced = take_frame && take_frame[item] != 0;
        bool due;
        if (time_interval == 0.0)
        {
            phase = *c_phase + 1;
            due = phase >= period;
        }
        else
        {
            n_rows = *c_rows;
            now = *it->time; // never NULL by this rule (create and set_items refuse it)
            due = n_rows == 0 || now - __builtin_bit_cast(double, *c_last) >= time_interval;
        }
        s_record = (due || forced) ? (1u | (forced ? 2u : 0u)) : 0u;
        s_slot = *c_slot;
    }
    __syncthreads();
    const unsigned record = s_record;
    if (!record)
    {
        if (threadIdx.x == 0)
        {
            *c_calls = calls;
            if (time_interval == 0.0)
                *c_phase = phase;
        }
        return;
    }

    // 2. the sections
    const unsigned N = it->N;
    const v2d* __restrict__ pos2 = it->pos2;
    const v2d* __restrict__ vel2 = it->vel2;
    const int* __restrict__ image = it->image;
    const uint64_t slot = s_slot;
    unsigned char* __restrict__ out = series + ((uint64_t)item * capacity + slot) * frame.frame_bytes;
    for (unsigned first = 0; first < N; first += BLOCK)
    {
        const unsigned i = first + threadIdx.x;
        v2d pxy = {0.0, 0.0}, pzw = {0.0, 0.0}, vxy = {0.0, 0.0}, vzw = {0.0, 0.0};
        int ix = 0, iy = 0, iz = 0;
        if (i < N)
        {
            pxy = pos2[2 * (size_t)i];
            pzw = pos2[2 * (size_t)i + 1];
            if (vel2)
            {
                vxy = vel2[2 * (size_t)i];
                vzw = vel2[2 * (size_t)i + 1];
            }
            ix = image[3 * (size_t)i];
            iy = image[3 * (size_t)i + 1];
            iz = image[3 * (size_t)i + 2];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (first != 0)
            __syncthreads(); // the chunks of the pass before have left LDS
        s_pos[3 * threadIdx.x] = (Element)pxy.x;
        s_pos[3 * threadIdx.x + 1] = (Element)pxy.y;
        s_pos[3 * threadIdx.x + 2] = (Element)pzw.x;
        s_vel[3 * threadIdx.x] = (Element)vxy.x;
        s_vel[3 * threadIdx.x + 1] = (Element)vxy.y;
        s_vel[3 * threadIdx.x + 2] = (Element)vzw.x;
        s_img[3 * threadIdx.x] = ix;
        s_img[3 * threadIdx.x + 1] = iy;
        s_img[3 * threadIdx.x + 2] = iz;
        __syncthreads();
        const unsigned count = (N - first < (unsigned)BLOCK) ? N - first : (unsigned)BLOCK;
        const unsigned chunks_e = (count * 3 * E + 15) / 16, chunks_i = (count * 12 + 15) / 16;
        trajectory_store_chunks<BLOCK>(out + kTrajHeaderBytes + (uint64_t)first * (3 * E), reinterpret_cast<const uint4*>(s_pos),
                                       chunks_e);
        trajectory_store_chunks<BLOCK>(out + frame.velocity_offset + (uint64_t)first * (3 * E),
                                       reinterpret_cast<const uint4*>(s_vel), chunks_e);
        trajectory_store_chunks<BLOCK>(out + frame.image_offset + (uint64_t)first * 12, reinterpret_cast<const uint4*>(s_img),
                                       chunks_i);
    }

    // 3. the header, then the counters
    if (threadIdx.x == 0)
    {
        if (time_interval == 0.0)
        {
            n_rows = *c_rows;
            now = it->time ? *it->time : 0.0;
        }
        TrajectoryHeader h;
        h.call = calls;
        h.row = n_rows;
        h.time = now;
        h.N = N;
        h.flags = ((record & 2u) ? kTrajFlagForced : 0u) | (vel2 ? kTrajFlagVelocities : 0u);
        h.box[0] = it->L[0];
        h.box[1] = it->L[1];
        h.box[2] = it->L[2];
        h.reserved = 0;
        // four 16-byte stores: the series is allocated by the library and every frame is a multiple of 16 bytes
        __builtin_memcpy(__builtin_assume_aligned(out, 16), &h, sizeof(h));
        *c_last = __builtin_bit_cast(uint64_t, now);
        record_counters_store(c_rows, c_calls, c_phase, c_slot, n_rows, slot, capacity, calls);
    }
}
} // namespace cavmd
