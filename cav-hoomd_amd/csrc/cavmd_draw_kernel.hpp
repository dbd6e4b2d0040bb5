// cavmd_draw_kernel.hpp -- the step inputs of a batch of independent small systems drawn on the device, ONE launch per step:
// for every item its row of the integrator's input table (cavmd_verlet_batch_kernel.hpp reads it) and its row of the
// thermostat's (cavmd_bussi_batch_kernel.hpp reads it), with seeded counter-based variates and the step's dt.
//
// include/cavmd.h ("the step inputs of a batch, drawn on the device") carries the contract; in short, per item:
//   generator  Philox4x32-10, key = the 64-bit seed, counter = (draws low, draws high, item, purpose); `draws` is the item's
//              counter in DEVICE memory, read and then advanced here, so a graph replay draws a new block each time
//   doubles    k = (w_hi << 21) | (w_lo >> 11) of two words; k * 2^-53 in [0, 1); (k + 1) * 2^-53 in (0, 1] feeds log
//   normal     sqrt(-2 log u1) * cospi(2 u2)
//   gamma      Marsaglia-Tsang, at most kDrawGammaTries tries, then the variate is d and `exhausted` counts it
//   dt         dt_initial, or sqrt(tolerance / S) clamped, S being the force_mass_sum of the item's last recorded row
// One LANE per item: items cost the same, a row is 160 bytes, and nothing of an item is shared between lanes -- the row, the
// state and the record are fetched with per-lane vector loads (a scalar load serves a value the whole wave shares, which no
// value here is), and the three dependent loads of the adaptive rule (row counter -> record; state) are issued by all lanes
// of a wave together.  No workgroup waits for another, there are no atomics, nothing is mapped; the state is written with
// plain stores by the item's own lane.  Every operation outside log, exp, cospi is one IEEE rounding (no FMA).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace cavmd
{
constexpr int kDrawBlock = 256;
constexpr int kDrawGammaTries = 16;

// the purpose word of a Philox counter: which variate a block of four words feeds (no purpose is used twice)
constexpr unsigned kDrawPurposeLangevinXY = 0; // words 0,1 -> uniform[0]; words 2,3 -> uniform[1]
constexpr unsigned kDrawPurposeLangevinZ = 1;  // words 0,1 -> uniform[2]
constexpr unsigned kDrawPurposeNormal = 2;     // words 0,1 -> u1 (log); words 2,3 -> u2 (cospi): the thermostat's normal
constexpr unsigned kDrawPurposeBoost = 3;      // words 0,1 -> the boost uniform of a gamma shape below 1 (log)
constexpr unsigned kDrawPurposeGammaTry = 16;  // + 2 t: the normal of try t (as kDrawPurposeNormal); + 2 t + 1: words 0,1 ->
                                               // the acceptance uniform of try t (log)

// what the kernel reads of a cavmd_record (the layout is asserted where cavmd.h is visible)
struct DrawRecord
{
    uint64_t before[14];
    double force_mass_sum;
    double pad;
};
static_assert(sizeof(DrawRecord) == 128, "one record = 128 bytes");

// One item as the kernel reads it: cavmd_draw_item with, in its reserved words, the two fixed-mode columns the host took
// with cavmd_verlet_input_make / cavmd_bussi_batch_input_make.
struct DrawRow
{
    double* verlet_row; // 8 words: dt, gamma, coeff, uniform[3], skip, reserved
    double* bussi_row;  // 8 words: normal, gamma variate, c, set_T, skip, reserved[3]
    const DrawRecord* records;
    const uint64_t* rows;
    uint64_t capacity;
    double gamma, kT;
    double set_T, tau, dof;
    double dt_initial, tol_target, tol_initial, tol_time_constant, dt_min, dt_max;
    double fixed_coeff, fixed_c;
    uint64_t pad[2];
};
static_assert(sizeof(DrawRow) == 160, "one draw row = 160 bytes");

// Per-item state in device memory (the layout of cavmd_draw_state).
struct DrawState
{
    uint64_t draws;
    double dt, elapsed, tolerance;
    uint64_t exhausted;
    uint64_t finished; // cavmd_draw_state.reserved[0]: 1 while the item is at rest behind its end time
    uint64_t pad[2];
};
static_assert(sizeof(DrawState) == 64, "one draw state = 64 bytes");

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) with the published constants
__device__ __forceinline__ uint4 draw_philox(uint4 c, uint2 k)
{
#pragma unroll
    for (int round = 0; round < 10; ++round)
    {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// exact: the 53 bits of two words
__device__ __forceinline__ uint64_t draw_bits53(unsigned w_hi, unsigned w_lo)
{
    return ((uint64_t)w_hi << 21) | (uint64_t)(w_lo >> 11);
}
__device__ __forceinline__ double draw_unit(unsigned w_hi, unsigned w_lo) // [0, 1)
{
    return (double)draw_bits53(w_hi, w_lo) * 0x1p-53;
}
__device__ __forceinline__ double draw_log_arg(unsigned w_hi, unsigned w_lo) // (0, 1]
{
    return (double)(draw_bits53(w_hi, w_lo) + 1) * 0x1p-53;
}

struct DrawStream // one item's counter prefix and the key
{
    unsigned draws_lo, draws_hi, item;
    uint2 key;
    __device__ __forceinline__ uint4 block(unsigned purpose) const
    {
        return draw_philox(make_uint4(draws_lo, draws_hi, item, purpose), key);
    }
    // Box-Muller from one block
    __device__ __forceinline__ double normal(unsigned purpose) const
    {
        const uint4 w = block(purpose);
        return sqrt(-2.0 * log(draw_log_arg(w.x, w.y))) * cospi(2.0 * draw_unit(w.z, w.w));
    }
};

// Marsaglia-Tsang for shape a >= 1; a bounded loop; *exhausted is incremented if no try was accepted
__device__ __forceinline__ double draw_gamma_ge1(const DrawStream& s, double a, uint64_t* exhausted)
{
    const double d = a - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double out = d;
    bool accepted = false;
    for (int t = 0; t < kDrawGammaTries && !accepted; ++t)
    {
        const double x = s.normal(kDrawPurposeGammaTry + 2u * (unsigned)t);
        const uint4 w = s.block(kDrawPurposeGammaTry + 2u * (unsigned)t + 1u);
        const double logu = log(draw_log_arg(w.x, w.y));
        const double v1 = 1.0 + c * x;
        const double v = (v1 * v1) * v1;
        if (v > 0.0 && logu < (((0.5 * x) * x + d) - d * v) + d * log(v))
        {
            out = d * v;
            accepted = true;
        }
    }
    if (!accepted)
        *exhausted += 1;
    return out;
}

// Both kernels have one body, cavmd_draw_fill_body.inc.  The first is the kernel of an object without end times, as it was
// before there were any; the second is launched once cavmd_runclock_draw_set_end was called (t_end_all: n_items doubles).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void draw_fill_kernel(const DrawRow* __restrict__ rows, unsigned n_items, unsigned seed_lo,
                                                          unsigned seed_hi, DrawState* __restrict__ state_all)
{
    constexpr bool END = false;
    const double* const t_end_all = nullptr;
#include "cavmd_draw_fill_body.inc"
}

template <int BLOCK, bool END>
__global__ __launch_bounds__(BLOCK) void draw_fill_kernel(const DrawRow* __restrict__ rows, unsigned n_items, unsigned seed_lo,
                                                          unsigned seed_hi, DrawState* __restrict__ state_all,
                                                          const double* __restrict__ t_end_all)
{
#include "cavmd_draw_fill_body.inc"
}
} // namespace cavmd
