// cavmd_ewald_phase.hpp -- the per-axis phase factors of the factored reciprocal-space method (cavmd_ewald_factored_kernel.hpp,
// and the FACTORED part of cavmd_coulomb_force_body.inc): E_c(m) = exp(i m phi_c) from one sincos and complex multiplications
// in the order include/cavmd.h states.
#pragma once

#include "cavmd_reduce.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr double kEwaldTwoPi = 2.0 * 3.141592653589793;

__device__ __forceinline__ v2d ewald_mul(const v2d a, const v2d b)
{
    const v2d c = {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
    return c;
}

// E_c(m) out of a table of E_c(0 .. M_c) with `step` entries between consecutive m
__device__ __forceinline__ v2d ewald_power(const v2d* __restrict__ table, int m, unsigned step)
{
    v2d e = table[(size_t)(m < 0 ? -m : m) * step];
    if (m < 0)
        e.y = -e.y;
    return e;
}

// E_c(0 .. M) of coordinate x into table[0], table[step], ...: (1, 0), one sincos, M - 1 multiplications.  E_c(1) is written
// for M == 0 too (the walk along mz multiplies by it after its last vector).
__device__ __forceinline__ void ewald_fill_axis(v2d* __restrict__ table, unsigned step, double x, double L, unsigned M)
{
    const double k1 = (kEwaldTwoPi * 1.0) / L;
    const double phi = k1 * x;
    double sn, cs;
    sincos(phi, &sn, &cs);
    const v2d one = {1.0, 0.0}, e1 = {cs, sn};
    table[0] = one;
    table[step] = e1;
    v2d p = e1;
    for (unsigned m = 2; m <= M; ++m)
    {
        p = ewald_mul(p, e1);
        table[(size_t)m * step] = p;
    }
}
} // namespace cavmd
