// cavmd_ewald_factored_kernel.hpp -- the FACTORED reciprocal-space method of the Ewald Coulomb batch: the two launches of
// cavmd_coulomb_batch_kernel.hpp with cos(k.x) and sin(k.x) taken from per-axis phase factors instead of one sincos per
// (particle, k).  The k-vectors lie on a lattice, k = 2 pi (mx / Lx, my / Ly, mz / Lz), so
//     exp(i k.x) = E_x(mx) E_y(my) E_z(mz),   E_c(m) = exp(i m phi_c),   phi_c = k1_c x_c,   k1_c = (2 pi * 1) / L_c:
// three sincos per particle, and about one complex multiplication per (particle, k).  The expressions, the kept set and order
// of k-vectors, the a_k table, the S(k) slots and everything of real space are the direct method's; include/cavmd.h states the
// order of the multiplications, which is the contract of this file:
//     E_c(0) = (1, 0);  E_c(1) = (cos phi_c, sin phi_c);  E_c(m) = E_c(m - 1) * E_c(1) for m = 2 .. M_c;  E_c(-m) = conj E_c(m)
//     a row (mx, my) of consecutive mz is cut into SEGMENTS of at most SEG vectors from its first mz on; for a segment that
//     starts at zs:  P(zs) = (E_x(mx) * E_y(my)) * E_z(zs);  P(mz + 1) = P(mz) * E_z(1)
//     a * b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re), no FMA
//
//   1. ewald_structure_factored_kernel: a system with G segments gets ceil(G / SEGROWS) workgroups.  Each walks the system in
//      tiles of TILE particles: 3 TILE lanes build the tile's E_x, E_y, E_z tables in LDS (one sincos and M_c - 1
//      multiplications each), then T = BLOCK / SEGROWS adjacent lanes share a segment, lane t walks j = t, t + T, ... of the
//      tile and adds q_j P to SEG pairs of registers; after the last tile the group folds left to right and lane 0 stores.
//   2. ewald_force_factored_kernel: ceil(n / ROWS) workgroups per system.  Real space, fold, self and background terms are
//      the direct kernel's own text (cavmd_coulomb_force_body.inc, the body of both); once every lane is done with the LDS
//      image of the system, 3 ROWS lanes write the tables of the workgroup's ROWS particles over it, and the S lanes of
//      particle i take the segments
//      g = s, s + S, ... in chunks of 2 S segments whose entries of ktab and structure the workgroup stages in LDS.
//
// The tables of the library (one array whose address is CoulombHeader::pad[0]; pad[1] = launch-1 workgroups | launch-2
// workgroups << 32; built by fill() of cavmd_coulomb.hip), all uint4:
//   ewald[0]            = {first entry of the launch-1 workgroup table, of the launch-2 one, of the item table, 0}
//   launch-1 table [b]  = {item, first segment of the workgroup (entry of `ewald`), its segments (<= SEGROWS), the item's k base}
//   launch-2 table [b]  = {item, first particle, first entry of the item's partner table, the item's k base}
//   item table [item]   = {first segment of the item (entry of `ewald`), its segments, Mx | My << 16, Mz}
//   a segment           = {mx | (my & 0xFFFF) << 16, zs (two's complement), count (1 .. SEG), first k of the segment in the item}
// No atomics, no workgroup waits for another one, every loop is bounded by n, a segment count or M_c, and every slot and every
// force entry is written by its owner.
#pragma once

#include "cavmd_coulomb_batch_kernel.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr int kEwaldTile = 64;    // particles whose tables are in LDS at a time (launch 1)
constexpr int kEwaldSegment = 8;  // SEG: k-vectors behind one (E_x E_y) E_z product
constexpr int kEwaldKSplit = 4;   // T: lanes that share a segment in launch 1
constexpr int kEwaldJSplit = 16;  // S: lanes that share a particle in launch 2

// bytes of dynamic LDS of launch 1 for per-axis limits of up to lds_m: three tables of (lds_m + 1) x TILE phases, TILE charges
constexpr size_t ewald_structure_lds_bytes(unsigned lds_m)
{
    return (size_t)kEwaldTile * (3 * ((size_t)lds_m + 1) * 16 + 8);
}

// ... and of launch 2 with `rows` particles a workgroup: the direct launch's image, later overwritten by the rows' tables and,
// behind them, a chunk of ktab and structure (2 S segments of SEG entries, 48 B each)
constexpr size_t ewald_force_lds_bytes(unsigned lds_n, unsigned lds_m, unsigned rows)
{
    const size_t image = coulomb_lds_bytes(lds_n);
    const size_t tables = (size_t)rows * 3 * ((size_t)lds_m + 1) * 16 + (size_t)2 * kEwaldJSplit * kEwaldSegment * 48;
    return image > tables ? image : tables;
}

// lds_m: the per-axis limit the launch has LDS for (frozen with the launch).  A system beyond it -- a table rewritten after
// the capture -- gets NaN structure factors here and NaN forces from launch 2, never an out-of-bounds access.
template <int BLOCK, int T, int SEG, int TILE>
__global__ __launch_bounds__(BLOCK) void ewald_structure_factored_kernel(const CoulombRow* __restrict__ rows,
                                                                         const CoulombHeader* __restrict__ hdr, unsigned lds_m)
{
    static_assert(T >= 1 && T <= kWave && (T & (T - 1)) == 0 && BLOCK % T == 0, "T lanes of one wave share a segment");
    static_assert(TILE % T == 0 && 3 * TILE <= BLOCK,
                  "lane t walks j = t, t + T, ... across tiles; one lane fills one axis of one particle");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_coulomb[];
    if (blockIdx.x >= (unsigned)hdr->pad[1])
        return; // a launch captured for a larger table
    const uint4* __restrict__ ewald = reinterpret_cast<const uint4*>(hdr->pad[0]);
    const uint4 top = ewald[0];
    const uint4 blk = ewald[(size_t)top.x + blockIdx.x];
    const unsigned item = __builtin_amdgcn_readfirstlane(blk.x);
    const unsigned seg_first = __builtin_amdgcn_readfirstlane(blk.y);
    const unsigned seg_count = __builtin_amdgcn_readfirstlane(blk.z);
    const unsigned k_base = __builtin_amdgcn_readfirstlane(blk.w);
    const uint4 info = ewald[(size_t)top.z + item];
    const unsigned Mx = __builtin_amdgcn_readfirstlane(info.z) & 0xFFFFu, My = __builtin_amdgcn_readfirstlane(info.z) >> 16;
    const unsigned Mz = __builtin_amdgcn_readfirstlane(info.w);
    const CoulombRow* __restrict__ row = rows + item;
    const unsigned n = row->n;
    const unsigned r = threadIdx.x / T, t = threadIdx.x % T;
    const bool owner = (r < seg_count);
    uint4 seg = {0u, 0u, 0u, 0u}; // lanes past the end walk nothing and write nothing, but take part in the shuffles
    if (owner)
        seg = ewald[(size_t)seg_first + r];
    const int mx = (int)(seg.x & 0xFFFFu), my = (int)(short)(seg.x >> 16), zs = (int)seg.y;
    const unsigned count = seg.z < (unsigned)SEG ? seg.z : (unsigned)SEG;
    v2d* __restrict__ out = hdr->structure + ((size_t)k_base + seg.w);
    if (Mx > lds_m || My > lds_m || Mz > lds_m)
    {
        if (owner && t == 0)
        {
            const double nan = __builtin_nan("");
            const v2d bad = {nan, nan};
            for (unsigned u = 0; u < count; ++u)
                out[u] = bad;
        }
        return;
    }
    // tables[axis][m][jj], then the tile's charges
    const unsigned stride = lds_m + 1;
    v2d* __restrict__ tables = reinterpret_cast<v2d*>(s_coulomb);
    double* __restrict__ sq = reinterpret_cast<double*>(tables + (size_t)3 * stride * TILE);
    const v2d* __restrict__ tx = tables;
    const v2d* __restrict__ ty = tables + (size_t)stride * TILE;
    const v2d* __restrict__ tz = tables + (size_t)2 * stride * TILE;
    const v2d* __restrict__ pos2 = row->pos2;
    const double* __restrict__ charge = row->charge;
    const unsigned fill_axis = threadIdx.x / TILE, fill_j = threadIdx.x % TILE;
    const double fill_L = fill_axis == 0 ? row->Lx : fill_axis == 1 ? row->Ly : row->Lz;
    const unsigned fill_M = fill_axis == 0 ? Mx : fill_axis == 1 ? My : Mz;

    double a[SEG], b[SEG];
#pragma unroll
    for (int u = 0; u < SEG; ++u)
    {
        a[u] = 0.0;
        b[u] = 0.0;
    }
    for (unsigned tile = 0; tile < n; tile += TILE)
    {
        const unsigned in_tile = (n - tile < (unsigned)TILE) ? n - tile : (unsigned)TILE;
        __syncthreads(); // the walk over the tile before is over
        if (fill_axis < 3 && fill_j < in_tile)
        {
            const size_t j = (size_t)tile + fill_j;
            const v2d xy = pos2[2 * j], zw = pos2[2 * j + 1];
            const double x = fill_axis == 0 ? xy.x : fill_axis == 1 ? xy.y : zw.x;
            ewald_fill_axis(tables + (size_t)fill_axis * stride * TILE + fill_j, TILE, x, fill_L, fill_M);
            if (fill_axis == 0)
                sq[fill_j] = charge[j];
        }
        __syncthreads();
        const unsigned j_end = owner ? in_tile : 0u;
        for (unsigned jj = t; jj < j_end; jj += T)
        {
            const v2d ex = ewald_power(tx + jj, mx, TILE), ey = ewald_power(ty + jj, my, TILE), ez = ewald_power(tz + jj, zs, TILE);
            const v2d e1 = tz[(size_t)TILE + jj];
            const double q = sq[jj];
            v2d p = ewald_mul(ewald_mul(ex, ey), ez);
#pragma unroll
            for (int u = 0; u < SEG; ++u)
            {
                if ((unsigned)u < count)
                {
                    a[u] = a[u] + q * p.x;
                    b[u] = b[u] + q * p.y;
                    p = ewald_mul(p, e1);
                }
            }
        }
    }
    // A = ((a_0 + a_1) + a_2) + ...: every lane of the group folds the same T values in the same order
#pragma unroll
    for (int u = 0; u < SEG; ++u)
    {
        double A = __shfl(a[u], 0, T), B = __shfl(b[u], 0, T);
#pragma unroll 1
        for (int v = 1; v < T; ++v)
        {
            A = A + __shfl(a[u], v, T);
            B = B + __shfl(b[u], v, T);
        }
        if (owner && t == 0 && (unsigned)u < count)
        {
            const v2d AB = {A, B};
            out[u] = AB;
        }
    }
}

// (lds_n as in the direct launch 2: the image of the system is staged first)
template <int BLOCK, int S, int SEG>
__global__ __launch_bounds__(BLOCK) void ewald_force_factored_kernel(const CoulombRow* __restrict__ rows,
                                                                     const CoulombHeader* __restrict__ hdr, unsigned lds_n,
                                                                     unsigned lds_m)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    constexpr bool FACTORED = true;
    constexpr unsigned PART = kCoulombPartAll;
#include "cavmd_coulomb_force_body.inc"
}

// the LONG part under the factored method (coulomb_long_kernel is the direct one), after ewald_structure_factored_kernel
template <int BLOCK, int S, int SEG>
__global__ __launch_bounds__(BLOCK) void ewald_long_factored_kernel(const CoulombRow* __restrict__ rows,
                                                                    const CoulombHeader* __restrict__ hdr, unsigned lds_n,
                                                                    unsigned lds_m)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    constexpr bool FACTORED = true;
    constexpr unsigned PART = kCoulombPartLong;
#include "cavmd_coulomb_force_body.inc"
}
} // namespace cavmd
