// cavmd_coulomb_batch_kernel.hpp -- Ewald Coulomb forces of a batch of independent small systems in TWO launches: the
// electrostatics next to cavmd_molecular_batch_kernel.hpp's bonds and Lennard-Jones pairs, between cavmd_verlet_batch_kernel.hpp's
// two half-steps.
//
// The reference's driver takes its electrostatics from HOOMD-blue's PPPM (make_pppm_coulomb_forces over the bond-excluding
// neighbour list, examples/05_advanced_run.py:598-608).  PPPM approximates the Ewald sum on a mesh; at N <= 2048 the sum itself
// is cheaper than a mesh and needs no FFT, so this file IS the Ewald sum, with the expressions of include/cavmd.h as the
// contract.  What separates it from a PPPM run is PPPM's discretisation error, which nothing in this repository measures.
//
//   1. coulomb_structure_kernel: a system with K kept k-vectors gets ceil(K / KROWS) workgroups.  Each stages x, y, z, q of
//      its WHOLE system into LDS (32 B a particle); T = BLOCK / KROWS adjacent lanes share one k-vector, lane t walks
//      j = t, t + T, ... and the group folds S(k) = sum_j q_j exp(i k.x_j) left to right with shuffles.  Lane 0 stores it.
//   2. coulomb_force_kernel: ceil(n / ROWS) workgroups per system, the same LDS image; S = BLOCK / ROWS adjacent lanes share
//      particle i and split first the j-walk (real-space term inside the cut-off, exclusion term for the listed partners, and
//      the total charge Q on the way) and then the k-walk (S(k) of launch 1 and the library's table of k and a_k out of global
//      memory), fold left to right with shuffles, and lane 0 adds the self and background terms and stores.  Its body is
//      cavmd_coulomb_force_body.inc, which the factored method's launch 2 (cavmd_ewald_factored_kernel.hpp) includes too.
//
// LDS is four arrays of doubles (x, y, z, q), not 32-byte records: the S (or T) lanes of a group read S consecutive doubles
// with one ds_read_b64 -- S distinct banks, every other lane of the wave a broadcast -- where records would put j and j + 8 on
// one bank.  No atomics, no workgroup waits for another one, every loop is bounded by n or K, every LDS index is below n (the
// partner tables are built and checked by the library), and every slot and every force entry is written by its owner.
#pragma once

#include "cavmd_ewald_phase.hpp"
#include "cavmd_reduce.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr int kCoulombBlock = 256;
constexpr int kCoulombMaxExclusions = 4;
constexpr unsigned kCoulombNoPartner = 0xFFFFFFFFu;
// which terms a kernel built on cavmd_coulomb_force_body.inc carries (PART there): the whole sum, or one of the two parts of
// include/cavmd.h (the values of CAVMD_COULOMB_PART_SHORT / CAVMD_COULOMB_PART_LONG)
constexpr unsigned kCoulombPartAll = 0, kCoulombPartShort = 1, kCoulombPartLong = 2;

// One system as the kernels read it.
struct CoulombRow
{
    const v2d* pos2;
    const double* charge;
    v2d* force2;
    double Lx, Ly, Lz;
    double kappa;   // > 0
    double rcutsq;  // r_cut * r_cut
    double self_c;  // kappa / sqrt(pi)
    double bg_c;    // pi / (2 V kappa^2)
    unsigned n;
    unsigned n_k; // K, the kept k-vectors
    uint64_t pad; // the item's LONG array (cavmd_mts_coulomb_set_long_forces), 0 without one: read by the LONG kernels alone
};
static_assert(sizeof(CoulombRow) == 96, "one coulomb row = 96 bytes");

// One kept k-vector, built by the library on the host: k and a_k = (4 pi / V) exp(-k^2 / (4 kappa^2)) / k^2.
struct CoulombK
{
    double kx, ky, kz, a;
};
static_assert(sizeof(CoulombK) == 32, "one k-table entry = 32 bytes");

// What the launches find their tables through.  The block lives in device memory at an address that never changes, so captured
// launches follow the tables set_items builds:
//   k_blocks[b] = {item, first k of the workgroup, first entry of the item's k-table, 0}                        (launch 1)
//   blocks[b]   = {item, first particle, first entry of the item's partner table, first entry of its k-table}   (launch 2)
//   partners[p] = the four slots of one particle, kCoulombNoPartner when empty, filled from slot 0
//   ktab[e], structure[e]: an item owns n_k + 1 consecutive entries; structure[base + k] = {A, B} of k-vector k, and
//   structure[base + n_k] = {Q, 0} (written by launch 2: it is the value the background term used).
struct CoulombHeader
{
    const uint4* k_blocks;
    const uint4* blocks;
    const uint4* partners;
    const CoulombK* ktab;
    v2d* structure;
    unsigned n_k_blocks;
    unsigned n_blocks;
    uint64_t pad[2];
};
static_assert(sizeof(CoulombHeader) == 64, "coulomb launch header = 64 bytes");

// bytes of dynamic LDS either launch needs for systems of up to lds_n particles
constexpr size_t coulomb_lds_bytes(unsigned lds_n)
{
    return (size_t)lds_n * 32;
}

// x, y, z, q of the n particles of `row` into the four LDS arrays
template <int BLOCK>
__device__ __forceinline__ void coulomb_stage(const CoulombRow* __restrict__ row, unsigned n, double* __restrict__ sx,
                                              double* __restrict__ sy, double* __restrict__ sz, double* __restrict__ sq)
{
    const v2d* __restrict__ pos2 = row->pos2;
    const double* __restrict__ charge = row->charge;
    for (unsigned j = threadIdx.x; j < n; j += BLOCK)
    {
        const v2d xy = pos2[2 * (size_t)j], zw = pos2[2 * (size_t)j + 1];
        sx[j] = xy.x;
        sy[j] = xy.y;
        sz[j] = zw.x;
        sq[j] = charge[j];
    }
    __syncthreads();
}

// lds_n: the particles the launch has LDS for (frozen with the launch, as the LDS size is).  A system beyond it -- a table
// rewritten after the capture -- gets NaN structure factors here and NaN forces from launch 2, never an out-of-bounds access.
template <int BLOCK, int T>
__global__ __launch_bounds__(BLOCK) void coulomb_structure_kernel(const CoulombRow* __restrict__ rows,
                                                                  const CoulombHeader* __restrict__ hdr, unsigned lds_n)
{
    static_assert(T >= 1 && T <= kWave && (T & (T - 1)) == 0 && BLOCK % T == 0, "T lanes of one wave share a k-vector");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_coulomb[];
    if (blockIdx.x >= hdr->n_k_blocks)
        return; // a launch captured for a larger table
    const uint4 blk = hdr->k_blocks[blockIdx.x];
    const unsigned item = __builtin_amdgcn_readfirstlane(blk.x);
    const unsigned first = __builtin_amdgcn_readfirstlane(blk.y);
    const unsigned base = __builtin_amdgcn_readfirstlane(blk.z);
    const CoulombRow* __restrict__ row = rows + item;
    const unsigned n = row->n, n_k = row->n_k;
    const unsigned r = threadIdx.x / T, t = threadIdx.x % T;
    const unsigned k = first + r;
    const bool owner = (k < n_k);
    v2d* __restrict__ out = hdr->structure + (size_t)base;
    if (n > lds_n)
    {
        if (owner && t == 0)
        {
            const double nan = __builtin_nan("");
            const v2d bad = {nan, nan};
            out[k] = bad;
        }
        return;
    }
    double* __restrict__ sx = reinterpret_cast<double*>(s_coulomb);
    double* __restrict__ sy = sx + lds_n;
    double* __restrict__ sz = sy + lds_n;
    double* __restrict__ sq = sz + lds_n;
    coulomb_stage<BLOCK>(row, n, sx, sy, sz, sq);

    // lanes past the end walk nothing and write nothing, but take part in the shuffles
    CoulombK kv = {0.0, 0.0, 0.0, 0.0};
    if (owner)
        kv = hdr->ktab[(size_t)base + k];
    double a = 0.0, b = 0.0;
    const unsigned j_end = owner ? n : 0u;
    for (unsigned j = t; j < j_end; j += T)
    {
        const double theta = (kv.kx * sx[j] + kv.ky * sy[j]) + kv.kz * sz[j];
        double sn, cs;
        sincos(theta, &sn, &cs);
        const double q = sq[j];
        a = a + q * cs;
        b = b + q * sn;
    }
    // A = ((a_0 + a_1) + a_2) + ...: every lane of the group folds the same T values in the same order
    double A = __shfl(a, 0, T), B = __shfl(b, 0, T);
#pragma unroll 1
    for (int u = 1; u < T; ++u)
    {
        A = A + __shfl(a, u, T);
        B = B + __shfl(b, u, T);
    }
    if (owner && t == 0)
    {
        const v2d AB = {A, B};
        out[k] = AB;
    }
}

template <int BLOCK, int S>
__global__ __launch_bounds__(BLOCK) void coulomb_force_kernel(const CoulombRow* __restrict__ rows,
                                                              const CoulombHeader* __restrict__ hdr, unsigned lds_n)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    constexpr bool FACTORED = false;
    constexpr unsigned PART = kCoulombPartAll;
    [[maybe_unused]] constexpr int SEG = 1;        // (of the factored method: nothing here reads them)
    [[maybe_unused]] constexpr unsigned lds_m = 0;
#include "cavmd_coulomb_force_body.inc"
}

// The two parts of the sum (include/cavmd.h, "the two parts of the Ewald sum"), the same body: SHORT into the item's force
// array -- no structure factor is read, so it needs no launch before it -- and LONG, after coulomb_structure_kernel, into the
// item's long array.  Workgroups, LDS image, j partition and fold are coulomb_force_kernel's.
template <int BLOCK, int S>
__global__ __launch_bounds__(BLOCK) void coulomb_short_kernel(const CoulombRow* __restrict__ rows,
                                                              const CoulombHeader* __restrict__ hdr, unsigned lds_n)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    constexpr bool FACTORED = false;
    constexpr unsigned PART = kCoulombPartShort;
    [[maybe_unused]] constexpr int SEG = 1;
    [[maybe_unused]] constexpr unsigned lds_m = 0;
#include "cavmd_coulomb_force_body.inc"
}

template <int BLOCK, int S>
__global__ __launch_bounds__(BLOCK) void coulomb_long_kernel(const CoulombRow* __restrict__ rows,
                                                             const CoulombHeader* __restrict__ hdr, unsigned lds_n)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    constexpr bool FACTORED = false;
    constexpr unsigned PART = kCoulombPartLong;
    [[maybe_unused]] constexpr int SEG = 1;
    [[maybe_unused]] constexpr unsigned lds_m = 0;
#include "cavmd_coulomb_force_body.inc"
}
} // namespace cavmd
