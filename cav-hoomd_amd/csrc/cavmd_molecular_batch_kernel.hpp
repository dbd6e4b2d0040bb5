// cavmd_molecular_batch_kernel.hpp -- harmonic bonds and Lennard-Jones pairs of a batch of independent small systems in ONE
// launch: the molecular forces between cavmd_verlet_batch_kernel.hpp's two half-steps, next to cavmd_batch_kernel.hpp's cavity
// force.
//
// The reference's driver takes both from HOOMD-blue (hoomd.md.bond.Harmonic, hoomd.md.pair.LJ(mode='shift') over a neighbour
// list that excludes bonded pairs, examples/05_advanced_run.py:566-596).  The expressions below restate EvaluatorBondHarmonic,
// EvaluatorPairLJ and BoxDim::minImage of HOOMD-blue 4.x [HOOMD upstream, not in checkout]; include/cavmd.h carries them, with
// the summation order, as the contract.  Every operation is one IEEE rounding (no FMA).
//
// A system of n particles gets ceil(n / ROWS) workgroups (the host's table: blockIdx.x -> item, first particle, start of the
// item's partner table).  A workgroup stages x, y, z and the type id of its WHOLE system into LDS (28 B a particle) and the
// pair table behind them; then S = BLOCK / ROWS adjacent lanes share one particle i: lane s walks j = s, s + S, ... out of LDS
// (S distinct addresses per wave access, the rest broadcast: no bank conflict), lane 0 of the group also takes i's bonds, and
// the group folds its S partial sums left to right with shuffles.  No neighbour list, no halving by Newton's third law, no
// atomics, no workgroup waits for another one; every loop is bounded by n, every index into LDS is below n (the partner tables
// are built and checked by the library), and every entry of the force array is written by its owner.
#pragma once

#include "cavmd_reduce.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr int kMolecularBlock = 256;
constexpr int kMolecularMaxTypes = 8;
constexpr int kMolecularMaxBonds = 4;
constexpr unsigned kMolecularNoPartner = 0xFFFFFFFFu;
constexpr int kMolecularPairWords = 6; // lj1, lj2, lj1_12, lj2_6, rcutsq, eshift: what of a pair entry goes into LDS

// One system as the kernel reads it.
struct MolecularRow
{
    const v2d* pos2;
    v2d* force2;
    double Lx, Ly, Lz;
    unsigned n;
    unsigned pad0;
    uint64_t pad[2];
};
static_assert(sizeof(MolecularRow) == 64, "one molecular row = 64 bytes");

// The layouts of cavmd_molecular_pair and cavmd_molecular_params (uploaded as they are).
struct MolecularPair
{
    double c[kMolecularPairWords];
    uint64_t pad[2];
};
struct MolecularParams
{
    unsigned n_types, n_bond_types;
    uint64_t pad;
    MolecularPair pair[kMolecularMaxTypes][kMolecularMaxTypes];
    double bond[8][2]; // K, r0
};
static_assert(sizeof(MolecularPair) == 64 && sizeof(MolecularParams) == 4240, "molecular parameter layout");

// What a launch finds its tables through.  The block lives in device memory at an address that never changes, so a captured
// launch follows the tables set_items builds: blocks[b] = {item, first particle, first entry of the item's partner table, 0};
// partners[k] = the four slots of one particle, each partner | bond type << 16, kMolecularNoPartner when empty, filled from
// slot 0.
struct MolecularHeader
{
    const uint4* blocks;
    const uint4* partners;
    unsigned n_blocks;
    unsigned pad0;
    uint64_t pad;
};
static_assert(sizeof(MolecularHeader) == 32, "molecular launch header = 32 bytes");

// bytes of dynamic LDS a launch needs for systems of up to lds_n particles (lds_n even)
constexpr size_t molecular_lds_bytes(unsigned lds_n)
{
    return (size_t)lds_n * 28 + sizeof(double) * kMolecularMaxTypes * kMolecularMaxTypes * kMolecularPairWords;
}

// lds_n: the particles the launch has LDS for (frozen with the launch, as the LDS size is); a system beyond it -- a table
// rewritten after the capture -- gets NaN forces, never an out-of-bounds access.
template <int BLOCK, int S>
__global__ __launch_bounds__(BLOCK) void molecular_force_kernel(const MolecularRow* __restrict__ rows,
                                                                const MolecularHeader* __restrict__ hdr,
                                                                const MolecularParams* __restrict__ prm, unsigned lds_n)
{
    static_assert(S >= 1 && S <= kWave && (S & (S - 1)) == 0 && BLOCK % S == 0, "S lanes of one wave share a particle");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_molecular[];
    if (blockIdx.x >= hdr->n_blocks)
        return; // a launch captured for a larger table
    const uint4 blk = hdr->blocks[blockIdx.x];
    const unsigned item = __builtin_amdgcn_readfirstlane(blk.x);
    const unsigned first = __builtin_amdgcn_readfirstlane(blk.y);
    const unsigned partner_base = __builtin_amdgcn_readfirstlane(blk.z);
    const MolecularRow* __restrict__ row = rows + item;
    const unsigned n = row->n;
    const v2d* __restrict__ pos2 = row->pos2;
    v2d* __restrict__ force2 = row->force2;
    const unsigned r = threadIdx.x / S, s = threadIdx.x % S;
    const unsigned i = first + r;
    const bool owner = (i < n);
    if (n > lds_n)
    {
        if (owner && s == 0)
        {
            const double nan = __builtin_nan("");
            const v2d bad = {nan, nan};
            force2[2 * (size_t)i] = bad;
            force2[2 * (size_t)i + 1] = bad;
        }
        return;
    }
    double* __restrict__ sx = reinterpret_cast<double*>(s_molecular);
    double* __restrict__ sy = sx + lds_n;
    double* __restrict__ sz = sy + lds_n;
    double* __restrict__ s_pair = sz + lds_n;
    int* __restrict__ st = reinterpret_cast<int*>(s_pair + kMolecularMaxTypes * kMolecularMaxTypes * kMolecularPairWords);

    const unsigned n_types = min(prm->n_types, (unsigned)kMolecularMaxTypes);
    for (unsigned j = threadIdx.x; j < n; j += BLOCK)
    {
        const v2d xy = pos2[2 * (size_t)j], zw = pos2[2 * (size_t)j + 1];
        sx[j] = xy.x;
        sy[j] = xy.y;
        sz[j] = zw.x;
        st[j] = __double2loint(zw.y);
    }
    for (unsigned k = threadIdx.x; k < n_types * n_types * kMolecularPairWords; k += BLOCK)
    {
        const unsigned a = k / (n_types * kMolecularPairWords), rest = k % (n_types * kMolecularPairWords);
        const unsigned b = rest / kMolecularPairWords, w = rest % kMolecularPairWords;
        s_pair[(a * kMolecularMaxTypes + b) * kMolecularPairWords + w] = prm->pair[a][b].c[w];
    }
    __syncthreads();

    const double Lx = row->Lx, Ly = row->Ly, Lz = row->Lz;
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5;
    const unsigned ii = owner ? i : 0u; // lanes past the end walk nothing and write nothing, but take part in the shuffles
    const double xi = sx[ii], yi = sy[ii], zi = sz[ii];
    const unsigned ti = (unsigned)st[ii];
    uint4 slots = {kMolecularNoPartner, kMolecularNoPartner, kMolecularNoPartner, kMolecularNoPartner};
    if (owner)
        slots = hdr->partners[(size_t)partner_base + i];
    const unsigned slot[kMolecularMaxBonds] = {slots.x, slots.y, slots.z, slots.w};
    unsigned partner[kMolecularMaxBonds];
#pragma unroll
    for (int k = 0; k < kMolecularMaxBonds; ++k)
        partner[k] = (slot[k] == kMolecularNoPartner) ? kMolecularNoPartner : (slot[k] & 0xFFFFu);

    // the pair part: partial s of particle i
    double px = 0.0, py = 0.0, pz = 0.0, pw = 0.0;
    const unsigned j_end = (owner && ti < n_types) ? n : 0u;
    const double* __restrict__ s_pair_i = s_pair + (size_t)(ti < n_types ? ti : 0u) * kMolecularMaxTypes * kMolecularPairWords;
    for (unsigned j = s; j < j_end; j += S)
    {
        const unsigned tj = (unsigned)st[j];
        const bool excluded = (j == i) | (j == partner[0]) | (j == partner[1]) | (j == partner[2]) | (j == partner[3]);
        if (excluded || tj >= n_types)
            continue;
        const double dx = min_image(xi - sx[j], Lx, hx);
        const double dy = min_image(yi - sy[j], Ly, hy);
        const double dz = min_image(zi - sz[j], Lz, hz);
        const double rsq = (dx * dx + dy * dy) + dz * dz;
        const double* __restrict__ c = s_pair_i + tj * kMolecularPairWords;
        if (rsq < c[4])
        {
            const double r2inv = 1.0 / rsq;
            const double r6inv = (r2inv * r2inv) * r2inv;
            const double fdivr = (r2inv * r6inv) * ((c[2] * r6inv) - c[3]);
            const double e = r6inv * ((c[0] * r6inv) - c[1]) - c[5];
            px = px + dx * fdivr;
            py = py + dy * fdivr;
            pz = pz + dz * fdivr;
            pw = pw + 0.5 * e;
        }
    }
    // P = ((p0 + p1) + p2) + ...: every lane of the group folds the same S values in the same order
    double Px = __shfl(px, 0, S), Py = __shfl(py, 0, S), Pz = __shfl(pz, 0, S), Pw = __shfl(pw, 0, S);
#pragma unroll 1
    for (int k = 1; k < S; ++k) // not unrolled: 4 (S - 1) shuffles in flight at once cost S = 16 two thirds of its occupancy
    {
        Px = Px + __shfl(px, k, S);
        Py = Py + __shfl(py, k, S);
        Pz = Pz + __shfl(pz, k, S);
        Pw = Pw + __shfl(pw, k, S);
    }
    if (!owner || s != 0)
        return;

    // the bonds of i, in the order of its partner table
    double Bx = 0.0, By = 0.0, Bz = 0.0, Bw = 0.0;
    const unsigned n_bond_types = min(prm->n_bond_types, 8u);
#pragma unroll
    for (int k = 0; k < kMolecularMaxBonds; ++k)
    {
        const unsigned p = partner[k], bt = slot[k] >> 16;
        if (p >= n || bt >= n_bond_types) // an empty slot; the library's tables hold nothing else that fails this
            continue;
        const double dx = min_image(xi - sx[p], Lx, hx);
        const double dy = min_image(yi - sy[p], Ly, hy);
        const double dz = min_image(zi - sz[p], Lz, hz);
        const double rsq = (dx * dx + dy * dy) + dz * dz;
        const double K = prm->bond[bt][0], r0 = prm->bond[bt][1];
        const double rr = sqrt(rsq);
        const double fdivr = K * (r0 / rr - 1.0);
        const double e = (0.5 * K) * ((r0 - rr) * (r0 - rr));
        Bx = Bx + dx * fdivr;
        By = By + dy * fdivr;
        Bz = Bz + dz * fdivr;
        Bw = Bw + 0.5 * e;
    }
    const v2d Fxy = {Bx + Px, By + Py}, Fzw = {Bz + Pz, Bw + Pw};
    force2[2 * (size_t)i] = Fxy;
    force2[2 * (size_t)i + 1] = Fzw;
}
} // namespace cavmd
