// cavmd_shared_cavity_kernel.hpp -- several systems of a batch coupled to ONE cavity mode, in TWO launches.
//
// A cavity is a set of 1 .. kSharedCavityMaxMembers items; one of them, the carrier, holds the photon.  The photon feels
// D = sum over the cavity's members of d_c, and every non-L particle of every member feels Dq = q_xy + (g/K) D_xy: the one
// force that crosses the boundaries of the systems of a batch (include/cavmd.h, cavmd_shared_cavity).
//   launch 1, shared_cavity_dipole_kernel: one workgroup per item; phase 1 of cavmd_small_system_body.hpp restated (same loads,
//             same Accum::add, same block_reduce); leaves the item's un-normalised block total in a 128-byte record, for a carrier
//             with the unwrapped photon row, and the cell dipole d_c.
//   launch 2, shared_cavity_force_kernel: one workgroup per item; folds the records of its cavity's members in ascending item
//             index (thread t: members t, t + 256, t + 512, t + 768 into an identity Accum; block_reduce; dd_norm inside
//             scalars_from_total), evaluates the scalars with the cavity's parameters and writes its own item's forces and result.
// Every member's workgroup performs the same fold on the same records, so all of them hold identical bits of Dq.  Inside a
// launch no workgroup waits for another one: there are no flags and no atomics, and the kernel boundary on the stream is what
// makes launch 1's records visible to launch 2 (the L2s of the XCDs are not coherent with each other).
// A cavity of one member gives, bit for bit, what cavity_batch_kernel gives for that item: merging (0, 0) with dd_merge is exact.
#pragma once

#include "cavmd_force_kernels.hpp"

#pragma clang fp contract(off)

namespace cavmd
{
constexpr unsigned kSharedCavityMaxMembers = 1024; // 4 records a thread of the fold
constexpr int kSharedCavityBlock = kSmallBlock;    // the block size of cavity_batch_kernel: the two paths share bits

// One item as the two kernels read it (the device twin of cavmd_shared_cavity_item; the parameters live with the cavity).
struct SharedCavityRow
{
    const v2d* pos2;
    const double* charge;
    const int* image;
    v2d* force2;
    double Lx, Ly, Lz;
    unsigned N;
    int L_typeid; // >= 0: the carrier of its cavity
    unsigned cavity;
    unsigned pad0;
    uint64_t pad[7];
};
static_assert(sizeof(SharedCavityRow) == 128, "one row = 128 bytes");

// What launch 1 leaves per item: the nine doubles and two ints of the block's Accum (not normalised), and for a carrier the
// unwrapped photon row with the photon's charge (read by launch 2 only if the carrier has more than one L-typed particle).
struct SharedCavityRecord
{
    double hx, lx, hy, ly, hz, lz;
    double sx, sy, sz;
    int lmin, lcnt;
    double qx, qy, qz;
    double pc;
    double pad[2];
};
static_assert(sizeof(SharedCavityRecord) == 128, "one record = 128 bytes: never straddles two lines");

// One cavity: its parameters (quotients taken on the host), its stretch of `members`, its carrier.
struct SharedCavity
{
    DeviceParams prm;
    unsigned first, count; // members[first .. first + count): item indices, ascending
    unsigned carrier;      // item index
    unsigned pad[5];
};
static_assert(sizeof(SharedCavity) == 64, "one cavity = 64 bytes");

// The tables derived from the items, found through this header at a device address that never changes: a launch captured
// before set_items follows the new membership.
struct SharedCavityHeader
{
    const SharedCavity* cavities;
    const unsigned* members;
    unsigned n_cavities;
    unsigned pad;
};

// The carrier's record as an input layout of scalars_from_total: the photon row is already unwrapped, so its images are zero.
struct SharedCavityPhotonInput
{
    double qx, qy, qz, pc;
    struct Raw
    {
        double px, py, pz, c;
        int ix, iy, iz;
    };
    __device__ __forceinline__ Raw load(size_t) const
    {
        return Raw {qx, qy, qz, pc, 0, 0, 0};
    }
    static __device__ __forceinline__ double x(const Raw& r) { return r.px; }
    static __device__ __forceinline__ double y(const Raw& r) { return r.py; }
    static __device__ __forceinline__ double z(const Raw& r) { return r.pz; }
};

// ---- launch 1 ------------------------------------------------------------------------------------------------------------------
// blockIdx.x -> order[blockIdx.x] (items by N descending, as the batch) -> the row.  records and cell_dipoles (4 doubles an
// item: x, y, z, 0) are indexed by ITEM.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void shared_cavity_dipole_kernel(const SharedCavityRow* __restrict__ rows,
                                                                     const unsigned* __restrict__ order,
                                                                     SharedCavityRecord* __restrict__ records,
                                                                     double* __restrict__ cell_dipoles)
{
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const SharedCavityRow* __restrict__ row = rows + item;
    const unsigned N = row->N;
    Accum acc;
    double qx = 0.0, qy = 0.0, qz = 0.0, pc = 0.0;
    if (N != 0) // (an empty system: nothing of it is read; its record is the identity)
    {
        AosInput in;
        in.pos2 = row->pos2;
        in.charge = row->charge;
        in.image = row->image;
        const double Lx = row->Lx, Ly = row->Ly, Lz = row->Lz;
        const int L_typeid = row->L_typeid;
        // phase 1 of cavmd_small_system_body.hpp, restated: particles base + j * BLOCK + tid, four in flight
        const PhotonRow guess = photon_row(in, (size_t)(N - 1));
        constexpr int BATCH = 4;
        for (unsigned base = 0; base < N; base += BATCH * BLOCK)
        {
            AosInput::Raw r[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; ++j)
            {
                const unsigned i = base + j * BLOCK + threadIdx.x;
                r[j] = in.load(i < N ? i : N - 1); // clamped, the duplicate is masked out below
            }
#pragma unroll
            for (int j = 0; j < BATCH; ++j)
            {
                const unsigned i = base + j * BLOCK + threadIdx.x;
                const double rx = AosInput::x(r[j]) + (double)r[j].ix * Lx;
                const double ry = AosInput::y(r[j]) + (double)r[j].iy * Ly;
                const double rz = AosInput::z(r[j]) + (double)r[j].iz * Lz;
                if (i < N)
                    acc.add(i, rx, ry, rz, r[j].c, AosInput::tag(r[j]), L_typeid);
            }
        }
        acc = block_reduce<BLOCK>(acc);
        if (threadIdx.x == 0 && acc.lmin != INT_MAX)
        {
            // the photon: the carrier's first particle of the named type, unwrapped as scalars_from_total unwraps it
            const int photon = acc.lmin;
            double px = guess.x, py = guess.y, pz = guess.z;
            int pix = guess.ix, piy = guess.iy, piz = guess.iz;
            if ((unsigned)photon != N - 1)
            {
                const PhotonRow r = photon_row(in, (size_t)photon);
                px = r.x; py = r.y; pz = r.z;
                pix = r.ix; piy = r.iy; piz = r.iz;
            }
            qx = px + (double)pix * Lx;
            qy = py + (double)piy * Ly;
            qz = pz + (double)piz * Lz;
            if (acc.lcnt > 1)
                pc = in.load((size_t)photon).c;
        }
    }
    if (threadIdx.x == 0)
    {
        SharedCavityRecord* __restrict__ rec = records + item;
        rec->hx = acc.hx; rec->lx = acc.lx; rec->hy = acc.hy; rec->ly = acc.ly; rec->hz = acc.hz; rec->lz = acc.lz;
        rec->sx = acc.sx; rec->sy = acc.sy; rec->sz = acc.sz;
        rec->lmin = acc.lmin;
        rec->lcnt = acc.lcnt;
        rec->qx = qx; rec->qy = qy; rec->qz = qz;
        rec->pc = pc;
        rec->pad[0] = rec->pad[1] = 0.0;
        // d_c, rounded once from the double-double
        dd_norm(acc.hx, acc.lx);
        dd_norm(acc.hy, acc.ly);
        dd_norm(acc.hz, acc.lz);
        double* __restrict__ d = cell_dipoles + 4 * (size_t)item;
        d[0] = acc.hx; d[1] = acc.hy; d[2] = acc.hz; d[3] = 0.0;
    }
}

// ---- launch 2 ------------------------------------------------------------------------------------------------------------------
// One workgroup per item, in the same order.  Results are indexed by ITEM.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void shared_cavity_force_kernel(const SharedCavityRow* __restrict__ rows,
                                                                    const unsigned* __restrict__ order,
                                                                    const SharedCavityHeader* __restrict__ header,
                                                                    const SharedCavityRecord* __restrict__ records,
                                                                    uint64_t sequence, cavmd_result* __restrict__ res_all)
{
    static_assert(4 * BLOCK >= (int)kSharedCavityMaxMembers, "a thread of the fold takes at most four members");
    __shared__ double s_m[5];
    __shared__ int s_mi[2];
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const SharedCavityRow* __restrict__ row = rows + item;
    const unsigned N = row->N;
    const SharedCavity* __restrict__ cav = header->cavities + row->cavity;
    const unsigned* __restrict__ members = header->members + cav->first;
    const unsigned count = cav->count; // 1 .. kSharedCavityMaxMembers (the host's table_check)
    const unsigned carrier = cav->carrier;
    const DeviceParams prm = cav->prm;

    // the fold, step 1: thread t merges members t, t + 256, t + 512, t + 768, in that order, into an identity Accum; the L-typed
    // sums, lmin and lcnt are the carrier's alone and join in thread 0 below
    constexpr int BATCH = 4;
    Accum o[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
    {
        const unsigned m = j * BLOCK + threadIdx.x;
        if (m < count)
        {
            const SharedCavityRecord* __restrict__ rec = records + members[m];
            o[j].hx = rec->hx; o[j].lx = rec->lx; o[j].hy = rec->hy; o[j].ly = rec->ly; o[j].hz = rec->hz; o[j].lz = rec->lz;
        }
    }
    Accum acc;
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
        if (j * BLOCK < (int)count) // block-uniform: skip batches nobody loaded
            acc.merge(o[j]);        // (a default-constructed Accum is the identity for the ragged last one)
    // step 2
    acc = block_reduce<BLOCK>(acc);
    SharedCavityPhotonInput in {0.0, 0.0, 0.0, 0.0};
    double own[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x == 0)
    {
        const SharedCavityRecord* __restrict__ rec = records + carrier;
        acc.sx = rec->sx; acc.sy = rec->sy; acc.sz = rec->sz;
        acc.lmin = rec->lmin;
        acc.lcnt = rec->lcnt;
        in.qx = rec->qx; in.qy = rec->qy; in.qz = rec->qz;
        in.pc = rec->pc;
        if (item != carrier)
        {
            const SharedCavityRecord* __restrict__ mine = records + item;
            own[0] = mine->hx; own[1] = mine->lx; own[2] = mine->hy; own[3] = mine->ly; own[4] = mine->hz; own[5] = mine->lz;
        }
    }
    // step 3 (dd_norm) and the scalars, by scalars_from_total itself: the photon row is the speculative one (N = photon + 1),
    // and an edge of -0.0 makes its unwrapping q + 0 * (-0.0) the identity on every q
    const PhotonRow guess = {in.qx, in.qy, in.qz, 0, 0, 0};
    const unsigned n_upto_photon = acc.lmin == INT_MAX ? 1u : (unsigned)acc.lmin + 1u;
    const Scalars sc = scalars_from_total<SharedCavityPhotonInput>(acc, guess, in, n_upto_photon, -0.0, -0.0, -0.0, prm, true);
    if (threadIdx.x == 0)
    {
        s_m[0] = sc.Dq[0]; s_m[1] = sc.Dq[1]; s_m[2] = sc.f[0]; s_m[3] = sc.f[1]; s_m[4] = sc.f[2];
        s_mi[0] = sc.photon;
        s_mi[1] = sc.nL;
    }
    __syncthreads();
    const double Dqx = s_m[0], Dqy = s_m[1], Fx = s_m[2], Fy = s_m[3], Fz = s_m[4];
    const bool coupled = s_mi[0] >= 0;                      // the carrier has a photon
    const int photon = item == carrier ? s_mi[0] : -1;      // local to the carrier
    const bool typed = item == carrier && s_mi[1] > 1;      // further L-typed particles: the carrier's alone
    const int L_typeid = row->L_typeid;
    const v2d* __restrict__ pos2 = row->pos2;
    const double* __restrict__ charge = row->charge;
    v2d* __restrict__ force2 = row->force2;
    const double ng = -prm.g;
    const unsigned nchunks = 2 * N;
    const bool odd = threadIdx.x & 1;
    const v2d zero = {0.0, 0.0};
    // the force map of cavmd_small_system_body.hpp, the charges from global memory: every 16-byte chunk of the item is written
    for (unsigned k = threadIdx.x; k < nchunks; k += BLOCK)
    {
        const unsigned p = k >> 1;
        v2d v = zero;
        if (coupled)
        {
            const double c = charge[p];
            const double sgc = ng * c; // ((-g) * charge) * Dq, src/CavityForceCompute.cc:194
            v = (v2d) {sgc * Dqx, sgc * Dqy};
            const bool typed_L = typed && (__double2loint(pos2[2 * p + 1].y) == L_typeid);
            v = (odd || typed_L) ? zero : v;
            if ((int)p == photon)
                v = odd ? (v2d) {Fz, 0.0} : (v2d) {Fx, Fy};
        }
        force2[k] = v;
    }
    if (threadIdx.x == 0)
    {
        cavmd_result* __restrict__ res = res_all + item;
        if (item == carrier)
            write_result(res, sc, N, count, sequence);
        else
        {
            // another member: its own cell's dipole, the cavity's q and Dq, no energy (the carrier's block holds the cavity's)
            Scalars mine;
            dd_norm(own[0], own[1]);
            dd_norm(own[2], own[3]);
            dd_norm(own[4], own[5]);
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                mine.d[k] = mine.dtot[k] = own[2 * k];
                mine.dlo[k] = own[2 * k + 1];
                mine.q[k] = sc.q[k];
                mine.e[k] = mine.f[k] = 0.0;
            }
            mine.Dq[0] = sc.Dq[0];
            mine.Dq[1] = sc.Dq[1];
            mine.photon = -1;
            mine.nL = 0;
            write_result(res, mine, N, 1u, sequence);
        }
    }
}
} // namespace cavmd
