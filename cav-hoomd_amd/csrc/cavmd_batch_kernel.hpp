// cavmd_batch_kernel.hpp -- a batch of independent small systems in ONE launch, one workgroup per system.
//
// The reference's production workload is N = 501 run as 500 independent replicas (submit.sh:3,
// examples/05_advanced_run.py:1570-1612).  One such system is one 256-thread workgroup (cavity_small_system_kernel), which
// occupies one CU of 256; a caller that holds many replicas on one GPU hands them over as a table of rows and gets one
// workgroup per row.  A workgroup runs cavmd_small_system_body.hpp on its row: the same program text, hence the same
// bits, as the single-system kernel.  Workgroups never wait for each other.
#pragma once

#include "cavmd_force_kernels.hpp"

namespace cavmd
{
// One system of a batch as the kernel reads it (the device twin of cavmd_batch_item, quotients of the parameters taken on the
// host as for every kernel here).  128 bytes, so a row never straddles two 128-byte lines.
struct BatchRow
{
    const v2d* pos2;
    const double* charge;
    const int* image;
    v2d* force2;
    double Lx, Ly, Lz;
    DeviceParams prm;
    unsigned N;
    int L_typeid;
    uint64_t pad[4];
};
static_assert(sizeof(BatchRow) == 128, "one batch row = 128 bytes");

// blockIdx.x -> order[blockIdx.x] (items sorted by N descending on the host: the hardware hands out workgroups in blockIdx
// order, so the long systems start first) -> the row -> the evaluation (cavmd_small_system_body.hpp).
// The row index depends on blockIdx only and goes
// through readfirstlane, so the row (pointers, box, parameters) is fetched with scalar loads into SGPRs, once per workgroup.
// Results and host blocks are indexed by ITEM, never by block.  `res_host` is the base of this evaluation's n_items blocks
// in mapped host memory.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cavity_batch_kernel(const BatchRow* __restrict__ rows,
                                                             const unsigned* __restrict__ order, uint64_t sequence,
                                                             cavmd_result* __restrict__ res_all,
                                                             HostResult* __restrict__ res_host_all)
{
    const unsigned item = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const BatchRow* __restrict__ row = rows + item;
    const unsigned N = row->N;
    cavmd_result* __restrict__ res = res_all + item;
    HostResult* __restrict__ res_host = res_host_all + item;
    if (N == 0)
    {
        // an empty system: nothing of it is read or written except its result block
        if (threadIdx.x == 0)
        {
            Scalars sc;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                sc.d[k] = sc.dlo[k] = sc.dtot[k] = sc.q[k] = sc.e[k] = sc.f[k] = 0.0;
            sc.Dq[0] = sc.Dq[1] = 0.0;
            sc.photon = -1;
            sc.nL = 0;
            write_result(res, sc, 0u, 0u, sequence);
            publish_to_host(res_host, sc, 0u, 0u, sequence);
        }
        return;
    }
    // (The array pointers come out of memory, so the compiler addresses the particle loads as flat_*, not global_*: same
    // data path, one more counter to wait on.  Its cost has not been measured separately: DESIGN.md 3.3c.)
    AosInput in;
    in.pos2 = row->pos2;
    in.charge = row->charge;
    in.image = row->image;
    v2d* __restrict__ force2 = row->force2;
    const double Lx = row->Lx, Ly = row->Ly, Lz = row->Lz;
    const DeviceParams prm = row->prm;
    const int L_typeid = row->L_typeid;
#include "cavmd_small_system_body.hpp" // the body of cavity_small_system_kernel, shared as text
}
} // namespace cavmd
