// cavmd_force_kernels.hpp -- the cavity-force kernels: input layouts, dipole_partials_kernel, the fixed-order fold +
// scalars (reduce_partials_and_finalize), finalize_kernel and the force-map kernels.  Overview: cavmd_kernels.hpp.
#pragma once

#include <math.h>

#include "cavmd_reduce.hpp"
#include "cavmd_tile_schedule.hpp"

#pragma clang fp contract(off)

namespace cavmd
{

// ---- input layouts -------------------------------------------------------------------------------
// HOOMD-native AoS: Scalar4 pos (type tag in the low 32 bits of .w), Scalar charge, int3 image.
// NT: 0 = plain loads, 1 = pos and image non-temporal (read once per evaluation) but charge temporal (the force
// map reads it again), 2 = all three non-temporal.
template <int NT>
struct AosInputT
{
    const v2d* __restrict__ pos2;      // 2 x 16 B per particle
    const double* __restrict__ charge;
    const int* __restrict__ image;     // 3 ints per particle, 12-byte stride

    struct Raw
    {
        v2d xy, zw;
        double c;
        int ix, iy, iz;
    };
    __device__ __forceinline__ Raw load(size_t i) const
    {
        Raw r;
        const int* im = image + 3 * i;
        if (NT)
        {
            r.xy = __builtin_nontemporal_load(pos2 + 2 * i);
            r.zw = __builtin_nontemporal_load(pos2 + 2 * i + 1);
            r.c = (NT == 2) ? __builtin_nontemporal_load(charge + i) : charge[i];
            r.ix = __builtin_nontemporal_load(im + 0);
            r.iy = __builtin_nontemporal_load(im + 1);
            r.iz = __builtin_nontemporal_load(im + 2);
        }
        else
            r = load_cached(i);
        return r;
    }
    // Temporal loads whatever NT: for a row that every wave of the grid reads (speculative_photon_row).
    __device__ __forceinline__ Raw load_cached(size_t i) const
    {
        Raw r;
        const int* im = image + 3 * i;
        r.xy = pos2[2 * i];
        r.zw = pos2[2 * i + 1];
        r.c = charge[i];
        r.ix = im[0];
        r.iy = im[1];
        r.iz = im[2];
        return r;
    }
    // Every field of a row as an operand of an empty statement: the compiler places its counted wait for the row's loads here
    // (loads return in order, so nothing issued after the row is waited for), and no later load is moved above it.
    static __device__ __forceinline__ void landed(const Raw& r)
    {
        asm volatile("" : : "v"(r.xy), "v"(r.zw), "v"(r.c), "v"(r.ix), "v"(r.iy), "v"(r.iz) : "memory");
    }
    static __device__ __forceinline__ double x(const Raw& r) { return r.xy.x; }
    static __device__ __forceinline__ double y(const Raw& r) { return r.xy.y; }
    static __device__ __forceinline__ double z(const Raw& r) { return r.zw.x; }
    static __device__ __forceinline__ int tag(const Raw& r) { return __double2loint(r.zw.y); }
};
typedef AosInputT<0> AosInput;

// Snapshot layout with byte strides: position (N,3) f64, typeid (N,) i32, image (N,3) i32, charge (N,) f64.
struct StridedInput
{
    const char* __restrict__ pos;
    const char* __restrict__ tid;
    const char* __restrict__ img;
    const char* __restrict__ chg;
    size_t pos_stride, tid_stride, img_stride, chg_stride;

    struct Raw
    {
        double px, py, pz, c;
        int ix, iy, iz, t;
    };
    __device__ __forceinline__ Raw load(size_t i) const
    {
        Raw r;
        const double* p = reinterpret_cast<const double*>(pos + i * pos_stride);
        r.px = __builtin_nontemporal_load(p + 0);
        r.py = __builtin_nontemporal_load(p + 1);
        r.pz = __builtin_nontemporal_load(p + 2);
        r.c = *reinterpret_cast<const double*>(chg + i * chg_stride); // temporal: the force map reads it again
        const int* im = reinterpret_cast<const int*>(img + i * img_stride);
        r.ix = __builtin_nontemporal_load(im + 0);
        r.iy = __builtin_nontemporal_load(im + 1);
        r.iz = __builtin_nontemporal_load(im + 2);
        r.t = __builtin_nontemporal_load(reinterpret_cast<const int*>(tid + i * tid_stride));
        return r;
    }
    __device__ __forceinline__ Raw load_cached(size_t i) const // as AosInputT::load_cached
    {
        Raw r;
        const double* p = reinterpret_cast<const double*>(pos + i * pos_stride);
        r.px = p[0];
        r.py = p[1];
        r.pz = p[2];
        r.c = *reinterpret_cast<const double*>(chg + i * chg_stride);
        const int* im = reinterpret_cast<const int*>(img + i * img_stride);
        r.ix = im[0];
        r.iy = im[1];
        r.iz = im[2];
        r.t = *reinterpret_cast<const int*>(tid + i * tid_stride);
        return r;
    }
    static __device__ __forceinline__ void landed(const Raw& r) // as AosInputT::landed
    {
        asm volatile("" : : "v"(r.px), "v"(r.py), "v"(r.pz), "v"(r.c), "v"(r.ix), "v"(r.iy), "v"(r.iz), "v"(r.t) : "memory");
    }
    static __device__ __forceinline__ double x(const Raw& r) { return r.px; }
    static __device__ __forceinline__ double y(const Raw& r) { return r.py; }
    static __device__ __forceinline__ double z(const Raw& r) { return r.pz; }
    static __device__ __forceinline__ int tag(const Raw& r) { return r.t; }
};

// cavmd_params plus the two quotients the formulas need, divided once on the host (IEEE division is correctly rounded
// on host and device alike, so this changes no bit; it removes two ~150-cycle fp64 divisions from the prologue).
struct DeviceParams
{
    double g;    // couplstr
    double K;    // phmass * omegac^2
    double gK;   // g / K            (src/CavityForceCompute.cc:183)
    double g2K;  // g * g / K        (src/CavityForceCompute.cc:176)
};

// (host) the quotients of a checked cavmd_params, and the check
inline DeviceParams derive(const cavmd_params* p)
{
    DeviceParams d;
    d.g = p->couplstr;
    d.K = p->K;
    d.gK = p->couplstr / p->K;                   // as `m_params.couplstr / m_params.K`, src/CavityForceCompute.cc:183
    d.g2K = p->couplstr * p->couplstr / p->K;    // as `couplstr * couplstr / K`, :176 (host code is built -ffp-contract=off)
    return d;
}

inline bool params_ok(const cavmd_params* p)
{
    return p && isfinite(p->omegac) && isfinite(p->couplstr) && isfinite(p->K) && isfinite(p->phmass) && p->K != 0.0;
}

// The speculatively fetched last particle (the driver appends the photon last), as plain scalars: handing the
// layout's whole Raw aggregate through the prologue made hipcc keep it in a stack object (52 B of scratch stores per
// thread of every block of the fused force map: 1.19x its algorithmic HBM traffic at N = 1e6).
struct PhotonRow
{
    double x, y, z;
    int ix, iy, iz;
};
template <class Input>
__device__ __forceinline__ PhotonRow as_photon_row(const typename Input::Raw& r)
{
    PhotonRow p;
    p.x = Input::x(r); p.y = Input::y(r); p.z = Input::z(r);
    p.ix = r.ix; p.iy = r.iy; p.iz = r.iz;
    return p;
}
template <class Input>
__device__ __forceinline__ PhotonRow photon_row(const Input& in, size_t i)
{
    return as_photon_row<Input>(in.load(i));
}
// The speculative row, fetched at kernel entry: row N - 1 through VECTOR loads, TEMPORAL ones.
// Vector: the address is the same in every lane, and with a provably uniform address and __restrict__ const pointers the
// compiler fetches the row with scalar loads.  Those return out of order, so every wait on them is a full lgkmcnt(0): the wait
// for the last kernel arguments then also waits for this row -- an HBM miss with nothing else in flight, in front of the first
// tile load.  The zero below comes out of a vector register the compiler cannot see into, so the index does not look uniform;
// the loads go down the vector path, where they are older than every tile load, return in order ahead of them and cost the
// counted waits of the tile loop nothing.  The row is first read after the reduction, in scalars_from_total.
// Temporal: every wave of the grid asks for the same two lines at the same moment.  As non-temporal (streaming) loads those
// requests made the single-launch step 0.2 us SLOWER than the scalar loads had been; as temporal loads, which the caches
// keep, 0.3 us faster (profiles/early_first_load/README.md).
template <class Input>
__device__ __forceinline__ PhotonRow speculative_photon_row(const Input& in, unsigned N)
{
    unsigned opaque_zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opaque_zero));
    return as_photon_row<Input>(in.load_cached((size_t)(N - 1) + opaque_zero));
}

// Where the per-block partials live (SoA so the finalize kernel reads them coalesced).
struct Partials
{
    double* d;      // kNumPartDoubles arrays of `stride` doubles
    int* i;         // kNumPartInts arrays of `stride` ints
    unsigned stride;
};

// ---- kernel 1: per-block partial dipole sums + photon search --------------------------------------
// One tile = BLOCK * UNROLL particles; block b takes tiles b, b + grid, ...  A lane keeps the loads of UNROLL particle rows in
// flight and waits for one row at a time (accumulate_full_tiles below: the rolling loop), so that the ~57 VALU operations per
// particle overlap with the block's own loads even at one wave per SIMD.  (The earlier attempt at the same, whole tiles
// double-buffered behind a PIPE template parameter, was last present in commit 1906464: DESIGN.md 3.8, profiles/rolling_tile/.)
template <class Input, int UNROLL>
struct TileRegs
{
    typename Input::Raw raw[UNROLL];
};

template <class Input, int BLOCK, int UNROLL>
__device__ __forceinline__ void tile_load(const Input& in, size_t base, TileRegs<Input, UNROLL>& r)
{
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        r.raw[u] = in.load(base + (size_t)u * BLOCK);
}

template <class Input, int BLOCK, int UNROLL>
__device__ __forceinline__ void tile_accumulate(const TileRegs<Input, UNROLL>& r, size_t base, double Lx, double Ly,
                                                double Lz, int L_typeid, Accum& acc)
{
    bool isL[UNROLL];
    bool any = false;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
    {
        isL[u] = (Input::tag(r.raw[u]) == L_typeid);
        any = any || isL[u];
    }
    if (!__any(any))
    {
        // fast path (wave-uniform): no lane of this wave holds an L-typed particle in this tile
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const double c = r.raw[u].c;
            dd_acc(acc.hx, acc.lx, c * (Input::x(r.raw[u]) + (double)r.raw[u].ix * Lx));
            dd_acc(acc.hy, acc.ly, c * (Input::y(r.raw[u]) + (double)r.raw[u].iy * Ly));
            dd_acc(acc.hz, acc.lz, c * (Input::z(r.raw[u]) + (double)r.raw[u].iz * Lz));
        }
    }
    else
    {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const double rx = Input::x(r.raw[u]) + (double)r.raw[u].ix * Lx;
            const double ry = Input::y(r.raw[u]) + (double)r.raw[u].iy * Ly;
            const double rz = Input::z(r.raw[u]) + (double)r.raw[u].iz * Lz;
            acc.add((unsigned)(base + (size_t)u * BLOCK), rx, ry, rz, r.raw[u].c, Input::tag(r.raw[u]), L_typeid);
        }
    }
}

// One row of a tile: what tile_accumulate does for row u, with the fast-path test taken per row.  Same bits: for a lane whose
// particle is not L-typed Accum::add performs the same dd_acc(c * r) and only adds +0.0 to sx, sy, sz (never -0.0: they start at
// +0.0 and only grow by sums) and keeps lmin and lcnt.
template <class Input>
__device__ __forceinline__ void row_accumulate(const typename Input::Raw& r, size_t i, double Lx, double Ly, double Lz,
                                               int L_typeid, Accum& acc)
{
    if (!__any(Input::tag(r) == L_typeid))
    {
        const double c = r.c;
        dd_acc(acc.hx, acc.lx, c * (Input::x(r) + (double)r.ix * Lx));
        dd_acc(acc.hy, acc.ly, c * (Input::y(r) + (double)r.iy * Ly));
        dd_acc(acc.hz, acc.lz, c * (Input::z(r) + (double)r.iz * Lz));
    }
    else
    {
        const double rx = Input::x(r) + (double)r.ix * Lx;
        const double ry = Input::y(r) + (double)r.iy * Ly;
        const double rz = Input::z(r) + (double)r.iz * Lz;
        acc.add((unsigned)i, rx, ry, rz, r.c, Input::tag(r), L_typeid);
    }
}

// The full tiles of one block, accumulated in tile order, then row order: exactly the operations of
//     for k: tile_load(k); tile_accumulate(k)
// on every lane.  UNROLL >= 2: the rolling loop of cavmd_tile_schedule.hpp -- a wave waits for one row at a time and has the
// next tile's row on its way before it starts the arithmetic, at the plain loop's bytes in flight (a whole-tile double buffer
// holds two tiles in flight instead, which queued twice the bytes on the slowest paths and lost).  UNROLL == 1: a row is a tile,
// rolling would BE that double buffer, so the plain loop stays.  row_hook(k, u, charge) runs once per row, before its
// arithmetic (the single-launch kernel parks the charge in LDS; the reduction kernel does nothing).  first_issued() runs once,
// when the rows of the block's first tile have been issued and none has been consumed (not at all for a block without a full
// tile): the place to wait for kernel arguments that the loads themselves did not need.  The UNROLL == 1 loop has its first
// trip peeled for that; a test inside the loop would leave the wait in every trip, where the paths join.
struct NoFirstIssuedHook
{
    __device__ __forceinline__ void operator()() const {}
};
template <class Input, int BLOCK, int UNROLL, class RowHook, class FirstIssued>
__device__ __forceinline__ void accumulate_full_tiles(const Input& in, const TileSchedule& sch, double Lx, double Ly, double Lz,
                                                      int L_typeid, Accum& acc, RowHook&& row_hook, FirstIssued&& first_issued)
{
    if constexpr (UNROLL == 1)
    {
        const auto one_tile = [&](unsigned k, auto first) {
            const size_t base = tile_row_base(sch, k, 0, BLOCK) + threadIdx.x;
            TileRegs<Input, 1> A;
            tile_load<Input, BLOCK, 1>(in, base, A);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(first)::value)
            {
                CAVMD_PSTAMP(8);
                first_issued();
            }
            row_hook(k, 0, A.raw[0].c);
            tile_accumulate<Input, BLOCK, 1>(A, base, Lx, Ly, Lz, L_typeid, acc);
        };
        constexpr bool peel = !std::is_same_v<std::decay_t<FirstIssued>, NoFirstIssuedHook>; // nothing to run: the plain loop
        if (peel && sch.nfull)
            one_tile(0, std::true_type {});
        for (unsigned k = peel ? 1 : 0; k < sch.nfull; ++k)
            one_tile(k, std::false_type {});
    }
    else
    {
        TileRegs<Input, UNROLL> R[2];
        rolling_rows<UNROLL>(
            sch, BLOCK,
            [&](int set, int u, size_t base) {
                R[set].raw[u] = in.load(base + threadIdx.x);
                __builtin_amdgcn_sched_barrier(0); // the row's loads stay ahead of the arithmetic that follows
            },
            [&](int set, int u) {
                __builtin_amdgcn_sched_barrier(0); // nothing of the row before is sunk behind this wait
                Input::landed(R[set].raw[u]);
                __builtin_amdgcn_sched_barrier(0); // and the next row's loads are not hoisted above it
            },
            [&](int set, int u, unsigned k, size_t base) {
                row_hook(k, u, R[set].raw[u].c);
                row_accumulate<Input>(R[set].raw[u], base + threadIdx.x, Lx, Ly, Lz, L_typeid, acc);
            },
            first_issued);
    }
}

// The ragged tile of one block: the `count` (< BLOCK * UNROLL) particles from `tile_base` on, bounds-checked, added in row order
// after the full tiles.  row_hook(o, charge) runs once per row of every lane, o = the particle's offset within the tile, with
// charge 0 for a lane beyond the end (the single-launch kernel parks it in LDS; the reduction kernel does nothing).
template <class Input, int BLOCK, int UNROLL, class RowHook>
__device__ __forceinline__ void accumulate_ragged_tile(const Input& in, size_t tile_base, unsigned count, double Lx, double Ly,
                                                       double Lz, int L_typeid, Accum& acc, RowHook&& row_hook)
{
    const size_t base = tile_base + threadIdx.x;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
    {
        const unsigned o = u * BLOCK + threadIdx.x;
        double c = 0.0;
        if (o < count)
        {
            const size_t i = base + (size_t)u * BLOCK;
            const typename Input::Raw r = in.load(i);
            const double rx = Input::x(r) + (double)r.ix * Lx;
            const double ry = Input::y(r) + (double)r.iy * Ly;
            const double rz = Input::z(r) + (double)r.iz * Lz;
            acc.add((unsigned)i, rx, ry, rz, r.c, Input::tag(r), L_typeid);
            c = r.c;
        }
        row_hook(o, c);
    }
}

// The reduction of one block, G = the grid's size: the body of the two kernels below.  first_issued: see accumulate_full_tiles.
template <class Input, int BLOCK, int UNROLL, class FirstIssued>
__device__ __forceinline__ void dipole_partials_body(const Input& in, unsigned N, unsigned G, double Lx, double Ly, double Lz,
                                                     int L_typeid, const Partials& part, FirstIssued&& first_issued)
{
    constexpr unsigned TILE = BLOCK * UNROLL;
    Accum acc;
    const unsigned full_tiles = N / TILE;
    accumulate_full_tiles<Input, BLOCK, UNROLL>(in, strided_tiles(N, G, blockIdx.x, TILE), Lx, Ly, Lz, L_typeid, acc,
                                                [](unsigned, int, double) {}, first_issued);
    // ragged tail: one block takes it, bounds-checked (restates accumulate_ragged_tile: calling it moves instructions here)
    if (blockIdx.x == full_tiles % G)
    {
        const size_t base = (size_t)full_tiles * TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const size_t i = base + (size_t)u * BLOCK;
            if (i < N)
            {
                const typename Input::Raw r = in.load(i);
                const double rx = Input::x(r) + (double)r.ix * Lx;
                const double ry = Input::y(r) + (double)r.iy * Ly;
                const double rz = Input::z(r) + (double)r.iz * Lz;
                acc.add((unsigned)i, rx, ry, rz, r.c, Input::tag(r), L_typeid);
            }
        }
    }
    acc = block_reduce<BLOCK>(acc);
    if (threadIdx.x == 0)
    {
        const unsigned b = blockIdx.x, s = part.stride;
        part.d[0 * s + b] = acc.hx; part.d[1 * s + b] = acc.lx;
        part.d[2 * s + b] = acc.hy; part.d[3 * s + b] = acc.ly;
        part.d[4 * s + b] = acc.hz; part.d[5 * s + b] = acc.lz;
        part.d[6 * s + b] = acc.sx; part.d[7 * s + b] = acc.sy; part.d[8 * s + b] = acc.sz;
        part.i[0 * s + b] = acc.lmin;
        part.i[1 * s + b] = acc.lcnt;
    }
}

// any layout (the snapshot layout's reduction); the grid's size from the launch's hidden arguments
template <class Input, int BLOCK, int UNROLL>
__global__ __launch_bounds__(BLOCK) void dipole_partials_kernel(Input in, unsigned N, double Lx, double Ly, double Lz,
                                                                int L_typeid, Partials part)
{
    dipole_partials_body<Input, BLOCK, UNROLL>(in, N, gridDim.x, Lx, Ly, Lz, L_typeid, part, NoFirstIssuedHook {});
}

// HOOMD's AoS layout.  The kernel arguments in the order a block needs them, so that the first fourteen dwords (the three
// pointers, N, G, L_typeid and two of the box lengths) are handed over in registers at wave start (kernel-argument preload,
// csrc/Makefile: fourteen = the sixteen user SGPRs less the pointer to the argument block); G = the grid's size, an argument
// of its own: gridDim.x sits in the hidden arguments, behind the last explicit one, in a line of the argument block that
// nothing else here needs.  The rest (Lz, the partials' place) is fetched by scalar loads issued at entry and waited for once,
// when the first tile rows are on their way.
template <int NT, int BLOCK, int UNROLL>
__global__ __launch_bounds__(BLOCK) void dipole_partials_aos_kernel(const v2d* __restrict__ pos2,
                                                                    const double* __restrict__ charge,
                                                                    const int* __restrict__ image, unsigned N, unsigned G,
                                                                    int L_typeid, double Lx, double Ly, double Lz,
                                                                    Partials part)
{
    const AosInputT<NT> in {pos2, charge, image};
    dipole_partials_body<AosInputT<NT>, BLOCK, UNROLL>(in, N, G, Lx, Ly, Lz, L_typeid, part,
                                                       [&] { asm volatile("" : : "s"(Lz)); });
}

// ---- final reduction + scalars (shared by the stand-alone finalize kernel and the fused force map) ------------
// Everything an evaluation produces besides the per-particle forces, as held by thread 0 of a block.
struct Scalars
{
    double d[3], dlo[3], q[3], Dq[2], e[3], f[3], dtot[3];
    int photon, nL;
};

// From the block total (valid in thread 0) to everything else: renormalise, unwrap the photon and evaluate energies,
// Dq and the photon force with the reference's operator association (src/CavityForceCompute.cc:169-183, 203-207).
// `guess` is the speculatively fetched last particle (the driver appends the photon last).
template <class Input>
__device__ __forceinline__ Scalars scalars_from_total(Accum acc, const PhotonRow guess, const Input& in,
                                                      unsigned N, double Lx, double Ly, double Lz,
                                                      const DeviceParams& prm, bool want_energies)
{
    Scalars sc;
    // `want_energies` marks the one block that publishes cavmd_result: only it needs d_z, the all-particle dipole and the
    // energies; every other block is on its way to the force map and needs Dq and F_L only.
    dd_norm(acc.hx, acc.lx);
    dd_norm(acc.hy, acc.ly);
    if (want_energies)
        dd_norm(acc.hz, acc.lz);
    double dx = acc.hx, dy = acc.hy, dz = acc.hz;
    sc.dtot[0] = sc.dtot[1] = sc.dtot[2] = 0.0;
    if (want_energies)
    {
        // all particles, L-typed included (the photon normally has charge 0, so this usually equals d): the L-typed sum
        // joins the double-double BEFORE the final rounding, so the low word is not thrown away when the two terms cancel
        double th = acc.hx, tl = acc.lx;
        dd_acc(th, tl, acc.sx);
        sc.dtot[0] = th + tl;
        th = acc.hy; tl = acc.ly;
        dd_acc(th, tl, acc.sy);
        sc.dtot[1] = th + tl;
        th = acc.hz; tl = acc.lz;
        dd_acc(th, tl, acc.sz);
        sc.dtot[2] = th + tl;
    }
    const int photon = (acc.lmin == INT_MAX) ? -1 : acc.lmin;
    const double g = prm.g, K = prm.K;
    double qx = 0.0, qy = 0.0, qz = 0.0, eh = 0.0, ec = 0.0, ed = 0.0, Dqx = 0.0, Dqy = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    if (threadIdx.x == 0)
    {
        if (photon >= 0)
        {
            // field-by-field select between the speculative row and the fallback load
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
            {
                // Degenerate input (the driver enforces exactly one 'L', examples/05_advanced_run.py:548-550): the
                // reference skips only the FIRST L-typed particle in the dipole (src/CavityForceCompute.cc:122), so
                // the later ones are added back here.  (Rare: the photon's charge is fetched here, not speculatively.)
                const double pc = in.load((size_t)photon).c;
                dx += acc.sx - pc * qx;
                dy += acc.sy - pc * qy;
                dz += acc.sz - pc * qz;
            }
            if (want_energies)
            {
                // src/CavityForceCompute.cc:174-176, dot() = a.x*b.x + a.y*b.y + a.z*b.z
                eh = 0.5 * K * (qx * qx + qy * qy + qz * qz);
                ec = g * (dx * qx + dy * qy + 0.0 * 0.0);
                ed = 0.5 * prm.g2K * (dx * dx + dy * dy + 0.0 * 0.0);
            }
            // :183
            Dqx = qx + prm.gK * dx;
            Dqy = qy + prm.gK * dy;
            // :203-207
            fx = -K * qx - g * dx;
            fy = -K * qy - g * dy;
            fz = -K * qz - g * 0.0;
        }
        else
        {
            // no photon: the reference zeroes energies and returns before it computes a dipole (:148-156)
            dx = dy = dz = 0.0;
            acc.lx = acc.ly = acc.lz = 0.0;
        }
    }
    CAVMD_STAMP(4);
    sc.d[0] = dx; sc.d[1] = dy; sc.d[2] = dz;
    sc.dlo[0] = acc.lx; sc.dlo[1] = acc.ly; sc.dlo[2] = acc.lz;
    sc.q[0] = qx; sc.q[1] = qy; sc.q[2] = qz;
    sc.Dq[0] = Dqx; sc.Dq[1] = Dqy;
    sc.e[0] = eh; sc.e[1] = ec; sc.e[2] = ed;
    sc.f[0] = fx; sc.f[1] = fy; sc.f[2] = fz;
    sc.photon = photon;
    sc.nL = acc.lcnt;
    return sc;
}

// Folds the `nparts` per-block partials in a FIXED order (thread t takes partials t, t+BLOCK, ... in index order,
// then the fixed-shape block tree), unwraps the photon and evaluates energies, Dq and the photon force with the
// reference's operator association (src/CavityForceCompute.cc:169-183, 203-207).  All threads of the block must
// call it; the result is valid in thread 0 only.  Any block that calls it with the same arguments gets the same
// bits, which is what lets every block of the fused force map redo it instead of waiting on a separate launch.
template <class Input, int BLOCK>
__device__ __forceinline__ Scalars reduce_partials_and_finalize(const Input& in, unsigned N, unsigned nparts, double Lx,
                                                                double Ly, double Lz, const DeviceParams& prm,
                                                                const Partials& part, bool want_energies)
{
    // Speculative fetch of the last particle: the driver appends the photon last (examples/05_advanced_run.py:
    // 497-505), so this usually removes a dependent memory round trip after the reduction.  Vector loads, in flight together
    // with the partials' loads below (as scalar loads the row was two serial misses ahead of them).
    CAVMD_STAMP(0);
    const PhotonRow guess = speculative_photon_row(in, N);

    Accum acc;
    const unsigned s = part.stride;
    constexpr int BATCH = 4; // partial sets in flight per thread
    for (unsigned base = 0; base < nparts; base += BATCH * BLOCK)
    {
        Accum o[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j)
        {
            const unsigned p = base + j * BLOCK + threadIdx.x;
            if (p < nparts)
            {
                o[j].hx = part.d[0 * s + p]; o[j].lx = part.d[1 * s + p];
                o[j].hy = part.d[2 * s + p]; o[j].ly = part.d[3 * s + p];
                o[j].hz = part.d[4 * s + p]; o[j].lz = part.d[5 * s + p];
                o[j].sx = part.d[6 * s + p]; o[j].sy = part.d[7 * s + p]; o[j].sz = part.d[8 * s + p];
                o[j].lmin = part.i[0 * s + p];
                o[j].lcnt = part.i[1 * s + p];
            }
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j)
            if (base + j * BLOCK < nparts) // block-uniform: skip batches nobody loaded
                acc.merge(o[j]);           // (a default-constructed Accum is the identity for the ragged last one)
    }
    CAVMD_STAMP(1);
    if (BLOCK == 256 && nparts <= 256)
    {
        // Two-level fold, the same tree the single-launch kernel walks across workgroups (cavmd_persistent_kernel.hpp):
        // 16 consecutive partials -> group total (one DPP row each), then the <= 16 group totals.
        __shared__ double s_gd[16][kNumPartDoubles];
        __shared__ int s_gi[16][kNumPartInts];
        acc = row_fold16(acc);
        CAVMD_STAMP(2);
        if ((threadIdx.x & 15) == 0)
        {
            const int gidx = threadIdx.x >> 4;
            s_gd[gidx][0] = acc.hx; s_gd[gidx][1] = acc.lx; s_gd[gidx][2] = acc.hy; s_gd[gidx][3] = acc.ly;
            s_gd[gidx][4] = acc.hz; s_gd[gidx][5] = acc.lz; s_gd[gidx][6] = acc.sx; s_gd[gidx][7] = acc.sy;
            s_gd[gidx][8] = acc.sz;
            s_gi[gidx][0] = acc.lmin;
            s_gi[gidx][1] = acc.lcnt;
        }
        __syncthreads();
        if (threadIdx.x < kWave)
        {
            Accum o;
            if (threadIdx.x < (nparts + 15) / 16)
            {
                const int gidx = threadIdx.x;
                o.hx = s_gd[gidx][0]; o.lx = s_gd[gidx][1]; o.hy = s_gd[gidx][2]; o.ly = s_gd[gidx][3];
                o.hz = s_gd[gidx][4]; o.lz = s_gd[gidx][5]; o.sx = s_gd[gidx][6]; o.sy = s_gd[gidx][7];
                o.sz = s_gd[gidx][8];
                o.lmin = s_gi[gidx][0];
                o.lcnt = s_gi[gidx][1];
            }
            Accum t;
            t.merge(o);
            acc = row_fold16(t);
        }
        CAVMD_STAMP(3);
    }
    else
        acc = block_reduce<BLOCK>(acc);
    return scalars_from_total<Input>(acc, guess, in, N, Lx, Ly, Lz, prm, want_energies);
}

__device__ __forceinline__ void write_result(cavmd_result* __restrict__ res, const Scalars& sc, unsigned N,
                                             unsigned nparts, uint64_t sequence)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        res->dipole[k] = sc.d[k];
        res->q[k] = sc.q[k];
        res->energy[k] = sc.e[k];
        res->photon_force[k] = sc.f[k];
        res->dipole_lo[k] = sc.dlo[k];
        res->total_dipole[k] = sc.dtot[k];
    }
    res->Dq[0] = sc.Dq[0];
    res->Dq[1] = sc.Dq[1];
    res->photon_idx = sc.photon;
    res->n_photon_typed = sc.nL;
    res->n_particles = N;
    res->n_partials = nparts;
    res->sequence = sequence;
    res->reserved = 0.0;
}

// Host hand-off of the result block: `host` points at mapped pinned host memory.  The block is written first, then the
// evaluation's sequence number is release-stored at SYSTEM scope into host->ready, so a host thread that acquires
// ready == sequence sees the whole block (cavmd_result_read spins on it instead of paying a stream synchronisation).
// The workspace keeps a ring of these (one slot per evaluation, sequence % depth: cavmd_result_at), padded to 256 bytes so
// that two slots never share a line.
struct HostResult
{
    cavmd_result result;
    uint64_t ready;
    uint64_t failed; // single-launch kernel, starved evaluation that could not be completed: (sequence << 2) | kSyncFailed,
                     // tagged so that a stale word of an earlier occupant of the slot never names a later evaluation
    unsigned char pad[48];
};
static_assert(sizeof(HostResult) == 256, "one result slot = 256 bytes");
__device__ __forceinline__ void publish_to_host(HostResult* __restrict__ host, const Scalars& sc, unsigned N,
                                                unsigned nparts, uint64_t sequence)
{
    write_result(&host->result, sc, N, nparts, sequence);
    __hip_atomic_store(&host->ready, sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- kernel 2 (three-launch path): one block publishes the result block ---------------------------------------
template <class Input, int BLOCK>
__global__ __launch_bounds__(BLOCK) void finalize_kernel(Input in, unsigned N, unsigned nparts, double Lx, double Ly,
                                                         double Lz, DeviceParams prm, Partials part, uint64_t sequence,
                                                         cavmd_result* __restrict__ res, HostResult* __restrict__ res_host)
{
    const Scalars sc = reduce_partials_and_finalize<Input, BLOCK>(in, N, nparts, Lx, Ly, Lz, prm, part, true);
    if (threadIdx.x == 0)
    {
        write_result(res, sc, N, nparts, sequence);
        publish_to_host(res_host, sc, N, nparts, sequence);
    }
}

// ---- force map, HOOMD AoS force array written as dense 16-byte chunks ------------------------------------------
// Store policy of the force array: 0 plain (write-back), 1 non-temporal, 2 write-through (sc1: the bytes leave the XCD's L2
// while the kernel runs instead of at its end-of-kernel release; after 320 MB of non-temporal stores at N = 1e7 the next
// kernel in the stream started 8.7 us late).
template <int NT>
__device__ __forceinline__ void store_chunk(v2d* p, v2d v)
{
    if (NT == 2)
    {
        // The hardware reads the data registers of a store wider than 64 bits up to two wait states after issue.  hipcc pads
        // its own stores but does not look into an asm statement, and may write v's registers in the very next
        // instruction: the pad (s_nop 1 = two wait states) ends the string.
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
    }
    else if (NT == 1)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// What every thread of the force map needs to know about the evaluation.
struct MapScalars
{
    double Dqx, Dqy, Fx, Fy, Fz;
    int photon, nL;
};

// thread 0's Scalars -> LDS (s_m: 5 doubles, s_mi: 2 ints), and after the block's barrier every thread's MapScalars from there
__device__ __forceinline__ void park_scalars(double* s_m, int* s_mi, const Scalars& sc)
{
    s_m[0] = sc.Dq[0]; s_m[1] = sc.Dq[1]; s_m[2] = sc.f[0]; s_m[3] = sc.f[1]; s_m[4] = sc.f[2];
    s_mi[0] = sc.photon;
    s_mi[1] = sc.nL;
}
__device__ __forceinline__ MapScalars map_scalars_from_lds(const double* s_m, const int* s_mi)
{
    MapScalars m;
    m.Dqx = s_m[0]; m.Dqy = s_m[1]; m.Fx = s_m[2]; m.Fy = s_m[3]; m.Fz = s_m[4];
    m.photon = s_mi[0];
    m.nL = s_mi[1];
    return m;
}

// The force-chunk rule.  Chunk k is 16 bytes: particle k >> 1, half k & 1 (`odd`); c is the particle's charge, ng = -g and
// pchunk the photon's first chunk.  Even chunk = (Fx, Fy) = ((-g c) Dq_x, (-g c) Dq_y), odd chunk = (Fz, w) = (0, 0); the
// photon's chunks carry F_L.  With several L-typed particles (degenerate) the reference gives a molecular force only to particles
// whose type is not L (src/CavityForceCompute.cc:190-191): the sibling takes the particle's type tag.
__device__ __forceinline__ v2d force_chunk(const MapScalars& m, double ng, double c, size_t k, bool odd, size_t pchunk)
{
    const v2d zero = {0.0, 0.0};
    const double s = ng * c; // ((-g) * charge) * Dq, src/CavityForceCompute.cc:194
    v2d v = {s * m.Dqx, s * m.Dqy};
    v = odd ? zero : v;
    if ((k | 1) == (pchunk | 1))
        v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
    return v;
}
__device__ __forceinline__ v2d force_chunk_typed(const MapScalars& m, double ng, double c, size_t k, bool odd, size_t pchunk,
                                                 int tag, int L_typeid)
{
    const v2d zero = {0.0, 0.0};
    const double s = ng * c;
    v2d v = {s * m.Dqx, s * m.Dqy};
    v = (odd || tag == L_typeid) ? zero : v;
    if ((k | 1) == (pchunk | 1))
        v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
    return v;
}

// Body shared by the three-launch and the fused force map.  Its three chunk sites keep their own text of the rule above:
// routed through force_chunk the compiler folds the photon test differently (profiles/single_launch_cleanup/README.md).
// PRE: the caller has already loaded the charges of this block's first full tile into c_first (issued before its
// prologue so that their latency is hidden behind it).  G: the grid's size.
template <int BLOCK, int UNROLL, int NT, bool PRE>
__device__ __forceinline__ void force_map_body(const MapScalars m, const double* __restrict__ charge,
                                               const v2d* __restrict__ pos2, unsigned N, double g, int L_typeid,
                                               v2d* __restrict__ force2, const double (&c_first)[UNROLL], unsigned G,
                                               bool reverse = false)
{
    constexpr unsigned TILE = BLOCK * UNROLL;
    const double ng = -g;
    const size_t nchunks = 2 * (size_t)N;
    const size_t pchunk = m.photon >= 0 ? 2 * (size_t)m.photon : ~(size_t)0; // photon's first chunk
    const unsigned full_tiles = (unsigned)(nchunks / TILE);
    const bool odd = threadIdx.x & 1; // BLOCK and TILE are even, so the half is fixed per thread
    const v2d zero = {0.0, 0.0};

    if (m.photon < 0)
    {
        // no photon: all forces are zero (src/CavityForceCompute.cc:145-156)
        for (size_t k = (size_t)blockIdx.x * BLOCK + threadIdx.x; k < nchunks; k += (size_t)G * BLOCK)
            store_chunk<NT>(force2 + k, zero);
        return;
    }

    if (m.nL <= 1)
    {
        // Tiles blockIdx.x, blockIdx.x + grid, ...; `reverse` walks the same tiles from the last to the first, so that
        // the charge lines the reduction touched most recently (same XCD, see cavmd_capi.hip) are asked for first.
        const unsigned count = blockIdx.x < full_tiles ? (full_tiles - blockIdx.x + G - 1) / G : 0;
        for (unsigned j = 0; j < count; ++j)
        {
            const unsigned t = blockIdx.x + (reverse ? count - 1 - j : j) * G;
            const size_t base = (size_t)t * TILE + threadIdx.x;
            double c[UNROLL];
            if (PRE && j == 0)
            {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    c[u] = c_first[u];
            }
            else
            {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    c[u] = charge[(base + (size_t)u * BLOCK) >> 1];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const size_t k = base + (size_t)u * BLOCK;
                const double s = ng * c[u]; // restates force_chunk (calling it changes this kernel's instructions)
                v2d v = {s * m.Dqx, s * m.Dqy};
                v = odd ? zero : v;
                if ((k | 1) == (pchunk | 1))
                    v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
                store_chunk<NT>(force2 + k, v);
            }
        }
        if (blockIdx.x == full_tiles % G)
        {
            const size_t base = (size_t)full_tiles * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const size_t k = base + (size_t)u * BLOCK;
                if (k < nchunks)
                {
                    const double s = ng * charge[k >> 1]; // restates force_chunk
                    v2d v = {s * m.Dqx, s * m.Dqy};
                    v = odd ? zero : v;
                    if ((k | 1) == (pchunk | 1))
                        v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
                    store_chunk<NT>(force2 + k, v);
                }
            }
        }
        return;
    }

    // Several L-typed particles (degenerate): the reference gives a molecular force only to particles
    // whose type is not L (src/CavityForceCompute.cc:190-191), so the type tag has to be read.
    for (size_t k = (size_t)blockIdx.x * BLOCK + threadIdx.x; k < nchunks; k += (size_t)G * BLOCK)
    {
        const size_t p = k >> 1;
        const int tag = __double2loint(pos2[2 * p + 1].y);
        const double s = ng * charge[p]; // restates force_chunk_typed
        v2d v = {s * m.Dqx, s * m.Dqy};
        v = (odd || tag == L_typeid) ? zero : v;
        if ((k | 1) == (pchunk | 1))
            v = odd ? (v2d) {m.Fz, 0.0} : (v2d) {m.Fx, m.Fy};
        store_chunk<NT>(force2 + k, v);
    }
}

// three-launch path: scalars come from the result block the finalize kernel wrote
template <int BLOCK, int UNROLL, int NT>
__global__ __launch_bounds__(BLOCK) void force_map_aos_kernel(const double* __restrict__ charge,
                                                              const v2d* __restrict__ pos2, // only read if several L-typed
                                                              unsigned N, double g, int L_typeid,
                                                              const cavmd_result* __restrict__ res, v2d* __restrict__ force2)
{
    MapScalars m;
    m.Dqx = res->Dq[0]; m.Dqy = res->Dq[1];
    m.Fx = res->photon_force[0]; m.Fy = res->photon_force[1]; m.Fz = res->photon_force[2];
    m.photon = res->photon_idx;
    m.nL = res->n_photon_typed;
    const double none[UNROLL] = {};
    force_map_body<BLOCK, UNROLL, NT, false>(m, charge, pos2, N, g, L_typeid, force2, none, gridDim.x);
}

// two-launch path: every block folds the partials itself (same fixed order -> same bits in every block), block 0
// publishes the result block; no separate finalize launch and no inter-workgroup hand-off inside the launch.
// The first fourteen dwords of the argument block are what the prologue needs for the loads it issues first (the first tile's
// charges, the speculative row) and all but the stride of what the partials' loads need, for the kernel-argument preload
// (dipole_partials_aos_kernel above); G = the grid's size, reverse as an int.
template <int BLOCK, int UNROLL, int NT>
__global__ __launch_bounds__(BLOCK) void force_map_aos_fused_kernel(const v2d* __restrict__ pos2,
                                                                    const double* __restrict__ charge,
                                                                    const int* __restrict__ image, double* part_d, int* part_i,
                                                                    unsigned N, unsigned G, int reverse, unsigned nparts,
                                                                    unsigned part_stride, int L_typeid, double Lx, double Ly,
                                                                    double Lz, DeviceParams prm, uint64_t sequence,
                                                                    cavmd_result* __restrict__ res,
                                                                    HostResult* __restrict__ res_host,
                                                                    v2d* __restrict__ force2)
{
    __shared__ double s_m[5];
    __shared__ int s_mi[2];
    const AosInput in {pos2, charge, image};
    const Partials part {part_d, part_i, part_stride};
    // charges of the first tile: independent of the prologue, so issue them first
    double c_first[UNROLL] = {};
    {
        constexpr unsigned TILE = BLOCK * UNROLL;
        const unsigned full_tiles = (unsigned)((2 * (size_t)N) / TILE);
        if (blockIdx.x < full_tiles)
        {
            const unsigned count = (full_tiles - blockIdx.x + G - 1) / G;
            const unsigned t0 = blockIdx.x + (reverse ? count - 1 : 0) * G;
            const size_t base = (size_t)t0 * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                c_first[u] = in.charge[(base + (size_t)u * BLOCK) >> 1];
        }
    }
    const Scalars sc = reduce_partials_and_finalize<AosInput, BLOCK>(in, N, nparts, Lx, Ly, Lz, prm, part, blockIdx.x == 0);
    if (threadIdx.x == 0)
    {
        park_scalars(s_m, s_mi, sc);
        if (blockIdx.x == 0)
        {
            write_result(res, sc, N, nparts, sequence);
            publish_to_host(res_host, sc, N, nparts, sequence);
        }
    }
    __syncthreads();
    const MapScalars m = map_scalars_from_lds(s_m, s_mi);
    force_map_body<BLOCK, UNROLL, NT, true>(m, in.charge, in.pos2, N, prm.g, L_typeid, force2, c_first, G, reverse != 0);
}

constexpr int kSmallSystemLdsCharges = 4096; // charges the single-block kernel keeps in LDS (32 KB); beyond: re-read

// ---- small systems: ONE block, ONE launch ----------------------------------------------------------------------
// The reference's production system is N = 501 (examples/init-0.gsd, 500 SLURM replicas of it).  At that size two
// launches are pure latency (~4 us each); a single block that reduces, finalises and maps in one go halves it.  Used
// below kSmallSystemMaxN particles, where one CU's bandwidth is not yet the limit.
constexpr int kSmallBlock = 256; // the block size both the workspace and the batch launch this body with: the two paths share bits
// (the arguments the loads need lead the argument block, for the kernel-argument preload: dipole_partials_aos_kernel above)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cavity_small_system_kernel(const v2d* __restrict__ pos2,
                                                                    const double* __restrict__ charge,
                                                                    const int* __restrict__ image, unsigned N, int L_typeid,
                                                                    double Lx, double Ly, double Lz, DeviceParams prm,
                                                                    uint64_t sequence, cavmd_result* __restrict__ res,
                                                                    HostResult* __restrict__ res_host,
                                                                    v2d* __restrict__ force2)
{
    const AosInput in {pos2, charge, image};
#include "cavmd_small_system_body.hpp" // the body, shared as text with cavity_batch_kernel
}

// ---- force map for the snapshot layout (strided (N,3) force + optional potential energy) ------------------------
// One particle per lane; UNROLL charges are loaded before the stores.  When the force rows are packed (stride 24) a
// wave's 64 rows are one contiguous 1.5 KB run, so the three 8-byte stores per lane still fill whole lines.
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void force_map_strided_body(const MapScalars m, const StridedInput& in, unsigned N, double g,
                                                       int L_typeid, char* __restrict__ force, size_t force_stride,
                                                       char* __restrict__ pe, size_t pe_stride)
{
    const double ng = -g;
    constexpr size_t TILE = (size_t)BLOCK * UNROLL;
    const size_t tiles = ((size_t)N + TILE - 1) / TILE;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x)
    {
        const size_t base = t * TILE + threadIdx.x;
        double c[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const size_t i = base + (size_t)u * BLOCK;
            c[u] = (m.photon >= 0 && i < N) ? *reinterpret_cast<const double*>(in.chg + i * in.chg_stride) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            const size_t i = base + (size_t)u * BLOCK;
            if (i >= N)
                continue;
            double fx = 0.0, fy = 0.0, fz = 0.0;
            if (m.photon >= 0)
            {
                const double s = ng * c[u]; // ((-g) * charge) * Dq, src/CavityForceCompute.cc:194
                fx = s * m.Dqx;
                fy = s * m.Dqy;
                if (m.nL > 1 && *reinterpret_cast<const int*>(in.tid + i * in.tid_stride) == L_typeid)
                {
                    fx = 0.0;
                    fy = 0.0;
                }
                if ((int)i == m.photon)
                {
                    fx = m.Fx;
                    fy = m.Fy;
                    fz = m.Fz;
                }
            }
            double* f = reinterpret_cast<double*>(force + i * force_stride);
            __builtin_nontemporal_store(fx, f + 0);
            __builtin_nontemporal_store(fy, f + 1);
            __builtin_nontemporal_store(fz, f + 2);
            if (pe)
                __builtin_nontemporal_store(0.0, reinterpret_cast<double*>(pe + i * pe_stride));
        }
    }
}

// three-launch variant (scalars from the result block)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void force_map_strided_kernel(StridedInput in, unsigned N, double g, int L_typeid,
                                                                  const cavmd_result* __restrict__ res,
                                                                  char* __restrict__ force, size_t force_stride,
                                                                  char* __restrict__ pe, size_t pe_stride)
{
    MapScalars m;
    m.Dqx = res->Dq[0]; m.Dqy = res->Dq[1];
    m.Fx = res->photon_force[0]; m.Fy = res->photon_force[1]; m.Fz = res->photon_force[2];
    m.photon = res->photon_idx;
    m.nL = res->n_photon_typed;
    force_map_strided_body<BLOCK, 4>(m, in, N, g, L_typeid, force, force_stride, pe, pe_stride);
}

// two-launch variant: the same prologue as force_map_aos_fused_kernel
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void force_map_strided_fused_kernel(StridedInput in, unsigned N, unsigned nparts,
                                                                        double Lx, double Ly, double Lz, DeviceParams prm,
                                                                        int L_typeid, Partials part, uint64_t sequence,
                                                                        cavmd_result* __restrict__ res,
                                                                        HostResult* __restrict__ res_host,
                                                                        char* __restrict__ force, size_t force_stride,
                                                                        char* __restrict__ pe, size_t pe_stride)
{
    __shared__ double s_m[5];
    __shared__ int s_mi[2];
    const Scalars sc = reduce_partials_and_finalize<StridedInput, BLOCK>(in, N, nparts, Lx, Ly, Lz, prm, part,
                                                                         blockIdx.x == 0);
    if (threadIdx.x == 0)
    {
        park_scalars(s_m, s_mi, sc);
        if (blockIdx.x == 0)
        {
            write_result(res, sc, N, nparts, sequence);
            publish_to_host(res_host, sc, N, nparts, sequence);
        }
    }
    __syncthreads();
    const MapScalars m = map_scalars_from_lds(s_m, s_mi);
    force_map_strided_body<BLOCK, 4>(m, in, N, prm.g, L_typeid, force, force_stride, pe, pe_stride);
}

} // namespace cavmd
