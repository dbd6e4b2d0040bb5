// cavmd_small_system_body.hpp -- the whole evaluation of ONE small system by ONE workgroup, as program text.
//
// NOT a stand-alone header: it is included INSIDE the body of cavity_small_system_kernel (cavmd_force_kernels.hpp) and of
// cavity_batch_kernel (cavmd_batch_kernel.hpp), which both provide, under these names,
//     AosInput in; unsigned N (>= 1); double Lx, Ly, Lz; DeviceParams prm; int L_typeid; uint64_t sequence;
//     cavmd_result* __restrict__ res; HostResult* __restrict__ res_host; v2d* __restrict__ force2;   and BLOCK.
// One text, hence the same arithmetic and the same bits on both paths.  It is shared as text and not as a function on
// purpose: wrapped into a __forceinline__ function, the single-system kernel compiled to different code (other loop
// structure after inlining) and measured 3.4 % slower on the MI355X; included, its code is unchanged, instruction for
// instruction (profiles/r05/isa_batch_kernel.txt).
    __shared__ double s_m[5];
    __shared__ int s_mi[2];
    __shared__ double s_c[kSmallSystemLdsCharges]; // the charges, for the force phase (no second trip to global memory)
    const PhotonRow guess = photon_row(in, (size_t)(N - 1));
    Accum acc;
    constexpr int BATCH = 4; // particles in flight per lane
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
            {
                acc.add(i, rx, ry, rz, r[j].c, AosInput::tag(r[j]), L_typeid);
                if (i < (unsigned)kSmallSystemLdsCharges)
                    s_c[i] = r[j].c;
            }
        }
    }
    acc = block_reduce<BLOCK>(acc);
    const Scalars sc = scalars_from_total<AosInput>(acc, guess, in, N, Lx, Ly, Lz, prm, true);
    if (threadIdx.x == 0)
    {
        s_m[0] = sc.Dq[0]; s_m[1] = sc.Dq[1]; s_m[2] = sc.f[0]; s_m[3] = sc.f[1]; s_m[4] = sc.f[2];
        s_mi[0] = sc.photon;
        s_mi[1] = sc.nL;
    }
    __syncthreads();
    const double Dqx = s_m[0], Dqy = s_m[1], Fx = s_m[2], Fy = s_m[3], Fz = s_m[4];
    const int photon = s_mi[0], nL = s_mi[1];
    const double ng = -prm.g;
    const unsigned nchunks = 2 * N;
    const bool odd = threadIdx.x & 1;
    const v2d zero = {0.0, 0.0};
    for (unsigned k = threadIdx.x; k < nchunks; k += BLOCK)
    {
        const unsigned p = k >> 1;
        v2d v = zero;
        if (photon >= 0)
        {
            const double c = p < (unsigned)kSmallSystemLdsCharges ? s_c[p] : in.charge[p];
            const double sgc = ng * c; // ((-g) * charge) * Dq, src/CavityForceCompute.cc:194
            v = (v2d) {sgc * Dqx, sgc * Dqy};
            const bool typed_L = (nL > 1) && (__double2loint(in.pos2[2 * p + 1].y) == L_typeid);
            v = (odd || typed_L) ? zero : v;
            if ((int)p == photon)
                v = odd ? (v2d) {Fz, 0.0} : (v2d) {Fx, Fy};
        }
        force2[k] = v;
    }
    // The result goes to the host AFTER the force stores have been issued: its system-scope release (~0.6 us) then overlaps
    // their drain instead of standing in front of them.
    if (threadIdx.x == 0)
    {
        write_result(res, sc, N, 1u, sequence);
        publish_to_host(res_host, sc, N, 1u, sequence);
    }
