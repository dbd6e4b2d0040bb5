// cavmd_coulomb_force_body.inc -- the body of launch 2 of both reciprocal-space methods: coulomb_force_kernel
// (cavmd_coulomb_batch_kernel.hpp) and ewald_force_factored_kernel (cavmd_ewald_factored_kernel.hpp), included into each.  It is
// the text of a kernel and not a function the two call: as functions, inlined, the shared parts changed the code of the kernel
// that was there before the factored method, whose device code stays what it was.  In scope: BLOCK, S, FACTORED (a constant
// expression), PART, rows, hdr, lds_n, and for FACTORED: SEG, lds_m and what cavmd_ewald_factored_kernel.hpp declares (the direct
// kernel declares SEG and lds_m as constants that nothing reads).
//
// The real-space walk, the fold, the self and background terms and the stores are the same text for both.  FACTORED: the
// workgroup table and the item's segments come from the tables behind hdr->pad[0], the guard also refuses a system whose M
// the launch has no LDS for, and the walk over k takes cos theta and sin theta from the particle's per-axis tables, which are
// written over the LDS image once every lane is done with it.
//
// PART (a constant expression, cavmd_coulomb_batch_kernel.hpp) selects the terms.  kCoulombPartAll: everything, into
// row->force2 -- the two kernels of cavmd_coulomb_compute, whose device code the `if constexpr` branches below leave what it
// was.  kCoulombPartShort (never FACTORED): the real-space terms of the pairs that are no exclusion partners and lie inside
// the cut-off, into row->force2; no Q, no walk over k, no self or background term.  kCoulombPartLong: the erf terms of the
// exclusion partners, Q, the walk over k, the self and background terms and the {Q, 0} slot, into the array row->pad names.
    extern __shared__ __attribute__((aligned(16))) unsigned char s_coulomb[];
    uint4 blk;
    [[maybe_unused]] unsigned seg_first = 0, seg_count = 0, Mx = 0, My = 0, Mz = 0;
    if constexpr (FACTORED)
    {
        if (blockIdx.x >= (unsigned)(hdr->pad[1] >> 32))
            return; // a launch captured for a larger table
        const uint4* __restrict__ ewald = reinterpret_cast<const uint4*>(hdr->pad[0]);
        const uint4 top = ewald[0];
        blk = ewald[(size_t)top.y + blockIdx.x];
        const uint4 info = ewald[(size_t)top.z + __builtin_amdgcn_readfirstlane(blk.x)];
        seg_first = __builtin_amdgcn_readfirstlane(info.x);
        seg_count = __builtin_amdgcn_readfirstlane(info.y);
        Mx = __builtin_amdgcn_readfirstlane(info.z) & 0xFFFFu;
        My = __builtin_amdgcn_readfirstlane(info.z) >> 16;
        Mz = __builtin_amdgcn_readfirstlane(info.w);
    }
    else
    {
        if (blockIdx.x >= hdr->n_blocks)
            return; // a launch captured for a larger table
        blk = hdr->blocks[blockIdx.x];
    }
    const unsigned item = __builtin_amdgcn_readfirstlane(blk.x);
    const unsigned first = __builtin_amdgcn_readfirstlane(blk.y);
    const unsigned partner_base = __builtin_amdgcn_readfirstlane(blk.z);
    const unsigned k_base = __builtin_amdgcn_readfirstlane(blk.w);
    const CoulombRow* __restrict__ row = rows + item;
    const unsigned n = row->n, n_k = row->n_k;
    v2d* __restrict__ force2 = row->force2;
    if constexpr (PART == kCoulombPartLong)
    {
        force2 = reinterpret_cast<v2d*>(row->pad);
        if (!force2)
            return; // a launch captured before the long arrays were dropped
    }
    const unsigned r = threadIdx.x / S, s = threadIdx.x % S;
    const unsigned i = first + r;
    const bool owner = (i < n);
    bool beyond = (n > lds_n);
    if constexpr (FACTORED)
        beyond = beyond || Mx > lds_m || My > lds_m || Mz > lds_m;
    if (beyond)
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
    double* __restrict__ sx = reinterpret_cast<double*>(s_coulomb);
    double* __restrict__ sy = sx + lds_n;
    double* __restrict__ sz = sy + lds_n;
    double* __restrict__ sq = sz + lds_n;
    coulomb_stage<BLOCK>(row, n, sx, sy, sz, sq);

    const double Lx = row->Lx, Ly = row->Ly, Lz = row->Lz;
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5;
    const double kappa = row->kappa, rcutsq = row->rcutsq;
    const double two_self_c = 2.0 * row->self_c; // 2 kappa / sqrt(pi)
    const unsigned ii = owner ? i : 0u;          // lanes past the end walk nothing and write nothing, but take part in the shuffles
    const double xi = sx[ii], yi = sy[ii], zi = sz[ii], qi = sq[ii];
    uint4 slots = {kCoulombNoPartner, kCoulombNoPartner, kCoulombNoPartner, kCoulombNoPartner};
    if (owner)
        slots = hdr->partners[(size_t)partner_base + i];

    // real space: partial s of particle i, and of the total charge
    double px = 0.0, py = 0.0, pz = 0.0, pw = 0.0, pq = 0.0;
    const unsigned j_end = owner ? n : 0u;
    for (unsigned j = s; j < j_end; j += S)
    {
        const double qj = sq[j];
        if constexpr (PART != kCoulombPartShort)
            pq = pq + qj;
        if (j == i)
            continue;
        const bool excluded = (j == slots.x) | (j == slots.y) | (j == slots.z) | (j == slots.w);
        if constexpr (PART == kCoulombPartShort)
            if (excluded)
                continue;
        if constexpr (PART == kCoulombPartLong)
            if (!excluded)
                continue;
        const double dx = min_image(xi - sx[j], Lx, hx);
        const double dy = min_image(yi - sy[j], Ly, hy);
        const double dz = min_image(zi - sz[j], Lz, hz);
        const double rsq = (dx * dx + dy * dy) + dz * dz;
        if (!excluded && !(rsq < rcutsq))
            continue;
        const double rr = sqrt(rsq);
        const double kr = kappa * rr;
        const double g = two_self_c * exp(-(kr * kr));
        const double qq = qi * qj;
        double e, fdivr;
        if (excluded)
        {
            const double u = erf(kr) / rr;
            e = -(qq * u);
            fdivr = -(qq * (u - g)) / rsq;
        }
        else
        {
            const double u = erfc(kr) / rr;
            e = qq * u;
            fdivr = (qq * (u + g)) / rsq;
        }
        px = px + dx * fdivr;
        py = py + dy * fdivr;
        pz = pz + dz * fdivr;
        pw = pw + 0.5 * e;
    }

    // reciprocal space: partial s over k = s, s + S, ... (FACTORED: over the segments g = s, s + S, ..., each in k order); the
    // factors q_i and 2 q_i are applied once, to the partial
    double rx = 0.0, ry = 0.0, rz = 0.0, rw = 0.0;
    unsigned k_end = owner ? n_k : 0u;
    if constexpr (PART == kCoulombPartShort)
        k_end = 0u; // no walk over k
    const CoulombK* __restrict__ ktab = hdr->ktab + (size_t)k_base;
    const v2d* __restrict__ structure = hdr->structure + (size_t)k_base;
    if constexpr (FACTORED)
    {
        // The image has served: the tables of the workgroup's ROWS particles go over it, tables[r][axis][m].  Lane 3 r + axis
        // takes its coordinate out of the image before the barrier and writes after it.
        constexpr unsigned ROWS = BLOCK / S;
        static_assert(3 * ROWS <= BLOCK, "one lane fills one axis of one particle");
        const unsigned stride = lds_m + 1;
        v2d* __restrict__ tables = reinterpret_cast<v2d*>(s_coulomb);
        const unsigned fill_r = threadIdx.x / 3, fill_axis = threadIdx.x % 3;
        const bool fills = (fill_r < ROWS) && (first + fill_r < n) && (seg_count != 0);
        double fill_x = 0.0;
        if (fills)
            fill_x = (fill_axis == 0 ? sx : fill_axis == 1 ? sy : sz)[first + fill_r];
        __syncthreads();
        if (fills)
            ewald_fill_axis(tables + ((size_t)fill_r * 3 + fill_axis) * stride, 1u, fill_x,
                            fill_axis == 0 ? Lx : fill_axis == 1 ? Ly : Lz, fill_axis == 0 ? Mx : fill_axis == 1 ? My : Mz);
        __syncthreads();
        const uint4* __restrict__ segments = reinterpret_cast<const uint4*>(hdr->pad[0]) + (size_t)seg_first;
        const v2d* __restrict__ tx = tables + (size_t)r * 3 * stride;
        const v2d* __restrict__ ty = tx + stride;
        const v2d* __restrict__ tz = ty + stride;
        // The walk goes through the segments in chunks of two a lane.  The workgroup stages a chunk's entries of ktab and
        // structure in LDS, behind the tables, each entry loaded once and coalesced: read per lane out of global memory, 16
        // different k-vectors a wave instruction and the same table once per particle, the loads bound the walk
        // (profiles/coulomb_batch/README.md).  Lane s still takes g = s, s + S, ... in ascending order.
        constexpr unsigned CHUNK_SEGS = 2 * S, CHUNK_K = CHUNK_SEGS * SEG;
        static_assert(CHUNK_K <= BLOCK, "one lane stages one entry");
        CoulombK* __restrict__ chunk_k = reinterpret_cast<CoulombK*>(tables + (size_t)ROWS * 3 * stride);
        v2d* __restrict__ chunk_s = reinterpret_cast<v2d*>(chunk_k + CHUNK_K);
        for (unsigned c0 = 0; c0 < seg_count; c0 += CHUNK_SEGS)
        {
            const unsigned c1 = (seg_count - c0 < CHUNK_SEGS) ? seg_count : c0 + CHUNK_SEGS;
            const uint4 head = segments[c0], tail = segments[c1 - 1];
            const unsigned k0 = __builtin_amdgcn_readfirstlane(head.w);
            const unsigned tail_count = __builtin_amdgcn_readfirstlane(tail.z);
            const unsigned k1 = __builtin_amdgcn_readfirstlane(tail.w) + (tail_count < (unsigned)SEG ? tail_count : (unsigned)SEG);
            unsigned staged = k1 > k0 ? k1 - k0 : 0u;
            if (staged > CHUNK_K)
                staged = CHUNK_K;
            if (k0 >= n_k)
                staged = 0u;
            else if (staged > n_k - k0)
                staged = n_k - k0;
            __syncthreads(); // the chunk before has been walked
            if (threadIdx.x < staged)
            {
                chunk_k[threadIdx.x] = ktab[k0 + threadIdx.x];
                chunk_s[threadIdx.x] = structure[k0 + threadIdx.x];
            }
            __syncthreads();
            const unsigned g_end = k_end != 0 ? c1 : 0u;
            for (unsigned g = c0 + s; g < g_end; g += S)
            {
                const uint4 seg = segments[g];
                const int mx = (int)(seg.x & 0xFFFFu), my = (int)(short)(seg.x >> 16), zs = (int)seg.y;
                const unsigned at = seg.w - k0; // (a segment outside the staged entries walks nothing)
                unsigned count = seg.z < (unsigned)SEG ? seg.z : (unsigned)SEG;
                if (seg.w < k0 || at >= staged)
                    count = 0u;
                else if (count > staged - at)
                    count = staged - at;
                const v2d e1 = tz[1];
                v2d ph = ewald_mul(ewald_mul(ewald_power(tx, mx, 1u), ewald_power(ty, my, 1u)), ewald_power(tz, zs, 1u));
                for (unsigned u = 0; u < count; ++u)
                {
                    const CoulombK kv = chunk_k[at + u];
                    const v2d AB = chunk_s[at + u];
                    const double cs = ph.x, sn = ph.y;
                    const double f = kv.a * (AB.x * sn - AB.y * cs);
                    rx = rx + kv.kx * f;
                    ry = ry + kv.ky * f;
                    rz = rz + kv.kz * f;
                    rw = rw + kv.a * (AB.x * cs + AB.y * sn);
                    ph = ewald_mul(ph, e1);
                }
            }
        }
    }
    else
    {
        for (unsigned k = s; k < k_end; k += S)
        {
            const CoulombK kv = ktab[k];
            const v2d AB = structure[k];
            const double theta = (kv.kx * xi + kv.ky * yi) + kv.kz * zi;
            double sn, cs;
            sincos(theta, &sn, &cs);
            const double f = kv.a * (AB.x * sn - AB.y * cs);
            rx = rx + kv.kx * f;
            ry = ry + kv.ky * f;
            rz = rz + kv.kz * f;
            rw = rw + kv.a * (AB.x * cs + AB.y * sn);
        }
    }
    if constexpr (PART != kCoulombPartShort)
    {
        const double qi2 = 2.0 * qi;
        px = px + qi2 * rx;
        py = py + qi2 * ry;
        pz = pz + qi2 * rz;
        pw = pw + qi * rw;
    }

    // P = ((p0 + p1) + p2) + ...: every lane of the group folds the same S values in the same order
    double Px = __shfl(px, 0, S), Py = __shfl(py, 0, S), Pz = __shfl(pz, 0, S), Pw = __shfl(pw, 0, S), Q = __shfl(pq, 0, S);
#pragma unroll 1
    for (int u = 1; u < S; ++u)
    {
        Px = Px + __shfl(px, u, S);
        Py = Py + __shfl(py, u, S);
        Pz = Pz + __shfl(pz, u, S);
        Pw = Pw + __shfl(pw, u, S);
        Q = Q + __shfl(pq, u, S);
    }
    if (!owner || s != 0)
        return;
    // self and background
    if constexpr (PART != kCoulombPartShort)
        Pw = (Pw - row->self_c * (qi * qi)) - row->bg_c * (qi * Q);
    const v2d Fxy = {Px, Py}, Fzw = {Pz, Pw};
    force2[2 * (size_t)i] = Fxy;
    force2[2 * (size_t)i + 1] = Fzw;
    if constexpr (PART != kCoulombPartShort)
        if (i == 0)
        {
            const v2d Q0 = {Q, 0.0};
            hdr->structure[(size_t)k_base + n_k] = Q0;
        }
