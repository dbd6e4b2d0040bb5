// cavmd_coulomb.hip -- cavmd_coulomb of include/cavmd.h: Ewald Coulomb forces of a batch of small systems in two launches.
// One of the eleven objects built on an item table (cavmd_item_table.hpp); the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cavmd.h"
#include "cavmd_coulomb_batch_kernel.hpp"
#include "cavmd_ewald_factored_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- Ewald Coulomb forces of a batch of independent small systems in TWO launches (cavmd_coulomb_batch_kernel.hpp) ------------
// A LinkedTable as well: the status of an item with its k-vectors, and how the device tables follow from the items.
namespace
{
constexpr int kCoulombJSplit = CAVMD_COULOMB_J_SPLIT;
constexpr int kCoulombKSplit = CAVMD_COULOMB_K_SPLIT;
constexpr unsigned kCoulombRows = kCoulombBlock / kCoulombJSplit;
constexpr unsigned kCoulombKRows = kCoulombBlock / kCoulombKSplit;
static_assert(kCoulombJSplit == 1 || kCoulombJSplit == 4 || kCoulombJSplit == 16 || kCoulombJSplit == 64, "S is one of the candidates");
static_assert(kCoulombKSplit == 1 || kCoulombKSplit == 4 || kCoulombKSplit == 16 || kCoulombKSplit == 64, "T is one of the candidates");
static_assert(sizeof(cavmd_coulomb_item) == 96, "coulomb item layout");
static_assert(CAVMD_COULOMB_MAX_EXCLUSIONS == kCoulombMaxExclusions, "the header's limit is the kernel's");
static_assert(coulomb_lds_bytes(CAVMD_COULOMB_MAX_ITEM_N) <= 64 * 1024, "the largest system fits the LDS a kernel gets without opt-in");
// the factored reciprocal method (cavmd_ewald_factored_kernel.hpp): its splits are its own, whatever the direct kernels' are
constexpr unsigned kEwaldRows = kCoulombBlock / kEwaldJSplit;
constexpr unsigned kEwaldSegRows = kCoulombBlock / kEwaldKSplit;
static_assert(CAVMD_EWALD_MAX_M >= 16 && CAVMD_EWALD_MAX_M < 32768, "the driver's geometry needs 11; a segment keeps mx and my in 16 bits");
static_assert(ewald_structure_lds_bytes(CAVMD_EWALD_MAX_M) <= 64 * 1024 && ewald_structure_lds_bytes(CAVMD_EWALD_MAX_M + 1) > 64 * 1024,
              "CAVMD_EWALD_MAX_M is the largest limit whose tile of tables fits the LDS a kernel gets without opt-in");
static_assert(ewald_force_lds_bytes(CAVMD_COULOMB_MAX_ITEM_N, CAVMD_EWALD_MAX_M, kEwaldRows) <= 64 * 1024, "launch 2 as well");
constexpr double kCoulombPi = 3.141592653589793;
constexpr double kCoulombSqrtPi = 1.7724538509055159;

// what the factored method needs of an item's k-vectors: every row (mx, my) of consecutive mz cut into segments of at most
// kEwaldSegment vectors from its first mz on ({mx | my << 16, first mz, count, first k}), and the largest |m| per axis
struct EwaldLattice
{
    std::vector<uint4> segments;
    unsigned m[3] = {0, 0, 0};
};

// The kept k-vectors of an item (whose box and cut-offs have been checked), in the contract's order; stops at `limit` + 1.
// Every loop visits kept vectors and one more per row, so the work is bounded by the limit whatever k_cut is.
void coulomb_k_vectors(const cavmd_coulomb_item& it, size_t limit, std::vector<CoulombK>* out, size_t* count,
                       EwaldLattice* lattice = nullptr)
{
    const double two_pi = 2.0 * kCoulombPi;
    const double kc2 = it.k_cut * it.k_cut;
    const double V = (it.Lx * it.Ly) * it.Lz;
    const double four_kappa2 = 4.0 * (it.kappa * it.kappa);
    size_t K = 0;
    auto component = [&](long m, double L) { return (two_pi * (double)m) / L; };
    for (long mx = 0;; ++mx)
    {
        const double kx = component(mx, it.Lx);
        const double kxx = kx * kx;
        if (!(kxx <= kc2))
            break;
        if (mx > (long)limit + 1)
        {
            *count = limit + 1;
            return;
        }
        // every (mx, my) in range keeps at least one vector, and so does every mz in range: a search that runs past the limit
        // has already decided the answer
        long My = 0;
        while (true)
        {
            const double ky = component(My + 1, it.Ly);
            if (!(kxx + ky * ky <= kc2))
                break;
            if (++My > (long)limit + 1)
            {
                *count = limit + 1;
                return;
            }
        }
        for (long my = -My; my <= My; ++my)
        {
            if (mx == 0 && my < 0)
                continue;
            const double ky = component(my, it.Ly);
            const double kxy = kxx + ky * ky;
            long Mz = 0;
            while (true)
            {
                const double kz = component(Mz + 1, it.Lz);
                if (!(kxy + kz * kz <= kc2))
                    break;
                if (++Mz > (long)limit + 1)
                {
                    *count = limit + 1;
                    return;
                }
            }
            for (long mz = -Mz; mz <= Mz; ++mz)
            {
                if (mx == 0 && my == 0 && mz <= 0)
                    continue;
                const double kz = component(mz, it.Lz);
                const double k2 = kxy + kz * kz;
                if (!(k2 > 0.0 && k2 <= kc2))
                    continue;
                if (++K > limit)
                {
                    *count = K;
                    return;
                }
                if (lattice)
                {
                    // (the kept mz of a row are consecutive: k2 grows with |mz|)
                    std::vector<uint4>& segs = lattice->segments;
                    const unsigned key = ((unsigned)mx & 0xFFFFu) | (((unsigned)my & 0xFFFFu) << 16);
                    const unsigned k = (unsigned)(K - 1);
                    if (!segs.empty() && segs.back().x == key && segs.back().z < (unsigned)kEwaldSegment &&
                        segs.back().w + segs.back().z == k && (long)(int)segs.back().y + (long)segs.back().z == mz)
                        segs.back().z += 1;
                    else
                        segs.push_back(make_uint4(key, (unsigned)(int)mz, 1u, k));
                    lattice->m[0] = std::max(lattice->m[0], (unsigned)mx);
                    lattice->m[1] = std::max(lattice->m[1], (unsigned)std::labs(my));
                    lattice->m[2] = std::max(lattice->m[2], (unsigned)std::labs(mz));
                }
                if (out)
                    out->push_back(CoulombK {kx, ky, kz, ((4.0 * kCoulombPi) / V) * exp(-k2 / four_kappa2) / k2});
            }
        }
    }
    *count = K;
}

// the tables derived from one item: its partner slots (four a particle, from the exclusion list) and its k-vectors
struct CoulombDerived
{
    std::vector<uint32_t> slots;
    std::vector<CoulombK> ktab;
    EwaldLattice lattice;
};

// The status of one item.  `out`, if given, receives the item's derived tables, `out_K` the number of its k-vectors.
int coulomb_item_status(const cavmd_coulomb_item* it, CoulombDerived* out, size_t* out_K)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_force & 15) || ((uintptr_t)it->d_charge & 7) || ((uintptr_t)it->h_exclusions & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N != 0 && (!it->d_pos || !it->d_force || !it->d_charge))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->n_exclusions != 0 && !it->h_exclusions)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_COULOMB_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    if (it->N != 0)
    {
        double cut_sq = 0.0;
        if (!box_ok(it->Lx, it->Ly, it->Lz, &cut_sq))
            return CAVMD_ERR_INVALID_VALUE;
        if (!(isfinite(it->kappa) && it->kappa > 0.0) || !finite_nonnegative(it->r_cut) || !finite_nonnegative(it->k_cut))
            return CAVMD_ERR_INVALID_VALUE;
        if (it->r_cut * it->r_cut > cut_sq)
            return CAVMD_ERR_INVALID_VALUE;
    }
    const int st = partner_slots(it->N, it->h_exclusions, it->n_exclusions, kCoulombMaxExclusions, kCoulombNoPartner,
                                 [](uint32_t partner, uint32_t) { return partner; }, out ? &out->slots : nullptr);
    if (st != CAVMD_OK)
        return st;
    size_t K = 0;
    if (out)
    {
        out->ktab.clear();
        out->lattice = EwaldLattice();
    }
    if (it->N != 0)
    {
        coulomb_k_vectors(*it, CAVMD_COULOMB_MAX_K, out ? &out->ktab : nullptr, &K, out ? &out->lattice : nullptr);
        if (K > CAVMD_COULOMB_MAX_K)
            return CAVMD_ERR_CAPACITY;
    }
    if (out_K)
        *out_K = K;
    return CAVMD_OK;
}

CoulombRow coulomb_row(const cavmd_coulomb_item& it)
{
    CoulombRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.charge = it.d_charge;
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx;
    r.Ly = it.Ly;
    r.Lz = it.Lz;
    r.kappa = it.kappa;
    r.rcutsq = it.r_cut * it.r_cut;
    r.n = it.N;
    if (it.N != 0)
    {
        size_t K = 0;
        coulomb_k_vectors(it, CAVMD_COULOMB_MAX_K, nullptr, &K); // the item has been checked: K <= CAVMD_COULOMB_MAX_K
        r.n_k = (unsigned)K;
        r.self_c = it.kappa / kCoulombSqrtPi;
        r.bg_c = kCoulombPi / ((2.0 * ((it.Lx * it.Ly) * it.Lz)) * (it.kappa * it.kappa));
    }
    return r;
}

// what set_items replaces together
struct CoulombTables
{
    DeviceArray<uint4> k_blocks, blocks, partners;
    DeviceArray<CoulombK> ktab;
    DeviceArray<v2d> structure;
    DeviceArray<uint4> ewald;      // the factored method's tables, one array (cavmd_ewald_factored_kernel.hpp)
    std::vector<uint32_t> offsets; // per item: its first entry of ktab / structure
    CoulombHeader header;
    unsigned lds_n = 2;
    unsigned lds_m = 1; // the largest |m| of the table on any axis, at least 1
    unsigned n_ewald_k_blocks = 0, n_ewald_blocks = 0; // workgroups of the factored launches (header.pad[1] holds both)
};

// CAVMD_OK, or CAVMD_ERR_CAPACITY for an item the factored method has no LDS for
int ewald_capacity_status(const EwaldLattice& l)
{
    return std::max(l.m[0], std::max(l.m[1], l.m[2])) > (unsigned)CAVMD_EWALD_MAX_M ? CAVMD_ERR_CAPACITY : CAVMD_OK;
}
} // namespace

// workgroups by N descending
struct cavmd_coulomb final : LinkedTable<cavmd_coulomb_item, CoulombRow, CoulombDerived, CoulombTables>
{
    int reciprocal = CAVMD_EWALD_RECIPROCAL_DIRECT; // which two kernels compute enqueues
    std::vector<uint64_t> long_forces;              // per item its LONG array (cavmd_mts_coulomb_set_long_forces); empty: not split

    cavmd_coulomb() : LinkedTable([](const cavmd_coulomb_item& it) { return it.N; }, coulomb_row) {}

    // the long pointers of items [first, first + count) into the rows' spare word (a row built from an item carries 0 there);
    // the caller holds the DeviceGuard and has waited for the launches in flight
    hipError_t write_long(size_t first, size_t count, const uint64_t* values)
    {
        if (count == 0)
            return hipSuccess;
        char* at = reinterpret_cast<char*>(d_rows.ptr + first) + offsetof(CoulombRow, pad);
        return hipMemcpy2D(at, sizeof(CoulombRow), values, sizeof(uint64_t), sizeof(uint64_t), count, hipMemcpyHostToDevice);
    }

    // (while the factored method is selected, an item beyond its per-axis limit is refused like any other bad row; `out` is
    // never NULL here: LinkedTable::check_into is the only caller)
    int item_status(const cavmd_coulomb_item* it, CoulombDerived* out) const override
    {
        const int st = coulomb_item_status(it, out, nullptr);
        if (st != CAVMD_OK || reciprocal != CAVMD_EWALD_RECIPROCAL_FACTORED)
            return st;
        return ewald_capacity_status(out->lattice);
    }

    void strip(cavmd_coulomb_item* it) const override
    {
        it->h_exclusions = nullptr;
        it->n_exclusions = 0;
    }

    hipError_t fill(const std::vector<cavmd_coulomb_item>& all, const std::vector<unsigned>& launch,
                    const std::vector<CoulombDerived>& d, CoulombTables* t) const override
    {
        const size_t B = all.size();
        std::vector<uint32_t> partner_base(B), pool;
        std::vector<CoulombK> kpool;
        t->offsets.assign(B, 0);
        unsigned largest = 0;
        for (size_t i = 0; i < B; ++i)
        {
            partner_base[i] = pool_append(&pool, d[i].slots) / kCoulombMaxExclusions;
            t->offsets[i] = pool_append(&kpool, d[i].ktab);
            kpool.push_back(CoulombK {0.0, 0.0, 0.0, 0.0}); // the slot of {Q, 0}
            largest = std::max(largest, all[i].N);
        }
        std::vector<uint4> k_table, table;
        for (unsigned item : launch)
        {
            if (all[item].N == 0)
                continue;
            emit_blocks(&k_table, item, (unsigned)d[item].ktab.size(), kCoulombKRows, t->offsets[item], 0u);
            emit_blocks(&table, item, all[item].N, kCoulombRows, partner_base[item], t->offsets[item]);
        }
        // the factored method's tables: {where each begins}, launch-1 workgroups, launch-2 workgroups, items, segments
        size_t n_segments = 0, n_seg_blocks = 0, n_row_blocks = 0;
        for (size_t i = 0; i < B; ++i)
        {
            if (all[i].N == 0)
                continue;
            n_segments += d[i].lattice.segments.size();
            n_seg_blocks += (d[i].lattice.segments.size() + kEwaldSegRows - 1) / kEwaldSegRows;
            n_row_blocks += (all[i].N + kEwaldRows - 1) / kEwaldRows;
        }
        const size_t at_seg_blocks = 1, at_row_blocks = at_seg_blocks + n_seg_blocks, at_items = at_row_blocks + n_row_blocks;
        const size_t at_segments = at_items + B;
        std::vector<uint4> ewald(at_segments + n_segments, make_uint4(0, 0, 0, 0));
        ewald[0] = make_uint4((unsigned)at_seg_blocks, (unsigned)at_row_blocks, (unsigned)at_items, 0u);
        unsigned lds_m = 1;
        size_t seg_at = at_segments;
        for (size_t i = 0; i < B; ++i)
        {
            if (all[i].N == 0)
                continue;
            const EwaldLattice& l = d[i].lattice;
            ewald[at_items + i] = make_uint4((unsigned)seg_at, (unsigned)l.segments.size(), l.m[0] | (l.m[1] << 16), l.m[2]);
            std::copy(l.segments.begin(), l.segments.end(), ewald.begin() + seg_at);
            seg_at += l.segments.size();
            lds_m = std::max(lds_m, std::max(l.m[0], std::max(l.m[1], l.m[2])));
        }
        size_t seg_block = at_seg_blocks, row_block = at_row_blocks;
        for (unsigned item : launch)
        {
            if (all[item].N == 0)
                continue;
            const uint4 info = ewald[at_items + item];
            for (unsigned first = 0; first < info.y; first += kEwaldSegRows)
                ewald[seg_block++] = make_uint4(item, info.x + first, std::min(info.y - first, kEwaldSegRows), t->offsets[item]);
            for (unsigned first = 0; first < all[item].N; first += kEwaldRows)
                ewald[row_block++] = make_uint4(item, first, partner_base[item], t->offsets[item]);
        }
        hipError_t e = t->k_blocks.upload(k_table.data(), k_table.size());
        if (e == hipSuccess)
            e = t->ewald.upload(ewald.data(), ewald.size());
        if (e == hipSuccess)
            e = t->blocks.upload(table.data(), table.size());
        if (e == hipSuccess)
            e = t->ktab.upload(kpool.data(), kpool.size());
        if (e == hipSuccess)
            e = t->structure.alloc_zeroed(kpool.size());
        if (e == hipSuccess)
            e = t->partners.upload(pool.data(), pool.size());
        memset(&t->header, 0, sizeof(t->header));
        t->header.k_blocks = t->k_blocks.ptr;
        t->header.blocks = t->blocks.ptr;
        t->header.partners = t->partners.ptr;
        t->header.ktab = t->ktab.ptr;
        t->header.structure = t->structure.ptr;
        t->header.n_k_blocks = (unsigned)k_table.size();
        t->header.n_blocks = (unsigned)table.size();
        t->header.pad[0] = (uint64_t)(uintptr_t)t->ewald.ptr;
        t->header.pad[1] = (uint64_t)n_seg_blocks | ((uint64_t)n_row_blocks << 32);
        t->n_ewald_k_blocks = (unsigned)n_seg_blocks;
        t->n_ewald_blocks = (unsigned)n_row_blocks;
        t->lds_n = lds_particles(largest);
        t->lds_m = lds_m;
        return e;
    }
};

extern "C"
{

int cavmd_coulomb_item_check(const cavmd_coulomb_item* it)
{
    return coulomb_item_status(it, nullptr, nullptr);
}

int cavmd_coulomb_k_count(const cavmd_coulomb_item* it, uint32_t* out_K)
{
    if (!out_K)
        return CAVMD_ERR_INVALID_VALUE;
    size_t K = 0;
    const int st = coulomb_item_status(it, nullptr, &K);
    if (st != CAVMD_OK)
        return st;
    *out_K = (uint32_t)K;
    return CAVMD_OK;
}

int cavmd_coulomb_parameters(double r_cut, double accuracy, double* kappa, double* k_cut)
{
    if (!kappa || !k_cut || !(isfinite(r_cut) && r_cut > 0.0) || !(accuracy > 0.0 && accuracy < 1.0))
        return CAVMD_ERR_INVALID_VALUE;
    const double s = sqrt(-log(accuracy));
    *kappa = s / r_cut;
    *k_cut = (2.0 * *kappa) * s;
    return CAVMD_OK;
}

int cavmd_coulomb_order(int* rows, int* j_split, int* k_rows, int* k_split)
{
    if (rows)
        *rows = (int)kCoulombRows;
    if (j_split)
        *j_split = kCoulombJSplit;
    if (k_rows)
        *k_rows = (int)kCoulombKRows;
    if (k_split)
        *k_split = kCoulombKSplit;
    return CAVMD_OK;
}

int cavmd_coulomb_create(cavmd_workspace* ws, size_t n_items, const cavmd_coulomb_item* h_items, cavmd_coulomb** out)
{
    return create_table(tie_of(ws), n_items, h_items, out, CAVMD_OK, [](cavmd_coulomb*) {});
}

int cavmd_coulomb_destroy(cavmd_coulomb* c)
{
    return destroy_table(c);
}

int cavmd_coulomb_set_items(cavmd_coulomb* c, size_t first, size_t count, const cavmd_coulomb_item* h_items)
{
    if (!c)
        return CAVMD_ERR_INVALID_VALUE;
    if (c->long_forces.empty())
        return c->set_items(first, count, h_items);
    // a split batch: every item keeps its long array, so a new item must be able to live with the one it inherits
    if (!c->within(first, count, h_items))
        return CAVMD_ERR_INVALID_VALUE;
    for (size_t i = 0; i < count; ++i)
    {
        const uint64_t kept = c->long_forces[first + i];
        if ((h_items[i].N != 0 && kept == 0) || (kept != 0 && kept == (uint64_t)(uintptr_t)h_items[i].d_force))
            return CAVMD_ERR_INVALID_VALUE;
    }
    const int st = c->set_items(first, count, h_items);
    if (st != CAVMD_OK)
        return st;
    DeviceGuard guard(c->device);
    return hip_status(c->write_long(first, count, c->long_forces.data() + first)); // (set_items has waited; nothing is in flight)
}

int cavmd_mts_coulomb_set_long_forces(cavmd_coulomb* c, size_t n_items, cavmd_double4* const* h_long_force)
{
    if (!c || !h_long_force || n_items != c->n)
        return CAVMD_ERR_INVALID_VALUE;
    size_t set = 0;
    for (size_t i = 0; i < n_items; ++i)
    {
        const uintptr_t p = (uintptr_t)h_long_force[i];
        if ((p & 15) || (p != 0 && p == (uintptr_t)c->items[i].d_force))
            return CAVMD_ERR_INVALID_VALUE;
        set += (p != 0);
    }
    if (set != 0) // all NULL drops the split; otherwise NULL only for N == 0
        for (size_t i = 0; i < n_items; ++i)
            if (!h_long_force[i] && c->items[i].N != 0)
                return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(c->device);
    const int st = c->wait_idle(); // refuses while the stream of the last launch is being captured
    if (st != CAVMD_OK)
        return st;
    std::vector<uint64_t> values(n_items);
    for (size_t i = 0; i < n_items; ++i)
        values[i] = (uint64_t)(uintptr_t)h_long_force[i];
    CAVMD_HIP_TRY(c->write_long(0, n_items, values.data()));
    if (set == 0)
        values.clear();
    c->long_forces.swap(values);
    return CAVMD_OK;
}

int cavmd_mts_coulomb_compute_parts(cavmd_coulomb* c, void* stream_, unsigned parts)
{
    if (!c || c->long_forces.empty() || parts == 0 || (parts & ~(CAVMD_COULOMB_PART_SHORT | CAVMD_COULOMB_PART_LONG)) != 0)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    const CoulombTables& t = c->tables;
    const size_t lds = coulomb_lds_bytes(t.lds_n);
    const dim3 block(kCoulombBlock), rows_grid(std::max(t.header.n_blocks, 1u));
    if (parts & CAVMD_COULOMB_PART_SHORT)
    {
        const int st = c->launch(stream, coulomb_short_kernel<kCoulombBlock, kCoulombJSplit>, rows_grid, block, lds, c->d_rows.ptr,
                                 c->d_header.ptr, t.lds_n);
        if (st != CAVMD_OK)
            return st;
    }
    if (!(parts & CAVMD_COULOMB_PART_LONG))
        return CAVMD_OK;
    // the structure factors by the batch's method, as cavmd_coulomb_compute launches them, then the long kernel of that method
    if (c->reciprocal == CAVMD_EWALD_RECIPROCAL_FACTORED)
    {
        const int st = c->launch(stream, ewald_structure_factored_kernel<kCoulombBlock, kEwaldKSplit, kEwaldSegment, kEwaldTile>,
                                 dim3(std::max(t.n_ewald_k_blocks, 1u)), block, ewald_structure_lds_bytes(t.lds_m), c->d_rows.ptr,
                                 c->d_header.ptr, t.lds_m);
        if (st != CAVMD_OK)
            return st;
        return c->launch(stream, ewald_long_factored_kernel<kCoulombBlock, kEwaldJSplit, kEwaldSegment>,
                         dim3(std::max(t.n_ewald_blocks, 1u)), block, ewald_force_lds_bytes(t.lds_n, t.lds_m, kEwaldRows),
                         c->d_rows.ptr, c->d_header.ptr, t.lds_n, t.lds_m);
    }
    const int st = c->launch(stream, coulomb_structure_kernel<kCoulombBlock, kCoulombKSplit>, dim3(std::max(t.header.n_k_blocks, 1u)),
                             block, lds, c->d_rows.ptr, c->d_header.ptr, t.lds_n);
    if (st != CAVMD_OK)
        return st;
    return c->launch(stream, coulomb_long_kernel<kCoulombBlock, kCoulombJSplit>, rows_grid, block, lds, c->d_rows.ptr, c->d_header.ptr,
                     t.lds_n);
}

int cavmd_coulomb_compute(cavmd_coulomb* c, void* stream_)
{
    if (!c)
        return CAVMD_ERR_INVALID_VALUE;
    hipStream_t stream = (hipStream_t)stream_;
    const CoulombTables& t = c->tables;
    if (c->reciprocal == CAVMD_EWALD_RECIPROCAL_FACTORED)
    {
        const int st = c->launch(stream, ewald_structure_factored_kernel<kCoulombBlock, kEwaldKSplit, kEwaldSegment, kEwaldTile>,
                                 dim3(std::max(t.n_ewald_k_blocks, 1u)), dim3(kCoulombBlock), ewald_structure_lds_bytes(t.lds_m),
                                 c->d_rows.ptr, c->d_header.ptr, t.lds_m);
        if (st != CAVMD_OK)
            return st;
        return c->launch(stream, ewald_force_factored_kernel<kCoulombBlock, kEwaldJSplit, kEwaldSegment>,
                         dim3(std::max(t.n_ewald_blocks, 1u)), dim3(kCoulombBlock),
                         ewald_force_lds_bytes(t.lds_n, t.lds_m, kEwaldRows), c->d_rows.ptr, c->d_header.ptr, t.lds_n, t.lds_m);
    }
    const size_t lds = coulomb_lds_bytes(t.lds_n);
    // two launches, each noted once it is in flight: a refused second one leaves the first to be waited for
    const int st = c->launch(stream, coulomb_structure_kernel<kCoulombBlock, kCoulombKSplit>, dim3(std::max(t.header.n_k_blocks, 1u)),
                             dim3(kCoulombBlock), lds, c->d_rows.ptr, c->d_header.ptr, t.lds_n);
    if (st != CAVMD_OK)
        return st;
    return c->launch(stream, coulomb_force_kernel<kCoulombBlock, kCoulombJSplit>, dim3(std::max(t.header.n_blocks, 1u)),
                     dim3(kCoulombBlock), lds, c->d_rows.ptr, c->d_header.ptr, t.lds_n);
}

int cavmd_coulomb_structure_device_ptr(cavmd_coulomb* c, const double** out, const uint32_t** h_offsets)
{
    if (!c || (!out && !h_offsets))
        return CAVMD_ERR_INVALID_VALUE;
    if (out)
        *out = reinterpret_cast<const double*>(c->tables.structure.ptr);
    if (h_offsets)
        *h_offsets = c->tables.offsets.data();
    return CAVMD_OK;
}

// ---- the reciprocal-space method of a Coulomb batch (include/cavmd.h) ----------------------------------------------------------
int cavmd_ewald_order(int* tile, int* segment, int* max_m, int* rows, int* segment_rows)
{
    if (tile)
        *tile = kEwaldTile;
    if (segment)
        *segment = kEwaldSegment;
    if (max_m)
        *max_m = CAVMD_EWALD_MAX_M;
    if (rows)
        *rows = (int)kEwaldRows;
    if (segment_rows)
        *segment_rows = (int)kEwaldSegRows;
    return CAVMD_OK;
}

int cavmd_ewald_set_reciprocal(cavmd_coulomb* c, int method)
{
    if (!c || (method != CAVMD_EWALD_RECIPROCAL_DIRECT && method != CAVMD_EWALD_RECIPROCAL_FACTORED))
        return CAVMD_ERR_INVALID_VALUE;
    if (c->enqueued && stream_capturing(c->last_stream))
        return CAVMD_ERR_INVALID_VALUE;
    if (method == CAVMD_EWALD_RECIPROCAL_FACTORED)
        for (size_t i = 0; i < c->n; ++i)
            if (c->items[i].N != 0 && ewald_capacity_status(c->derived[i].lattice) != CAVMD_OK)
                return CAVMD_ERR_CAPACITY;
    c->reciprocal = method;
    return CAVMD_OK;
}

int cavmd_ewald_get_reciprocal(const cavmd_coulomb* c, int* method)
{
    if (!c || !method)
        return CAVMD_ERR_INVALID_VALUE;
    *method = c->reciprocal;
    return CAVMD_OK;
}

} // extern "C"
