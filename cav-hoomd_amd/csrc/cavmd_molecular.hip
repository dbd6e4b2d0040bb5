// cavmd_molecular.hip -- cavmd_molecular of include/cavmd.h: bonds and Lennard-Jones pairs of a batch of small systems in one launch.
// One of the eleven objects built on an item table (cavmd_item_table.hpp); the workspace is an incomplete type here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cavmd.h"
#include "cavmd_molecular_batch_kernel.hpp"
#include "cavmd_item_table.hpp"

using namespace cavmd;

// ---- harmonic bonds and Lennard-Jones pairs of a batch of independent small systems in ONE launch (cavmd_molecular_batch_kernel.hpp) --
// A LinkedTable (cavmd_item_table.hpp): what is below is the status of an item and how the device tables follow from the items.
namespace
{
constexpr int kMolecularJSplit = CAVMD_MOLECULAR_J_SPLIT;
constexpr unsigned kMolecularRows = kMolecularBlock / kMolecularJSplit;
static_assert(kMolecularJSplit == 1 || kMolecularJSplit == 4 || kMolecularJSplit == 16, "S is one of the measured candidates");
static_assert(sizeof(cavmd_molecular_pair) == sizeof(MolecularPair) && sizeof(cavmd_molecular_params) == sizeof(MolecularParams)
                  && offsetof(cavmd_molecular_pair, lj1) == 0 && offsetof(cavmd_molecular_pair, lj2) == 8
                  && offsetof(cavmd_molecular_pair, lj1_12) == 16 && offsetof(cavmd_molecular_pair, lj2_6) == 24
                  && offsetof(cavmd_molecular_pair, rcutsq) == 32 && offsetof(cavmd_molecular_pair, eshift) == 40
                  && offsetof(cavmd_molecular_params, n_types) == offsetof(MolecularParams, n_types)
                  && offsetof(cavmd_molecular_params, n_bond_types) == offsetof(MolecularParams, n_bond_types)
                  && offsetof(cavmd_molecular_params, pair) == offsetof(MolecularParams, pair)
                  && offsetof(cavmd_molecular_params, bond) == offsetof(MolecularParams, bond),
              "the molecular parameters are uploaded as they are");
static_assert(sizeof(cavmd_molecular_item) == 64 && sizeof(cavmd_molecular_bond) == 12, "molecular item layout");
static_assert(CAVMD_MOLECULAR_MAX_TYPES == kMolecularMaxTypes && CAVMD_MOLECULAR_MAX_BONDS == kMolecularMaxBonds
                  && CAVMD_MOLECULAR_MAX_BOND_TYPES == 8,
              "the header's limits are the kernel's");
static_assert(molecular_lds_bytes(CAVMD_MOLECULAR_MAX_ITEM_N) <= 64 * 1024, "the largest system fits the LDS a kernel gets without opt-in");
static_assert(CAVMD_MOLECULAR_MAX_ITEM_N <= 0xFFFF, "a partner index takes the low 16 bits of a slot");

// The status of one item; `prm` NULL: only what can be said without the parameters (bond types and the cut-offs are not
// looked at).  `slots`, if given, receives the item's partner table: four slots a particle, partner | bond type << 16.
int molecular_item_status(const cavmd_molecular_params* prm, const cavmd_molecular_item* it, std::vector<uint32_t>* slots)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (((uintptr_t)it->d_pos & 15) || ((uintptr_t)it->d_force & 15) || ((uintptr_t)it->h_bonds & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N != 0 && (!it->d_pos || !it->d_force))
        return CAVMD_ERR_INVALID_VALUE;
    if (it->n_bonds != 0 && !it->h_bonds)
        return CAVMD_ERR_INVALID_VALUE;
    if (it->N > CAVMD_MOLECULAR_MAX_ITEM_N)
        return CAVMD_ERR_CAPACITY;
    if (it->N != 0)
    {
        double cut_sq = 0.0;
        if (!box_ok(it->Lx, it->Ly, it->Lz, &cut_sq))
            return CAVMD_ERR_INVALID_VALUE;
        if (prm)
            for (unsigned a = 0; a < prm->n_types; ++a)
                for (unsigned b = 0; b < prm->n_types; ++b)
                    if (prm->pair[a][b].rcutsq > cut_sq)
                        return CAVMD_ERR_INVALID_VALUE;
    }
    const uint32_t n_bond_types = prm ? prm->n_bond_types : CAVMD_MOLECULAR_MAX_BOND_TYPES;
    for (uint32_t k = 0; k < it->n_bonds; ++k)
        if (it->h_bonds[k].type >= n_bond_types)
            return CAVMD_ERR_INVALID_VALUE;
    return partner_slots(it->N, it->h_bonds, it->n_bonds, kMolecularMaxBonds, kMolecularNoPartner,
                         [](uint32_t partner, uint32_t type) { return partner | (type << 16); }, slots);
}

MolecularRow molecular_row(const cavmd_molecular_item& it)
{
    MolecularRow r;
    memset(&r, 0, sizeof(r));
    r.pos2 = reinterpret_cast<const v2d*>(it.d_pos);
    r.force2 = reinterpret_cast<v2d*>(it.d_force);
    r.Lx = it.Lx;
    r.Ly = it.Ly;
    r.Lz = it.Lz;
    r.n = it.N;
    return r;
}

// what set_items replaces together
struct MolecularTables
{
    DeviceArray<uint4> blocks, partners;
    MolecularHeader header;
    unsigned lds_n = 2; // particles the next launch has LDS for
};
} // namespace

// workgroups by N descending; per item its partner table
struct cavmd_molecular final : LinkedTable<cavmd_molecular_item, MolecularRow, std::vector<uint32_t>, MolecularTables>
{
    cavmd_molecular_params params;
    DeviceArray<MolecularParams> d_params;

    cavmd_molecular() : LinkedTable([](const cavmd_molecular_item& it) { return it.N; }, molecular_row) {}

    int item_status(const cavmd_molecular_item* it, std::vector<uint32_t>* slots) const override
    {
        return molecular_item_status(&params, it, slots);
    }

    void strip(cavmd_molecular_item* it) const override
    {
        it->h_bonds = nullptr;
        it->n_bonds = 0;
    }

    hipError_t alloc_own()
    {
        const hipError_t e = LinkedTable::alloc_own();
        return e == hipSuccess ? d_params.upload(&params, 1) : e; // a blocking copy: there before any launch
    }

    hipError_t fill(const std::vector<cavmd_molecular_item>& all, const std::vector<unsigned>& launch,
                    const std::vector<std::vector<uint32_t>>& slots, MolecularTables* t) const override
    {
        std::vector<uint32_t> base(all.size()), pool;
        unsigned largest = 0;
        for (size_t i = 0; i < all.size(); ++i)
        {
            base[i] = pool_append(&pool, slots[i]) / kMolecularMaxBonds;
            largest = std::max(largest, all[i].N);
        }
        std::vector<uint4> table;
        for (unsigned item : launch)
            emit_blocks(&table, item, all[item].N, kMolecularRows, base[item], 0u);
        hipError_t e = t->blocks.upload(table.data(), table.size());
        if (e == hipSuccess)
            e = t->partners.upload(pool.data(), pool.size());
        memset(&t->header, 0, sizeof(t->header));
        t->header.blocks = t->blocks.ptr;
        t->header.partners = t->partners.ptr;
        t->header.n_blocks = (unsigned)table.size();
        t->lds_n = lds_particles(largest);
        return e;
    }
};

extern "C"
{

int cavmd_molecular_pair_make(double epsilon, double sigma, double r_cut, int shift, cavmd_molecular_pair* out)
{
    if (!out || !finite_nonnegative(epsilon) || !finite_nonnegative(sigma) || !finite_nonnegative(r_cut))
        return CAVMD_ERR_INVALID_VALUE;
    cavmd_molecular_pair p;
    memset(&p, 0, sizeof(p));
    const double s2 = sigma * sigma;
    const double s6 = (s2 * s2) * s2;
    p.lj2 = (4.0 * epsilon) * s6;
    p.lj1 = p.lj2 * s6;
    p.lj1_12 = 12.0 * p.lj1;
    p.lj2_6 = 6.0 * p.lj2;
    p.rcutsq = r_cut * r_cut;
    p.eshift = 0.0;
    if (shift && p.rcutsq > 0.0)
    {
        const double r2inv = 1.0 / p.rcutsq;
        const double r6inv = (r2inv * r2inv) * r2inv;
        p.eshift = r6inv * ((p.lj1 * r6inv) - p.lj2);
    }
    if (!isfinite(p.lj1_12) || !isfinite(p.lj2_6) || !isfinite(p.rcutsq) || !isfinite(p.eshift))
        return CAVMD_ERR_INVALID_VALUE;
    *out = p;
    return CAVMD_OK;
}

int cavmd_molecular_params_check(const cavmd_molecular_params* prm)
{
    if (!prm || prm->n_types > CAVMD_MOLECULAR_MAX_TYPES || prm->n_bond_types > CAVMD_MOLECULAR_MAX_BOND_TYPES || prm->reserved != 0)
        return CAVMD_ERR_INVALID_VALUE;
    for (unsigned a = 0; a < prm->n_types; ++a)
        for (unsigned b = 0; b < prm->n_types; ++b)
        {
            const cavmd_molecular_pair& p = prm->pair[a][b];
            if (!finite_nonnegative(p.lj1) || !finite_nonnegative(p.lj2) || !finite_nonnegative(p.lj1_12) || !finite_nonnegative(p.lj2_6)
                || !finite_nonnegative(p.rcutsq) || !isfinite(p.eshift) || p.reserved[0] != 0 || p.reserved[1] != 0)
                return CAVMD_ERR_INVALID_VALUE;
            if (memcmp(&p, &prm->pair[b][a], sizeof(p)) != 0)
                return CAVMD_ERR_INVALID_VALUE;
        }
    for (unsigned k = 0; k < prm->n_bond_types; ++k)
        if (!finite_nonnegative(prm->bond[k].K) || !finite_nonnegative(prm->bond[k].r0))
            return CAVMD_ERR_INVALID_VALUE;
    return CAVMD_OK;
}

int cavmd_molecular_item_check(const cavmd_molecular_params* prm, const cavmd_molecular_item* it)
{
    if (!it)
        return CAVMD_ERR_INVALID_VALUE;
    const int st = cavmd_molecular_params_check(prm);
    if (st != CAVMD_OK)
        return st;
    return molecular_item_status(prm, it, nullptr);
}

int cavmd_molecular_order(int* rows, int* j_split)
{
    if (rows)
        *rows = (int)kMolecularRows;
    if (j_split)
        *j_split = kMolecularJSplit;
    return CAVMD_OK;
}

int cavmd_molecular_create(cavmd_workspace* ws, const cavmd_molecular_params* prm, size_t n_items, const cavmd_molecular_item* h_items,
                           cavmd_molecular** out)
{
    return create_table(tie_of(ws), n_items, h_items, out, cavmd_molecular_params_check(prm),
                        [&](cavmd_molecular* m) { m->params = *prm; });
}

int cavmd_molecular_destroy(cavmd_molecular* m)
{
    return destroy_table(m);
}

int cavmd_molecular_set_items(cavmd_molecular* m, size_t first, size_t count, const cavmd_molecular_item* h_items)
{
    return m ? m->set_items(first, count, h_items) : CAVMD_ERR_INVALID_VALUE;
}

int cavmd_molecular_compute(cavmd_molecular* m, void* stream_)
{
    if (!m)
        return CAVMD_ERR_INVALID_VALUE;
    const MolecularTables& t = m->tables;
    return m->launch((hipStream_t)stream_, molecular_force_kernel<kMolecularBlock, kMolecularJSplit>,
                     dim3(std::max(t.header.n_blocks, 1u)), dim3(kMolecularBlock), molecular_lds_bytes(t.lds_n), m->d_rows.ptr,
                     m->d_header.ptr, m->d_params.ptr, t.lds_n);
}

} // extern "C"
