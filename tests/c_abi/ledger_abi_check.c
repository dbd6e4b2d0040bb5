/* ledger_abi_check.c -- the energy-ledger part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it
 * with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_ledger_row and cavmd_ledger_item for the
 * test to compare with the ctypes structures, and checks the per-item validation (host arithmetic), the refusals of
 * cavmd_ledger_create's scalar arguments and that every entry point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, type, field) ABI_OFF(which, cavmd_##type, field)

int main(void)
{
    cavmd_ledger_item it;
    cavmd_ledger* l = NULL;
    cavmd_ledger_row row;
    const cavmd_ledger_row* dr = NULL;
    const uint64_t* drows = NULL;
    uint64_t rows = 0;
    ABI_SIZE(row, cavmd_ledger_row);
    ABI_SIZE(item, cavmd_ledger_item);
    OFF(row, ledger_row, call);
    OFF(row, ledger_row, n_terms);
    OFF(row, ledger_row, n_reservoirs);
    OFF(row, ledger_row, time);
    OFF(row, ledger_row, potential);
    OFF(row, ledger_row, cavity);
    OFF(row, ledger_row, cavity_potential);
    OFF(row, ledger_row, potential_total);
    OFF(row, ledger_row, kinetic_group);
    OFF(row, ledger_row, kinetic_cavity);
    OFF(row, ledger_row, kinetic_total);
    OFF(row, ledger_row, system_total);
    OFF(row, ledger_row, reservoir);
    OFF(row, ledger_row, reservoir_total);
    OFF(row, ledger_row, universe_total);
    OFF(row, ledger_row, temperature);
    OFF(row, ledger_row, reserved);
    OFF(item, ledger_item, d_result);
    OFF(item, ledger_item, d_vel);
    OFF(item, ledger_item, d_members);
    OFF(item, ledger_item, n_members);
    OFF(item, ledger_item, N);
    OFF(item, ledger_item, d_energy);
    OFF(item, ledger_item, d_reservoir);
    OFF(item, ledger_item, d_time);
    OFF(item, ledger_item, dof);
    OFF(item, ledger_item, add_cavity_kinetic);
    OFF(item, ledger_item, reserved0);
    OFF(item, ledger_item, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 3;
    memset(&it, 0, sizeof(it));
    memset(&row, 0, sizeof(row));
    if (cavmd_ledger_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 4;
    if (cavmd_ledger_item_check(&it) != CAVMD_OK) /* everything may be left out: a row of zeros */
        return 5;
    it.d_result = (const cavmd_result*)(uintptr_t)0x1000;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x2000;
    it.d_members = (const uint32_t*)(uintptr_t)0x3004;
    it.n_members = 500;
    it.N = 501;
    it.d_energy[0] = (const cavmd_double4*)(uintptr_t)0x4000;
    it.d_energy[1] = (const cavmd_double4*)(uintptr_t)0x5000;
    it.d_reservoir[0] = (const double*)(uintptr_t)0x6008;
    it.d_time = (const double*)(uintptr_t)0x7008;
    it.dof = 1500.0;
    it.add_cavity_kinetic = 1;
    if (cavmd_ledger_item_check(&it) != CAVMD_OK)
        return 6;
    it.d_energy[1] = (const cavmd_double4*)(uintptr_t)0x5008;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 7;
    it.d_energy[1] = NULL;
    it.d_energy[2] = (const cavmd_double4*)(uintptr_t)0x5000; /* a gap */
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 8;
    it.d_energy[2] = NULL;
    it.d_reservoir[0] = (const double*)(uintptr_t)0x6004;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it.d_reservoir[0] = NULL;
    it.d_reservoir[1] = (const double*)(uintptr_t)0x6008; /* a gap */
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_reservoir[1] = NULL;
    it.d_time = (const double*)(uintptr_t)0x7004;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.d_time = NULL;
    it.dof = -1.0;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    it.dof = 0.0;
    it.add_cavity_kinetic = 2;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.add_cavity_kinetic = 0;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 14;
    it.N = CAVMD_BATCH_MAX_ITEM_N;
    it.n_members = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 15;
    it.n_members = CAVMD_BATCH_MAX_ITEM_N;
    if (cavmd_ledger_item_check(&it) != CAVMD_OK)
        return 16;
    it.reserved = 1;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 17;
    it.reserved = 0;
    it.reserved0 = 1;
    if (cavmd_ledger_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 18;
    it.reserved0 = 0;
    /* null handles are refused before anything else */
    if (cavmd_ledger_create(NULL, 1, &it, 8, 1, 3.167e-6, &l) != CAVMD_ERR_INVALID_VALUE || l != NULL)
        return 19;
    if (cavmd_ledger_create(NULL, 1, &it, 8, 1, 3.167e-6, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 20;
    if (cavmd_ledger_destroy(NULL) != CAVMD_OK)
        return 21;
    if (cavmd_ledger_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_ledger_record(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_ledger_rows(NULL, NULL, &rows) != CAVMD_ERR_INVALID_VALUE
        || cavmd_ledger_read(NULL, NULL, 0, 1, 0, 1, &row) != CAVMD_ERR_INVALID_VALUE
        || cavmd_ledger_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_ledger_device_ptr(NULL, &dr, &drows) != CAVMD_ERR_INVALID_VALUE)
        return 22;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            /* the 1 GiB cap: 2^30 / 192 rows of one item */
            if (cavmd_ledger_create(ws, 0, &it, 8, 1, 3.167e-6, &l) != CAVMD_ERR_INVALID_VALUE
                || cavmd_ledger_create(ws, 1, &it, 0, 1, 3.167e-6, &l) != CAVMD_ERR_INVALID_VALUE
                || cavmd_ledger_create(ws, 1, &it, 8, 0, 3.167e-6, &l) != CAVMD_ERR_INVALID_VALUE
                || cavmd_ledger_create(ws, 1, &it, 8, 1, 0.0, &l) != CAVMD_ERR_INVALID_VALUE
                || cavmd_ledger_create(ws, 1, &it, 8, 1, -1.0, &l) != CAVMD_ERR_INVALID_VALUE
                || cavmd_ledger_create(ws, 1, &it, ((size_t)1 << 30) / 192 + 1, 1, 3.167e-6, &l) != CAVMD_ERR_CAPACITY || l != NULL)
                return 23;
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no ledger\n");
        else
            return 24;
    }
    printf("LEDGER-ABI-OK\n");
    return 0;
}
