/* recorder_abi_check.c -- the recorder part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it
 * with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_record and cavmd_recorder_item for the
 * test to compare with the ctypes structures, and checks the per-item validation (host arithmetic), the refusals of
 * cavmd_recorder_create's scalar arguments and that every entry point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, type, field) ABI_OFF(which, cavmd_##type, field)

int main(void)
{
    cavmd_recorder_item it;
    cavmd_recorder* r = NULL;
    cavmd_record rec;
    const cavmd_record* dr = NULL;
    const uint64_t* drows = NULL;
    uint64_t rows = 0;
    ABI_SIZE(record, cavmd_record);
    ABI_SIZE(item, cavmd_recorder_item);
    OFF(record, record, call);
    OFF(record, record, eval_sequence);
    OFF(record, record, energy);
    OFF(record, record, total_dipole);
    OFF(record, record, q);
    OFF(record, record, cavity_kinetic);
    OFF(record, record, cavity_temperature);
    OFF(record, record, kinetic_energy);
    OFF(record, record, force_mass_sum);
    OFF(record, record, reserved);
    OFF(item, recorder_item, d_result);
    OFF(item, recorder_item, d_vel);
    OFF(item, recorder_item, d_net_force);
    OFF(item, recorder_item, d_members);
    OFF(item, recorder_item, N);
    OFF(item, recorder_item, n_members);
    OFF(item, recorder_item, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 3;
    memset(&it, 0, sizeof(it));
    memset(&rec, 0, sizeof(rec));
    if (cavmd_recorder_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 4;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* d_result is required */
        return 5;
    it.d_result = (const cavmd_result*)(uintptr_t)0x1000;
    if (cavmd_recorder_item_check(&it) != CAVMD_OK) /* everything else may be left out */
        return 6;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x2000;
    it.d_net_force = (const cavmd_double4*)(uintptr_t)0x3000;
    it.d_members = (const uint32_t*)(uintptr_t)0x4004;
    it.N = 501;
    it.n_members = 500;
    if (cavmd_recorder_item_check(&it) != CAVMD_OK)
        return 7;
    it.d_result = (const cavmd_result*)(uintptr_t)0x1008;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 8;
    it.d_result = (const cavmd_result*)(uintptr_t)0x1000;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x2008;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x2000;
    it.d_net_force = (const cavmd_double4*)(uintptr_t)0x3004;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_net_force = (const cavmd_double4*)(uintptr_t)0x3000;
    it.d_members = (const uint32_t*)(uintptr_t)0x4002;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.d_members = (const uint32_t*)(uintptr_t)0x4004;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 12;
    it.N = CAVMD_BATCH_MAX_ITEM_N;
    it.n_members = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 13;
    it.n_members = CAVMD_BATCH_MAX_ITEM_N;
    if (cavmd_recorder_item_check(&it) != CAVMD_OK)
        return 14;
    it.reserved[1] = 1;
    if (cavmd_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 15;
    it.reserved[1] = 0;
    /* null handles are refused before anything else */
    if (cavmd_recorder_create(NULL, 1, &it, 8, 1, 3.167e-6, &r) != CAVMD_ERR_INVALID_VALUE || r != NULL)
        return 16;
    if (cavmd_recorder_create(NULL, 1, &it, 8, 1, 3.167e-6, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 17;
    if (cavmd_recorder_destroy(NULL) != CAVMD_OK)
        return 18;
    if (cavmd_recorder_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_recorder_record(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_recorder_rows(NULL, NULL, &rows) != CAVMD_ERR_INVALID_VALUE
        || cavmd_recorder_read(NULL, NULL, 0, 1, 0, 1, &rec) != CAVMD_ERR_INVALID_VALUE
        || cavmd_recorder_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_recorder_device_ptr(NULL, &dr, &drows) != CAVMD_ERR_INVALID_VALUE)
        return 19;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            if (cavmd_recorder_create(ws, 0, &it, 8, 1, 3.167e-6, &r) != CAVMD_ERR_INVALID_VALUE
                || cavmd_recorder_create(ws, 1, &it, 0, 1, 3.167e-6, &r) != CAVMD_ERR_INVALID_VALUE
                || cavmd_recorder_create(ws, 1, &it, 8, 0, 3.167e-6, &r) != CAVMD_ERR_INVALID_VALUE
                || cavmd_recorder_create(ws, 1, &it, 8, 1, 0.0, &r) != CAVMD_ERR_INVALID_VALUE
                || cavmd_recorder_create(ws, 1, &it, 8, 1, -1.0, &r) != CAVMD_ERR_INVALID_VALUE
                || cavmd_recorder_create(ws, 1, &it, ((size_t)1 << 23) + 1, 1, 3.167e-6, &r) != CAVMD_ERR_CAPACITY || r != NULL)
                return 20;
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no recorder\n");
        else
            return 21;
    }
    printf("RECORDER-ABI-OK\n");
    return 0;
}
