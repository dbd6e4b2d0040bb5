/* batch_abi_check.c -- the batch part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it with
 * -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_batch_item and cavmd_params for the test to
 * compare with the ctypes structures, and checks the per-item validation (cavmd_batch_item_check is host arithmetic) and that
 * every entry point refuses null arguments. */
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, type, field) ABI_OFF(which, cavmd_##type, field)

int main(void)
{
    cavmd_batch_item it;
    cavmd_batch* b = NULL;
    cavmd_result r;
    const cavmd_result* dp = NULL;
    uint64_t seq = 0;
    double e[3];
    ABI_SIZE(item, cavmd_batch_item);
    ABI_SIZE(params, cavmd_params);
    OFF(item, batch_item, d_pos);
    OFF(item, batch_item, d_charge);
    OFF(item, batch_item, d_image);
    OFF(item, batch_item, d_force);
    OFF(item, batch_item, Lx);
    OFF(item, batch_item, Ly);
    OFF(item, batch_item, Lz);
    OFF(item, batch_item, params);
    OFF(item, batch_item, N);
    OFF(item, batch_item, L_typeid);
    OFF(item, batch_item, reserved);
    OFF(params, params, omegac);
    OFF(params, params, couplstr);
    OFF(params, params, K);
    OFF(params, params, phmass);
    if (CAVMD_BATCH_MAX_ITEMS != 65536 || CAVMD_BATCH_MAX_ITEM_N != 65536)
        return 2;
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 3;
    memset(&it, 0, sizeof(it));
    if (cavmd_batch_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 4;
    if (cavmd_batch_item_check(&it) != CAVMD_OK) /* N == 0: the arrays may be NULL */
        return 5;
    it.N = 10;
    if (cavmd_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* N > 0 with null arrays */
        return 6;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1000;
    it.d_charge = (const double*)(uintptr_t)0x2000;
    it.d_image = (const cavmd_int3*)(uintptr_t)0x3000;
    it.d_force = (cavmd_double4*)(uintptr_t)0x4000;
    it.Lx = it.Ly = it.Lz = 10.0;
    if (cavmd_batch_item_check(&it) != CAVMD_ERR_BAD_PARAMS) /* K == 0 */
        return 7;
    it.params = cavmd_make_params(0.0091, 1e-3, 1.0);
    if (cavmd_batch_item_check(&it) != CAVMD_OK)
        return 8;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_batch_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 9;
    it.N = 10;
    it.reserved[3] = 1;
    if (cavmd_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.reserved[3] = 0;
    /* null handles are refused before anything else */
    if (cavmd_batch_create(NULL, 1, &it, 4, &b) != CAVMD_ERR_INVALID_VALUE || b != NULL)
        return 11;
    if (cavmd_batch_create(NULL, 1, &it, 4, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    if (cavmd_batch_destroy(NULL) != CAVMD_OK)
        return 13;
    if (cavmd_batch_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE || cavmd_batch_compute(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_batch_last_sequence(NULL, &seq) != CAVMD_ERR_INVALID_VALUE
        || cavmd_batch_results_read(NULL, &r) != CAVMD_ERR_INVALID_VALUE
        || cavmd_batch_results_at(NULL, 1, &r) != CAVMD_ERR_INVALID_VALUE
        || cavmd_batch_energies_at(NULL, 1, e) != CAVMD_ERR_INVALID_VALUE
        || cavmd_batch_results_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    {
        cavmd_workspace* ws = NULL;
        const int st = cavmd_create(-1, 1000, &ws);
        if (st == CAVMD_OK)
        {
            /* a device is present: the table-level refusals of create */
            if (cavmd_batch_create(ws, 0, &it, 4, &b) != CAVMD_ERR_INVALID_VALUE)
                return 15;
            if (cavmd_batch_create(ws, 1, &it, 1, &b) != CAVMD_ERR_INVALID_VALUE)
                return 16;
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (st == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no batch\n");
        else
            return 17;
    }
    printf("BATCH-ABI-OK\n");
    return 0;
}
