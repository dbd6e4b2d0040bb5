/* bath_abi_check.c -- the bath part of include/cavmd.h consumed as plain C99 (tests/test_bath_abi.py builds it with -pedantic
 * -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_bath_item and cavmd_bath_state as "name offset" lines for
 * the test to compare with the ctypes structures, and checks the per-item validation (host arithmetic) and that every entry
 * point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_bath_##which, field)

int main(void)
{
    cavmd_bath_item it;
    cavmd_bath_state st;
    cavmd_bath* b = NULL;
    const cavmd_bath_state* dp = NULL;
    cavmd_verlet_input* rows = (cavmd_verlet_input*)(uintptr_t)0x1000;
    ABI_SIZE(item, cavmd_bath_item);
    ABI_SIZE(state, cavmd_bath_state);
    OFF(item, d_gamma);
    OFF(item, seed);
    OFF(item, kT);
    OFF(item, N);
    OFF(item, reserved0);
    OFF(item, reserved);
    OFF(state, draws);
    OFF(state, coupled);
    OFF(state, reservoir);
    OFF(state, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    memset(&it, 0, sizeof(it));
    if (cavmd_bath_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_bath_item_check(&it) != CAVMD_OK) /* d_gamma NULL with N == 0: no bath on this item */
        return 6;
    it.N = 5;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* NULL with N != 0 */
        return 7;
    it.d_gamma = (const double*)(uintptr_t)0x2000;
    if (cavmd_bath_item_check(&it) != CAVMD_OK)
        return 8;
    it.N = 0;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* non-NULL with N == 0 */
        return 9;
    it.N = 5;
    it.d_gamma = (const double*)(uintptr_t)0x2004;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_gamma = (const double*)(uintptr_t)0x2008;
    it.kT = -1.0;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.kT = HUGE_VAL;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    it.kT = 1e-3;
    it.reserved0 = 1;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.reserved0 = 0;
    it.reserved[3] = 1;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.reserved[3] = 0;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_bath_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 15;
    it.N = CAVMD_BATCH_MAX_ITEM_N;
    it.seed = UINT64_MAX;
    if (cavmd_bath_item_check(&it) != CAVMD_OK)
        return 16;
    /* null handles are refused before anything else */
    if (cavmd_bath_create(NULL, 1, &it, &b) != CAVMD_ERR_INVALID_VALUE || b != NULL)
        return 20;
    if (cavmd_bath_create(NULL, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 21;
    if (cavmd_bath_destroy(NULL) != CAVMD_OK)
        return 22;
    if (cavmd_bath_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE || cavmd_bath_step_two(NULL, NULL, rows) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bath_read(NULL, NULL, &st) != CAVMD_ERR_INVALID_VALUE || cavmd_bath_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bath_state_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
        return 23;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no integrator and no bath\n");
        else
            return 24;
    }
    printf("BATH-ABI-OK\n");
    return 0;
}
