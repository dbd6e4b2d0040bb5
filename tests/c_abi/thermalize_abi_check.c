/* thermalize_abi_check.c -- the thermalize part of include/cavmd.h consumed as plain C99 (tests/test_thermalize_abi.py builds it
 * with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_thermalize_item and cavmd_thermalize_state
 * as "name offset" lines for the test to compare with the ctypes structures, and checks the per-item validation (host
 * arithmetic) and that every entry point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_thermalize_##which, field)

static cavmd_thermalize_item good(void)
{
    cavmd_thermalize_item it;
    memset(&it, 0, sizeof(it));
    it.d_vel = (cavmd_double4*)(uintptr_t)0x10000;
    it.d_pos = (cavmd_double4*)(uintptr_t)0x20000;
    it.d_image = (cavmd_int3*)(uintptr_t)0x30004;
    it.d_result = (const cavmd_result*)(uintptr_t)0x40008;
    it.seed = UINT64_MAX;
    it.kT = 1e-3;
    it.N = 501;
    it.flags = CAVMD_THERMALIZE_ZERO_MOMENTUM | CAVMD_THERMALIZE_PLACE_PHOTON | CAVMD_THERMALIZE_FINITE_Q
               | CAVMD_THERMALIZE_PHOTON_VELOCITY;
    it.L[0] = 40.0;
    it.L[1] = 41.0;
    it.L[2] = 42.0;
    it.params = cavmd_make_params(0.0091, 1e-3, 1.0);
    return it;
}

int main(void)
{
    cavmd_thermalize_item it;
    cavmd_thermalize_state st;
    cavmd_thermalize* t = NULL;
    const cavmd_thermalize_state* dp = NULL;
    ABI_SIZE(item, cavmd_thermalize_item);
    ABI_SIZE(state, cavmd_thermalize_state);
    OFF(item, d_vel);
    OFF(item, d_members);
    OFF(item, d_pos);
    OFF(item, d_image);
    OFF(item, d_result);
    OFF(item, seed);
    OFF(item, kT);
    OFF(item, N);
    OFF(item, n_members);
    OFF(item, flags);
    OFF(item, reserved0);
    OFF(item, L);
    OFF(item, params);
    OFF(item, reserved);
    OFF(state, draws);
    OFF(state, thermalised);
    OFF(state, skipped);
    OFF(state, momentum);
    OFF(state, photon);
    OFF(state, reserved0);
    OFF(state, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    if (CAVMD_THERMALIZE_ZERO_MOMENTUM != 1u || CAVMD_THERMALIZE_PLACE_PHOTON != 2u || CAVMD_THERMALIZE_FINITE_Q != 4u
        || CAVMD_THERMALIZE_PHOTON_VELOCITY != 8u || CAVMD_THERMALIZE_TILE != 512u)
        return 3;
    if (cavmd_thermalize_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    memset(&it, 0, sizeof(it));
    if (cavmd_thermalize_item_check(&it) != CAVMD_OK) /* N == 0: nothing of the item is touched */
        return 6;
    it = good();
    if (cavmd_thermalize_item_check(&it) != CAVMD_OK)
        return 7;
    it.d_vel = NULL;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* d_vel is required */
        return 8;
    it = good();
    it.d_vel = (cavmd_double4*)(uintptr_t)0x10008;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it = good();
    it.d_result = (const cavmd_result*)(uintptr_t)0x40004;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it = good();
    it.kT = -1.0;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.kT = HUGE_VAL;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    it = good();
    it.reserved0 = 1;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it = good();
    it.reserved[3] = 1;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it = good();
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 15;
    it.N = CAVMD_BATCH_MAX_ITEM_N;
    if (cavmd_thermalize_item_check(&it) != CAVMD_OK)
        return 16;
    it = good();
    it.d_result = NULL; /* the displaced start and the placement need the result block */
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 17;
    it.flags = CAVMD_THERMALIZE_ZERO_MOMENTUM | CAVMD_THERMALIZE_PHOTON_VELOCITY;
    if (cavmd_thermalize_item_check(&it) != CAVMD_OK)
        return 18;
    it = good();
    it.flags |= 16u;
    if (cavmd_thermalize_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 19;
    /* null handles are refused before anything else */
    it = good();
    if (cavmd_thermalize_create(NULL, 1, &it, &t) != CAVMD_ERR_INVALID_VALUE || t != NULL)
        return 20;
    if (cavmd_thermalize_create(NULL, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 21;
    if (cavmd_thermalize_destroy(NULL) != CAVMD_OK)
        return 22;
    if (cavmd_thermalize_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE || cavmd_thermalize_run(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_thermalize_read(NULL, NULL, &st) != CAVMD_ERR_INVALID_VALUE
        || cavmd_thermalize_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_thermalize_state_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
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
            printf("no device: no workspace, hence no thermalize object\n");
        else
            return 24;
    }
    printf("THERMALIZE-ABI-OK\n");
    return 0;
}
