/* shared_cavity_abi_check.c -- the shared cavity of include/cavmd.h consumed as plain C99 (tests/test_shared_cavity_abi.py
 * builds it with -pedantic -Werror and runs it).  Needs no GPU: it prints the item's layout and the cap as the C compiler sees
 * them, runs the table rules on host tables and calls every prototype that takes a handle with a null one. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

static cavmd_shared_cavity_item member(uint32_t cavity, int carrier)
{
    cavmd_shared_cavity_item it;
    memset(&it, 0, sizeof(it));
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x10000;
    it.d_charge = (const double*)(uintptr_t)0x20000;
    it.d_image = (const cavmd_int3*)(uintptr_t)0x30000;
    it.d_force = (cavmd_double4*)(uintptr_t)0x40000;
    it.Lx = it.Ly = it.Lz = 20.0;
    it.params = cavmd_make_params(0.0091, 1e-3, 1.0);
    it.N = 8;
    it.L_typeid = carrier ? 2 : -1;
    it.cavity = cavity;
    return it;
}

int main(void)
{
    cavmd_shared_cavity_item t[4];
    cavmd_shared_cavity_item* big;
    cavmd_shared_cavity* obj = (cavmd_shared_cavity*)(uintptr_t)1;
    cavmd_result res;
    const cavmd_result* d_res = NULL;
    const double* d_cell = NULL;
    uint64_t seq = 0;
    uint32_t n = 99, item = 0;
    int k;

    ABI_SIZE(item, cavmd_shared_cavity_item);
    ABI_OFF(item, cavmd_shared_cavity_item, d_pos);
    ABI_OFF(item, cavmd_shared_cavity_item, d_charge);
    ABI_OFF(item, cavmd_shared_cavity_item, d_image);
    ABI_OFF(item, cavmd_shared_cavity_item, d_force);
    ABI_OFF(item, cavmd_shared_cavity_item, Lx);
    ABI_OFF(item, cavmd_shared_cavity_item, Ly);
    ABI_OFF(item, cavmd_shared_cavity_item, Lz);
    ABI_OFF(item, cavmd_shared_cavity_item, params);
    ABI_OFF(item, cavmd_shared_cavity_item, N);
    ABI_OFF(item, cavmd_shared_cavity_item, L_typeid);
    ABI_OFF(item, cavmd_shared_cavity_item, cavity);
    ABI_OFF(item, cavmd_shared_cavity_item, reserved0);
    ABI_OFF(item, cavmd_shared_cavity_item, reserved);
    printf("CAVMD_SHARED_CAVITY_MAX_MEMBERS %d\n", CAVMD_SHARED_CAVITY_MAX_MEMBERS);

    /* two cavities of two members, interleaved */
    t[0] = member(0, 1); t[1] = member(1, 0); t[2] = member(0, 0); t[3] = member(1, 1);
    if (cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_OK || n != 2)
        return 3;
    if (cavmd_shared_cavity_table_check(4, t, NULL) != CAVMD_OK || cavmd_shared_cavity_item_check(&t[0]) != CAVMD_OK)
        return 4;
    t[2].L_typeid = 2; /* two carriers */
    if (cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    t[2].L_typeid = -1;
    t[3].L_typeid = -1; /* none */
    if (cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_ERR_INVALID_VALUE)
        return 6;
    t[3].L_typeid = 2;
    t[1].cavity = t[3].cavity = 2; /* sparse ids */
    if (cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_ERR_INVALID_VALUE)
        return 7;
    t[1].cavity = t[3].cavity = 1;
    t[2].params.couplstr = 2e-3; /* differing params */
    if (cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_ERR_BAD_PARAMS)
        return 8;
    t[2] = member(0, 0);
    t[2].reserved[1] = 1;
    if (cavmd_shared_cavity_item_check(&t[2]) != CAVMD_ERR_INVALID_VALUE || cavmd_shared_cavity_item_check(NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_table_check(4, t, &n) != CAVMD_ERR_INVALID_VALUE || cavmd_shared_cavity_table_check(0, t, &n) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_table_check(4, NULL, &n) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    if (n != 2) /* written for a table that passes only */
        return 10;

    /* the cap: 1024 members pass, the 1025th is refused */
    big = (cavmd_shared_cavity_item*)malloc(sizeof(*big) * (CAVMD_SHARED_CAVITY_MAX_MEMBERS + 1));
    if (!big)
        return 11;
    for (k = 0; k <= CAVMD_SHARED_CAVITY_MAX_MEMBERS; ++k)
        big[k] = member(0, k == 17);
    if (cavmd_shared_cavity_table_check(CAVMD_SHARED_CAVITY_MAX_MEMBERS, big, &n) != CAVMD_OK || n != 1)
        return 12;
    if (cavmd_shared_cavity_table_check(CAVMD_SHARED_CAVITY_MAX_MEMBERS + 1, big, &n) != CAVMD_ERR_CAPACITY)
        return 13;
    free(big);

    /* null handles; without a workspace there is no object */
    t[2] = member(0, 0);
    if (cavmd_shared_cavity_create(NULL, 4, t, &obj) != CAVMD_ERR_INVALID_VALUE || obj != NULL)
        return 14;
    if (cavmd_shared_cavity_create(NULL, 4, t, NULL) != CAVMD_ERR_INVALID_VALUE || cavmd_shared_cavity_destroy(NULL) != CAVMD_OK)
        return 15;
    if (cavmd_shared_cavity_set_items(NULL, 0, 1, t) != CAVMD_ERR_INVALID_VALUE || cavmd_shared_cavity_compute(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_last_sequence(NULL, &seq) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_results_read(NULL, NULL, &res) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_results_device_ptr(NULL, &d_res) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_cell_dipoles_device_ptr(NULL, &d_cell) != CAVMD_ERR_INVALID_VALUE
        || cavmd_shared_cavity_count(NULL, &n) != CAVMD_ERR_INVALID_VALUE || cavmd_shared_cavity_carrier(NULL, 0, &item) != CAVMD_ERR_INVALID_VALUE)
        return 16;
    if (cavmd_version() != 2)
        return 17;
    printf("SHARED-CAVITY-ABI-OK\n");
    return 0;
}
