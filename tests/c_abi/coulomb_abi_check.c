/* coulomb_abi_check.c -- the Coulomb part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it with
 * -pedantic -Werror and runs it).  Needs no GPU: it prints the layout of cavmd_coulomb_item as "name offset" lines for the test
 * to compare with the ctypes structure, and checks the host arithmetic (item check, k count, parameters) and that every entry
 * point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(field) ABI_OFF(item, cavmd_coulomb_item, field)

int main(void)
{
    cavmd_coulomb_item it;
    cavmd_molecular_bond ex[2];
    cavmd_coulomb* c = NULL;
    const double* structure = NULL;
    const uint32_t* offsets = NULL;
    uint32_t K = 77;
    double kappa = 0.0, k_cut = 0.0;
    int rows = 0, split = 0, k_rows = 0, k_split = 0;
    ABI_SIZE(item, cavmd_coulomb_item);
    OFF(d_pos);
    OFF(d_charge);
    OFF(d_force);
    OFF(h_exclusions);
    OFF(Lx);
    OFF(Ly);
    OFF(Lz);
    OFF(kappa);
    OFF(r_cut);
    OFF(k_cut);
    OFF(N);
    OFF(n_exclusions);
    OFF(reserved);
    printf("limits %d %d %d %d %d\n", CAVMD_COULOMB_MAX_ITEM_N, CAVMD_COULOMB_MAX_K, CAVMD_COULOMB_MAX_EXCLUSIONS,
           CAVMD_COULOMB_J_SPLIT, CAVMD_COULOMB_K_SPLIT);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    if (cavmd_coulomb_order(&rows, &split, &k_rows, &k_split) != CAVMD_OK || rows * split != 256 || k_rows * k_split != 256
        || split != CAVMD_COULOMB_J_SPLIT || k_split != CAVMD_COULOMB_K_SPLIT
        || cavmd_coulomb_order(NULL, NULL, NULL, NULL) != CAVMD_OK)
        return 5;
    printf("order %d %d %d %d\n", rows, split, k_rows, k_split);
    /* parameters */
    if (cavmd_coulomb_parameters(2.0, 1e-6, NULL, &k_cut) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_parameters(2.0, 1e-6, &kappa, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_parameters(0.0, 1e-6, &kappa, &k_cut) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_parameters(2.0, 1.0, &kappa, &k_cut) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_parameters(2.0, 0.0, &kappa, &k_cut) != CAVMD_ERR_INVALID_VALUE)
        return 6;
    if (cavmd_coulomb_parameters(2.0, exp(-16.0), &kappa, &k_cut) != CAVMD_OK || fabs(kappa - 2.0) > 1e-15 || fabs(k_cut - 16.0) > 1e-14)
        return 7;
    /* items */
    memset(&it, 0, sizeof(it));
    if (cavmd_coulomb_item_check(NULL) != CAVMD_ERR_INVALID_VALUE || cavmd_coulomb_k_count(NULL, &K) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_k_count(&it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 8;
    if (cavmd_coulomb_item_check(&it) != CAVMD_OK || cavmd_coulomb_k_count(&it, &K) != CAVMD_OK || K != 0) /* N == 0 */
        return 9;
    it.N = 10;
    it.Lx = it.Ly = it.Lz = 8.0;
    it.kappa = 1.0;
    it.r_cut = 4.0;
    it.k_cut = 0.8; /* 2 pi / 8 = 0.785...: the three axis vectors */
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* particles without arrays */
        return 10;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1000;
    it.d_charge = (const double*)(uintptr_t)0x3000;
    it.d_force = (cavmd_double4*)(uintptr_t)0x2000;
    if (cavmd_coulomb_item_check(&it) != CAVMD_OK || cavmd_coulomb_k_count(&it, &K) != CAVMD_OK || K != 3)
        return 11;
    it.Lz = 7.9;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* r_cut above min(L) / 2 */
        return 12;
    it.Lz = 8.0;
    it.kappa = 0.0;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.kappa = 1.0;
    it.k_cut = -1.0;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.k_cut = 1e6;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_CAPACITY || cavmd_coulomb_k_count(&it, &K) != CAVMD_ERR_CAPACITY)
        return 15;
    it.k_cut = 0.8;
    ex[0].a = 0;
    ex[0].b = 1;
    ex[0].type = 99; /* ignored */
    ex[1].a = 1;
    ex[1].b = 9;
    ex[1].type = 0;
    it.h_exclusions = ex;
    it.n_exclusions = 2;
    if (cavmd_coulomb_item_check(&it) != CAVMD_OK)
        return 16;
    ex[1].b = 10;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* index not below N */
        return 17;
    ex[1].b = 1;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* a == b */
        return 18;
    ex[1].b = 9;
    it.N = CAVMD_COULOMB_MAX_ITEM_N + 1u;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 19;
    it.N = 10;
    it.reserved = 1;
    if (cavmd_coulomb_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 20;
    it.reserved = 0;
    /* null handles are refused before anything else */
    if (cavmd_coulomb_create(NULL, 1, &it, &c) != CAVMD_ERR_INVALID_VALUE || c != NULL)
        return 21;
    if (cavmd_coulomb_create(NULL, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 22;
    if (cavmd_coulomb_destroy(NULL) != CAVMD_OK)
        return 23;
    if (cavmd_coulomb_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE || cavmd_coulomb_compute(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_coulomb_structure_device_ptr(NULL, &structure, &offsets) != CAVMD_ERR_INVALID_VALUE)
        return 24;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no Coulomb batch\n");
        else
            return 25;
    }
    printf("COULOMB-ABI-OK\n");
    return 0;
}
