/* molecular_abi_check.c -- the molecular-force part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds
 * it with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_molecular_pair, _bond_params, _params,
 * _bond and _item as "name offset" lines for the test to compare with the ctypes structures, and checks the pair maker, the two
 * validations (host arithmetic) and that every entry point refuses null arguments. */
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_molecular_##which, field)

int main(void)
{
    static cavmd_molecular_params prm;
    cavmd_molecular_pair pair;
    cavmd_molecular_item it;
    cavmd_molecular_bond bonds[2];
    cavmd_molecular* m = NULL;
    int rows = 0, split = 0;
    ABI_SIZE(pair, cavmd_molecular_pair);
    ABI_SIZE(bond_params, cavmd_molecular_bond_params);
    ABI_SIZE(params, cavmd_molecular_params);
    ABI_SIZE(bond, cavmd_molecular_bond);
    ABI_SIZE(item, cavmd_molecular_item);
    OFF(pair, lj1);
    OFF(pair, lj2);
    OFF(pair, lj1_12);
    OFF(pair, lj2_6);
    OFF(pair, rcutsq);
    OFF(pair, eshift);
    OFF(pair, reserved);
    OFF(bond_params, K);
    OFF(bond_params, r0);
    OFF(params, n_types);
    OFF(params, n_bond_types);
    OFF(params, reserved);
    OFF(params, pair);
    OFF(params, bond);
    OFF(bond, a);
    OFF(bond, b);
    OFF(bond, type);
    OFF(item, d_pos);
    OFF(item, d_force);
    OFF(item, h_bonds);
    OFF(item, Lx);
    OFF(item, Ly);
    OFF(item, Lz);
    OFF(item, N);
    OFF(item, n_bonds);
    OFF(item, reserved);
    printf("limits %d %d %d %d %d\n", CAVMD_MOLECULAR_MAX_ITEM_N, CAVMD_MOLECULAR_MAX_TYPES, CAVMD_MOLECULAR_MAX_BOND_TYPES,
           CAVMD_MOLECULAR_MAX_BONDS, CAVMD_MOLECULAR_J_SPLIT);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    if (cavmd_molecular_order(&rows, &split) != CAVMD_OK || rows * split != 256 || split != CAVMD_MOLECULAR_J_SPLIT
        || cavmd_molecular_order(NULL, NULL) != CAVMD_OK)
        return 5;
    printf("order %d %d\n", rows, split);
    /* the pair maker */
    if (cavmd_molecular_pair_make(1.0, 1.0, 3.0, 1, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_molecular_pair_make(-1.0, 1.0, 3.0, 1, &pair) != CAVMD_ERR_INVALID_VALUE)
        return 6;
    memset(&pair, 0xff, sizeof(pair));
    if (cavmd_molecular_pair_make(0.5, 2.0, 4.0, 0, &pair) != CAVMD_OK || pair.lj2 != 128.0 || pair.lj1 != 8192.0
        || pair.lj1_12 != 98304.0 || pair.lj2_6 != 768.0 || pair.rcutsq != 16.0 || pair.eshift != 0.0 || pair.reserved[0] != 0
        || pair.reserved[1] != 0)
        return 7;
    if (cavmd_molecular_pair_make(0.5, 2.0, 4.0, 1, &pair) != CAVMD_OK || pair.eshift != (1.0 / 4096.0) * (8192.0 / 4096.0 - 128.0))
        return 8;
    /* parameters */
    memset(&prm, 0, sizeof(prm));
    if (cavmd_molecular_params_check(NULL) != CAVMD_ERR_INVALID_VALUE || cavmd_molecular_params_check(&prm) != CAVMD_OK)
        return 9;
    prm.n_types = 2;
    prm.n_bond_types = 1;
    prm.bond[0].K = 0.7;
    prm.bond[0].r0 = 2.2;
    prm.pair[0][1] = pair;
    if (cavmd_molecular_params_check(&prm) != CAVMD_ERR_INVALID_VALUE) /* asymmetric */
        return 10;
    prm.pair[1][0] = pair;
    if (cavmd_molecular_params_check(&prm) != CAVMD_OK)
        return 11;
    prm.n_types = 9;
    if (cavmd_molecular_params_check(&prm) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    prm.n_types = 2;
    /* items */
    memset(&it, 0, sizeof(it));
    if (cavmd_molecular_item_check(&prm, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_molecular_item_check(NULL, &it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_OK) /* N == 0: every array may be NULL */
        return 14;
    it.N = 10;
    it.Lx = it.Ly = it.Lz = 8.0;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE) /* particles without arrays */
        return 15;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1000;
    it.d_force = (cavmd_double4*)(uintptr_t)0x2000;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_OK) /* r_cut = 4 = L / 2 */
        return 16;
    it.Lz = 7.9;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE) /* r_cut above min(L) / 2 */
        return 17;
    it.Lz = 8.0;
    bonds[0].a = 0;
    bonds[0].b = 1;
    bonds[0].type = 0;
    bonds[1].a = 1;
    bonds[1].b = 9;
    bonds[1].type = 0;
    it.h_bonds = bonds;
    it.n_bonds = 2;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_OK)
        return 18;
    bonds[1].b = 10;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE) /* index not below N */
        return 19;
    bonds[1].b = 1;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE) /* a == b */
        return 20;
    bonds[1].b = 9;
    bonds[1].type = 1;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE) /* bond type not below n_bond_types */
        return 21;
    bonds[1].type = 0;
    it.N = CAVMD_MOLECULAR_MAX_ITEM_N + 1u;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_CAPACITY)
        return 22;
    it.N = 10;
    it.reserved = 1;
    if (cavmd_molecular_item_check(&prm, &it) != CAVMD_ERR_INVALID_VALUE)
        return 23;
    it.reserved = 0;
    /* null handles are refused before anything else */
    if (cavmd_molecular_create(NULL, &prm, 1, &it, &m) != CAVMD_ERR_INVALID_VALUE || m != NULL)
        return 24;
    if (cavmd_molecular_create(NULL, &prm, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 25;
    if (cavmd_molecular_destroy(NULL) != CAVMD_OK)
        return 26;
    if (cavmd_molecular_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_molecular_compute(NULL, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 27;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no molecular batch\n");
        else
            return 28;
    }
    printf("MOLECULAR-ABI-OK\n");
    return 0;
}
