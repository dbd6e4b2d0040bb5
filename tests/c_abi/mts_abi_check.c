/* mts_abi_check.c -- the two parts of the Ewald sum and the kick of include/cavmd.h consumed as plain C99
 * (tests/test_coulomb_parts_abi.py builds it with -pedantic -Werror and runs it).  Needs no GPU: it prints the two constants
 * as the C compiler sees them and calls every cavmd_mts_* prototype with a null handle, which each refuses before anything
 * else is looked at. */
#include <stdio.h>

#include "cavmd.h"

int main(void)
{
    cavmd_double4* const long_force[2] = {NULL, NULL};
    const cavmd_double4* const forces[2] = {NULL, NULL};
    const cavmd_verlet_input rows[2] = {{0.0, 0.0, 0.0, {0.0, 0.0, 0.0}, 0, 0}, {0.0, 0.0, 0.0, {0.0, 0.0, 0.0}, 0, 0}};
    const unsigned both = CAVMD_COULOMB_PART_SHORT | CAVMD_COULOMB_PART_LONG;
    printf("CAVMD_COULOMB_PART_SHORT %u\n", CAVMD_COULOMB_PART_SHORT);
    printf("CAVMD_COULOMB_PART_LONG %u\n", CAVMD_COULOMB_PART_LONG);
    if (cavmd_mts_coulomb_set_long_forces(NULL, 2, long_force) != CAVMD_ERR_INVALID_VALUE)
        return 3;
    if (cavmd_mts_coulomb_compute_parts(NULL, NULL, CAVMD_COULOMB_PART_SHORT) != CAVMD_ERR_INVALID_VALUE
        || cavmd_mts_coulomb_compute_parts(NULL, NULL, CAVMD_COULOMB_PART_LONG) != CAVMD_ERR_INVALID_VALUE
        || cavmd_mts_coulomb_compute_parts(NULL, NULL, both) != CAVMD_ERR_INVALID_VALUE
        || cavmd_mts_coulomb_compute_parts(NULL, NULL, 0u) != CAVMD_ERR_INVALID_VALUE
        || cavmd_mts_coulomb_compute_parts(NULL, NULL, 4u) != CAVMD_ERR_INVALID_VALUE)
        return 4;
    if (cavmd_mts_verlet_kick(NULL, NULL, rows, forces, 0.5) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_version() != 2)
        return 6;
    printf("MTS-ABI-OK\n");
    return 0;
}
