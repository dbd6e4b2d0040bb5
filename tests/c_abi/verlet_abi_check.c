/* verlet_abi_check.c -- the integrator part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it with
 * -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_verlet_item, cavmd_verlet_input and
 * cavmd_verlet_state as "name offset" lines for the test to compare with the ctypes structures, and checks the per-item
 * validation, the input row maker (host arithmetic) and that every entry point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_verlet_##which, field)

int main(void)
{
    cavmd_verlet_item it;
    cavmd_verlet_input row;
    cavmd_verlet_state st;
    cavmd_verlet* v = NULL;
    const cavmd_verlet_state* dp = NULL;
    const double u[3] = {0.25, -0.5, 0.75};
    ABI_SIZE(item, cavmd_verlet_item);
    ABI_SIZE(input, cavmd_verlet_input);
    ABI_SIZE(state, cavmd_verlet_state);
    OFF(item, d_pos);
    OFF(item, d_image);
    OFF(item, d_vel);
    OFF(item, d_accel);
    OFF(item, d_force);
    OFF(item, d_net_force);
    OFF(item, Lx);
    OFF(item, Ly);
    OFF(item, Lz);
    OFF(item, N);
    OFF(item, langevin_index);
    OFF(item, reserved);
    OFF(input, dt);
    OFF(input, langevin_gamma);
    OFF(input, langevin_coeff);
    OFF(input, uniform);
    OFF(input, skip);
    OFF(input, reserved);
    OFF(state, steps);
    OFF(state, out_of_box);
    OFF(state, langevin_reservoir);
    OFF(state, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    memset(&it, 0, sizeof(it));
    it.langevin_index = -1;
    if (cavmd_verlet_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_verlet_item_check(&it) != CAVMD_OK) /* N == 0: every array may be NULL */
        return 6;
    it.N = 10;
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* particles without arrays */
        return 7;
    it.d_pos = (cavmd_double4*)(uintptr_t)0x1000;
    it.d_image = (cavmd_int3*)(uintptr_t)0x2004;
    it.d_vel = (cavmd_double4*)(uintptr_t)0x3000;
    it.d_accel = (double*)(uintptr_t)0x4008;
    it.d_force[0] = (const cavmd_double4*)(uintptr_t)0x5000;
    if (cavmd_verlet_item_check(&it) != CAVMD_OK)
        return 8;
    it.d_force[2] = (const cavmd_double4*)(uintptr_t)0x6000; /* after a NULL one */
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it.d_force[2] = NULL;
    it.d_accel = (double*)(uintptr_t)0x4004;
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_accel = (double*)(uintptr_t)0x4008;
    it.langevin_index = 10;
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.langevin_index = 9;
    if (cavmd_verlet_item_check(&it) != CAVMD_OK)
        return 12;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 13;
    it.N = 10;
    it.reserved[1] = 1;
    if (cavmd_verlet_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.reserved[1] = 0;
    /* the input row */
    if (cavmd_verlet_input_make(0.5, 0.1, 2.0, u, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_input_make(0.5, 0.1, 2.0, NULL, &row) != CAVMD_ERR_INVALID_VALUE)
        return 15;
    memset(&row, 0xff, sizeof(row));
    if (cavmd_verlet_input_make(0.5, 0.1, 2.0, u, &row) != CAVMD_OK || row.dt != 0.5 || row.langevin_gamma != 0.1
        || row.langevin_coeff != sqrt(6.0 * 0.1 * 2.0 / 0.5) || row.uniform[0] != 0.25 || row.uniform[1] != -0.5
        || row.uniform[2] != 0.75 || row.skip != 0 || row.reserved != 0)
        return 16;
    if (cavmd_verlet_input_make(0.5, 0.0, 2.0, u, &row) != CAVMD_OK || row.langevin_coeff != 0.0 || row.skip != 0)
        return 17;
    if (cavmd_verlet_input_make(0.0, 0.1, 2.0, u, &row) != CAVMD_OK || row.skip == 0)
        return 18;
    /* null handles are refused before anything else */
    if (cavmd_verlet_create(NULL, 1, &it, &v) != CAVMD_ERR_INVALID_VALUE || v != NULL)
        return 20;
    if (cavmd_verlet_create(NULL, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 21;
    if (cavmd_verlet_destroy(NULL) != CAVMD_OK)
        return 22;
    if (cavmd_verlet_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_accelerations(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_step_one(NULL, NULL, (const cavmd_verlet_input*)(uintptr_t)0x1000) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_step_two(NULL, NULL, (const cavmd_verlet_input*)(uintptr_t)0x1000) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_read(NULL, NULL, &st) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_verlet_state_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
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
            printf("no device: no workspace, hence no integrator batch\n");
        else
            return 24;
    }
    printf("VERLET-ABI-OK\n");
    return 0;
}
