/* bussi_batch_abi_check.c -- the thermostat-batch part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py
 * builds it with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_bussi_batch_item,
 * cavmd_bussi_batch_input and cavmd_bussi_device_state for the test to compare with the ctypes structures, and checks the
 * per-item validation and the input row maker (host arithmetic), and that every entry point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, type, field) ABI_OFF(which, cavmd_bussi_##type, field)

int main(void)
{
    cavmd_bussi_batch_item it;
    cavmd_bussi_batch_input row;
    cavmd_bussi_batch* b = NULL;
    cavmd_bussi_device_state st;
    const cavmd_bussi_device_state* dp = NULL;
    uint64_t seq = 0;
    ABI_SIZE(item, cavmd_bussi_batch_item);
    ABI_SIZE(input, cavmd_bussi_batch_input);
    ABI_SIZE(state, cavmd_bussi_device_state);
    OFF(item, batch_item, d_vel);
    OFF(item, batch_item, d_members);
    OFF(item, batch_item, n_members);
    OFF(item, batch_item, reserved0);
    OFF(item, batch_item, dof_translational);
    OFF(item, batch_item, reserved);
    OFF(input, batch_input, normal_variate);
    OFF(input, batch_input, gamma_variate);
    OFF(input, batch_input, c);
    OFF(input, batch_input, set_T);
    OFF(input, batch_input, skip);
    OFF(input, batch_input, reserved);
    OFF(state, device_state, reservoir_translational);
    OFF(state, device_state, instantaneous_translational);
    OFF(state, device_state, last_alpha);
    OFF(state, device_state, last_kinetic_energy);
    OFF(state, device_state, steps);
    OFF(state, device_state, refused);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    memset(&it, 0, sizeof(it));
    if (cavmd_bussi_batch_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_OK) /* n_members == 0: d_vel may be NULL */
        return 6;
    it.n_members = 10;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* members without velocities */
        return 7;
    it.d_vel = (cavmd_double4*)(uintptr_t)0x1000;
    it.dof_translational = 27.0;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_OK)
        return 8;
    it.d_vel = (cavmd_double4*)(uintptr_t)0x1008;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it.d_vel = (cavmd_double4*)(uintptr_t)0x1000;
    it.d_members = (const uint32_t*)(uintptr_t)0x2002;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_members = (const uint32_t*)(uintptr_t)0x2004;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_OK)
        return 11;
    it.n_members = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 12;
    it.n_members = 10;
    it.dof_translational = -1.0;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.dof_translational = 27.0;
    it.reserved0 = 1;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.reserved0 = 0;
    it.reserved[2] = 1;
    if (cavmd_bussi_batch_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 15;
    it.reserved[2] = 0;
    /* the input row: c as cavmd_bussi_step_device takes it, skip iff deltaT == 0 */
    if (cavmd_bussi_batch_input_make(0.005, 1.5, 0.5, 0.25, 3.0, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 16;
    memset(&row, 0xff, sizeof(row));
    if (cavmd_bussi_batch_input_make(0.005, 1.5, 0.5, 0.25, 3.0, &row) != CAVMD_OK || row.c != exp(-0.005 / 0.5)
        || row.set_T != 1.5 || row.normal_variate != 0.25 || row.gamma_variate != 3.0 || row.skip != 0 || row.reserved[0] != 0
        || row.reserved[1] != 0 || row.reserved[2] != 0)
        return 17;
    if (cavmd_bussi_batch_input_make(0.005, 1.5, 0.0, 0.25, 3.0, &row) != CAVMD_OK || row.c != 0.0 || row.skip != 0)
        return 18;
    if (cavmd_bussi_batch_input_make(0.0, 1.5, 0.5, 0.25, 3.0, &row) != CAVMD_OK || row.skip == 0)
        return 19;
    /* null handles are refused before anything else */
    if (cavmd_bussi_batch_create(NULL, 1, &it, &b) != CAVMD_ERR_INVALID_VALUE || b != NULL)
        return 20;
    if (cavmd_bussi_batch_create(NULL, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 21;
    if (cavmd_bussi_batch_destroy(NULL) != CAVMD_OK)
        return 22;
    if (cavmd_bussi_batch_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bussi_batch_step(NULL, NULL, (const cavmd_bussi_batch_input*)(uintptr_t)0x1000) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bussi_batch_last_sequence(NULL, &seq) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bussi_batch_read(NULL, &st) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bussi_batch_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_bussi_batch_state_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
        return 23;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            if (cavmd_bussi_batch_create(ws, 0, &it, &b) != CAVMD_ERR_INVALID_VALUE)
                return 24;
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no batch\n");
        else
            return 25;
    }
    printf("BUSSI-BATCH-ABI-OK\n");
    return 0;
}
