/* draw_abi_check.c -- the draw part of include/cavmd.h consumed as plain C99 (tests/test_draw_abi.py builds it with -pedantic
 * -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_draw_item and cavmd_draw_state as "name offset" lines for
 * the test to compare with the ctypes structures, and checks the per-item validation (host arithmetic) and that every entry
 * point refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_draw_##which, field)

int main(void)
{
    cavmd_draw_item it;
    cavmd_draw_state st;
    cavmd_draw* d = NULL;
    const cavmd_draw_state* dp = NULL;
    ABI_SIZE(item, cavmd_draw_item);
    ABI_SIZE(state, cavmd_draw_state);
    OFF(item, d_verlet_row);
    OFF(item, d_bussi_row);
    OFF(item, d_records);
    OFF(item, d_rows);
    OFF(item, capacity);
    OFF(item, langevin_gamma);
    OFF(item, langevin_kT);
    OFF(item, bussi_set_T);
    OFF(item, bussi_tau);
    OFF(item, bussi_dof);
    OFF(item, dt_initial);
    OFF(item, tolerance_target);
    OFF(item, tolerance_initial);
    OFF(item, tolerance_time_constant);
    OFF(item, dt_min);
    OFF(item, dt_max);
    OFF(item, reserved);
    OFF(state, draws);
    OFF(state, dt);
    OFF(state, elapsed);
    OFF(state, tolerance);
    OFF(state, exhausted);
    OFF(state, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 4;
    memset(&it, 0, sizeof(it));
    if (cavmd_draw_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* both destinations NULL */
        return 6;
    it.d_verlet_row = (cavmd_verlet_input*)(uintptr_t)0x1000;
    if (cavmd_draw_item_check(&it) != CAVMD_OK) /* a fixed dt of 0: every step is skipped, which is legal */
        return 7;
    it.d_verlet_row = NULL;
    it.d_bussi_row = (cavmd_bussi_batch_input*)(uintptr_t)0x2008;
    if (cavmd_draw_item_check(&it) != CAVMD_OK)
        return 8;
    it.d_bussi_row = (cavmd_bussi_batch_input*)(uintptr_t)0x2004;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    it.d_bussi_row = (cavmd_bussi_batch_input*)(uintptr_t)0x2000;
    it.d_records = (const cavmd_record*)(uintptr_t)0x3000; /* without a row counter, with capacity 0 */
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 10;
    it.d_rows = (const uint64_t*)(uintptr_t)0x4000;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* capacity 0 */
        return 11;
    it.capacity = 8;
    if (cavmd_draw_item_check(&it) != CAVMD_OK)
        return 12;
    it.dt_min = 2.0;
    it.dt_max = 1.0;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.dt_max = 2.0;
    it.bussi_tau = -1.0;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.bussi_tau = 1.0;
    it.tolerance_target = HUGE_VAL;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 15;
    it.tolerance_target = 1e-3;
    it.reserved[3] = 1;
    if (cavmd_draw_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 16;
    it.reserved[3] = 0;
    if (cavmd_draw_item_check(&it) != CAVMD_OK)
        return 17;
    /* null handles are refused before anything else */
    if (cavmd_draw_create(NULL, 1, 1, &it, &d) != CAVMD_ERR_INVALID_VALUE || d != NULL)
        return 20;
    if (cavmd_draw_create(NULL, 1, 1, &it, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 21;
    if (cavmd_draw_destroy(NULL) != CAVMD_OK)
        return 22;
    if (cavmd_draw_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE || cavmd_draw_fill(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_draw_read(NULL, NULL, &st) != CAVMD_ERR_INVALID_VALUE || cavmd_draw_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_draw_state_device_ptr(NULL, &dp) != CAVMD_ERR_INVALID_VALUE)
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
            printf("no device: no workspace, hence no draw object\n");
        else
            return 24;
    }
    printf("DRAW-ABI-OK\n");
    return 0;
}
