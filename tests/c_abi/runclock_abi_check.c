/* runclock_abi_check.c -- the run clock's part of include/cavmd.h consumed as plain C99 (tests/test_runclock_abi.py builds it
 * with -pedantic -Werror and runs it).  Needs no GPU: it calls every cavmd_runclock_* prototype with a null handle, which each
 * refuses before anything else is looked at, and checks that a refused call writes nothing. */
#include "abi_print.h"
#include "cavmd.h"

int main(void)
{
    const double t_end[2] = {1.0, 2.0};
    uint64_t n = 7;
    ABI_SIZE(draw_state, cavmd_draw_state);
    ABI_OFF(draw_state, cavmd_draw_state, elapsed);
    ABI_OFF(draw_state, cavmd_draw_state, reserved);
    if (cavmd_runclock_draw_set_end(NULL, 0, 2, t_end) != CAVMD_ERR_INVALID_VALUE)
        return 3;
    if (cavmd_runclock_draw_finished(NULL, NULL, &n) != CAVMD_ERR_INVALID_VALUE || n != 7)
        return 4;
    if (cavmd_runclock_ledger_set_rule(NULL, 1.0, 0.0) != CAVMD_ERR_INVALID_VALUE
        || cavmd_runclock_ledger_set_rule(NULL, 0.0, 0.0) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    if (cavmd_runclock_field_set_rule(NULL, t_end, 8, 1.0, 0.0) != CAVMD_ERR_INVALID_VALUE)
        return 7;
    if (cavmd_version() != 2)
        return 6;
    printf("RUNCLOCK-ABI-OK\n");
    return 0;
}
