/* field_recorder_abi_check.c -- the field-recorder part of include/cavmd.h consumed as plain C99
 * (tests/batch_objects.py builds it with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of
 * cavmd_field_record and cavmd_field_item as the C compiler sees them, and checks the per-item validation (host arithmetic)
 * and that every entry point refuses null arguments. */
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, field) ABI_OFF(which, cavmd_field_##which, field)

int main(void)
{
    cavmd_field_item it;
    cavmd_field_recorder* r = NULL;
    cavmd_field_record rec;
    const cavmd_field_record* dr = NULL;
    const uint64_t* drows = NULL;
    uint64_t rows = 0;
    uint32_t n_refs = 0;
    double k[3] = {0.0, 0.0, 1.0};
    ABI_SIZE(record, cavmd_field_record);
    ABI_SIZE(item, cavmd_field_item);
    OFF(record, call);
    OFF(record, n_references);
    OFF(record, took_reference);
    OFF(record, rho2);
    OFF(record, reserved);
    OFF(record, F);
    OFF(item, d_position);
    OFF(item, position_stride);
    OFF(item, N);
    OFF(item, reserved0);
    OFF(item, reserved);
    printf("limits %d %d\n", CAVMD_FIELD_MAX_WAVEVECTORS, CAVMD_FIELD_MAX_REFERENCES);
    memset(&it, 0, sizeof(it));
    memset(&rec, 0, sizeof(rec));
    if (cavmd_field_recorder_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 1;
    if (cavmd_field_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* stride 0 */
        return 2;
    it.position_stride = 24;
    if (cavmd_field_recorder_item_check(&it) != CAVMD_OK) /* N = 0 with a null pointer is legal */
        return 3;
    it.N = 501;
    if (cavmd_field_recorder_item_check(&it) != CAVMD_ERR_INVALID_VALUE) /* N > 0 needs positions */
        return 4;
    it.d_position = (const double*)(uintptr_t)0x1000;
    if (cavmd_field_recorder_item_check(&it) != CAVMD_OK)
        return 5;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1;
    if (cavmd_field_recorder_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 6;
    it.N = 501;
    if (cavmd_field_recorder_create(NULL, 1, &it, 1, k, 8, 1, 1, 0, &r) != CAVMD_ERR_INVALID_VALUE || r != NULL)
        return 7;
    if (cavmd_field_recorder_destroy(NULL) != CAVMD_OK || cavmd_field_recorder_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_record(NULL, NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_rows(NULL, NULL, &rows) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_read(NULL, NULL, 0, 1, 0, 1, &rec) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_read_fields(NULL, NULL, 0, NULL, NULL, NULL, &n_refs) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_field_recorder_device_ptr(NULL, &dr, &drows) != CAVMD_ERR_INVALID_VALUE)
        return 8;
    {
        cavmd_workspace* ws = NULL;
        const int st = cavmd_create(-1, 1, &ws);
        if (st == CAVMD_ERR_NO_DEVICE)
            printf("no device: no workspace, hence no field recorder\n");
        else if (st == CAVMD_OK)
            cavmd_destroy(ws);
        else
            return 9;
    }
    printf("FIELD-RECORDER-ABI-OK\n");
    return 0;
}
