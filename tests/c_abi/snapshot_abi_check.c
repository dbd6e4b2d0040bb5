/* snapshot_abi_check.c -- the save-and-restore part of include/cavmd.h consumed as plain C99 (tests/test_snapshot_abi.py builds
 * it with -pedantic -Werror and runs it).  Needs no GPU: it prints the layout of cavmd_snapshot_header as "name offset" lines
 * for the test to compare with the ctypes structure and the numpy dtype, checks cavmd_snapshot_check on a header made by hand
 * and that all 27 object entry points refuse null arguments. */
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(field) ABI_OFF(header, cavmd_snapshot_header, field)

#define NULLS(object)                                                                                             \
    (cavmd_snapshot_##object##_bytes(NULL, &n) == CAVMD_ERR_INVALID_VALUE                                         \
     && cavmd_snapshot_##object##_save(NULL, NULL, blob, sizeof(blob)) == CAVMD_ERR_INVALID_VALUE                 \
     && cavmd_snapshot_##object##_save(NULL, NULL, NULL, sizeof(blob)) == CAVMD_ERR_INVALID_VALUE                 \
     && cavmd_snapshot_##object##_load(NULL, NULL, blob, sizeof(blob)) == CAVMD_ERR_INVALID_VALUE                 \
     && cavmd_snapshot_##object##_load(NULL, NULL, NULL, sizeof(blob)) == CAVMD_ERR_INVALID_VALUE)

int main(void)
{
    cavmd_snapshot_header h;
    unsigned char blob[64 + 32];
    size_t n = 7;
    ABI_SIZE(header, cavmd_snapshot_header);
    OFF(magic);
    OFF(version);
    OFF(kind);
    OFF(n_items);
    OFF(n_counters);
    OFF(capacity);
    OFF(record_bytes);
    OFF(word);
    OFF(bytes);
    OFF(reserved);
    /* a verlet blob of one item by hand: the header and one 32-byte state */
    memset(&h, 0, sizeof(h));
    h.magic = CAVMD_SNAPSHOT_MAGIC;
    h.version = CAVMD_SNAPSHOT_VERSION;
    h.kind = CAVMD_SNAPSHOT_VERLET;
    h.n_items = 1;
    h.record_bytes = sizeof(cavmd_verlet_state);
    h.bytes = sizeof(blob);
    memset(blob, 0, sizeof(blob));
    memcpy(blob, &h, sizeof(h));
    if (memcmp(blob, "CAVSNAP1", 8) != 0 && memcmp(blob, "1PANSVAC", 8) != 0)
        return 3;
    if (cavmd_snapshot_check(blob, sizeof(blob), &h) != CAVMD_OK)
        return 4;
    if (cavmd_snapshot_check(NULL, sizeof(blob), &h) != CAVMD_ERR_INVALID_VALUE
        || cavmd_snapshot_check(blob, sizeof(blob), NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_snapshot_check(blob, sizeof(blob) - 1, &h) != CAVMD_ERR_INVALID_VALUE
        || cavmd_snapshot_check(blob, 63, &h) != CAVMD_ERR_INVALID_VALUE)
        return 5;
    h.kind = CAVMD_SNAPSHOT_BATH;
    if (cavmd_snapshot_check(blob, sizeof(blob), &h) != CAVMD_ERR_INVALID_VALUE)
        return 6;
    if (!NULLS(verlet) || !NULLS(bath) || !NULLS(draw) || !NULLS(thermalize) || !NULLS(bussi_batch) || !NULLS(recorder)
        || !NULLS(ledger) || !NULLS(trajectory) || !NULLS(field_recorder))
        return 7;
    if (n != 7) /* a refused bytes call writes nothing */
        return 8;
    if (cavmd_snapshot_verlet_bytes(NULL, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 9;
    printf("SNAPSHOT-ABI-OK\n");
    return 0;
}
