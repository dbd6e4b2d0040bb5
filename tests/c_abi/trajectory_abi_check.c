/* trajectory_abi_check.c -- the trajectory part of include/cavmd.h consumed as plain C99 (tests/batch_objects.py builds it
 * with -pedantic -Werror and runs it).  Needs no GPU: it prints the layouts of cavmd_trajectory_item, cavmd_trajectory_header
 * and struct cavmd_trajectory_layout for the test to compare with the ctypes structures, and checks the layout function, the
 * per-item validation (host arithmetic), the refusals of cavmd_trajectory_create's scalar arguments and that every entry point
 * refuses null arguments. */
#include <math.h>
#include <string.h>

#include "abi_print.h"
#include "cavmd.h"

#define OFF(which, type, field) ABI_OFF(which, type, field)

static uint64_t pad16(uint64_t x)
{
    return (x + 15u) / 16u * 16u;
}

int main(void)
{
    cavmd_trajectory_item it;
    cavmd_trajectory* t = NULL;
    struct cavmd_trajectory_layout lay;
    const void* series = NULL;
    const uint64_t* drows = NULL;
    uint64_t rows = 0;
    unsigned char frame[64];
    static const uint32_t sizes[] = {1, 2, 3, 4, 5, 255, 256, 257, 501, 65536};
    unsigned k, f;
    ABI_SIZE(item, cavmd_trajectory_item);
    ABI_SIZE(header, cavmd_trajectory_header);
    ABI_SIZE(layout, struct cavmd_trajectory_layout);
    OFF(item, cavmd_trajectory_item, d_pos);
    OFF(item, cavmd_trajectory_item, d_image);
    OFF(item, cavmd_trajectory_item, d_vel);
    OFF(item, cavmd_trajectory_item, d_time);
    OFF(item, cavmd_trajectory_item, Lx);
    OFF(item, cavmd_trajectory_item, Ly);
    OFF(item, cavmd_trajectory_item, Lz);
    OFF(item, cavmd_trajectory_item, N);
    OFF(item, cavmd_trajectory_item, reserved0);
    OFF(header, cavmd_trajectory_header, call);
    OFF(header, cavmd_trajectory_header, row);
    OFF(header, cavmd_trajectory_header, time);
    OFF(header, cavmd_trajectory_header, N);
    OFF(header, cavmd_trajectory_header, flags);
    OFF(header, cavmd_trajectory_header, box);
    OFF(header, cavmd_trajectory_header, reserved);
    OFF(layout, struct cavmd_trajectory_layout, frame_bytes);
    OFF(layout, struct cavmd_trajectory_layout, position_offset);
    OFF(layout, struct cavmd_trajectory_layout, velocity_offset);
    OFF(layout, struct cavmd_trajectory_layout, image_offset);
    OFF(layout, struct cavmd_trajectory_layout, max_N);
    OFF(layout, struct cavmd_trajectory_layout, format);
    OFF(layout, struct cavmd_trajectory_layout, element_bytes);
    OFF(layout, struct cavmd_trajectory_layout, reserved);
    if (cavmd_version() != CAVMD_VERSION_MAJOR * 1000 + CAVMD_VERSION_MINOR || CAVMD_VERSION_MINOR != 2)
        return 3;
    if (CAVMD_TRAJECTORY_F64 != 0 || CAVMD_TRAJECTORY_F32 != 1 || CAVMD_TRAJECTORY_MAX_BYTES != ((uint64_t)1 << 32))
        return 4;
    /* the layout function against the header's formulas */
    for (f = 0; f < 2; ++f)
        for (k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k)
        {
            const uint64_t e = f == CAVMD_TRAJECTORY_F64 ? 8 : 4, n = sizes[k];
            memset(&lay, 0xff, sizeof(lay));
            if (cavmd_trajectory_layout(sizes[k], f, &lay) != CAVMD_OK)
                return 5;
            if (lay.position_offset != 64 || lay.velocity_offset != 64 + pad16(3 * n * e)
                || lay.image_offset != lay.velocity_offset + pad16(3 * n * e) || lay.frame_bytes != lay.image_offset + pad16(12 * n)
                || lay.max_N != sizes[k] || lay.format != f || lay.element_bytes != e || lay.reserved != 0)
                return 6;
        }
    if (cavmd_trajectory_layout(0, 0, &lay) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_layout(CAVMD_BATCH_MAX_ITEM_N + 1u, 0, &lay) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_layout(501, 2, &lay) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_layout(501, 0, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 7;
    /* the item check */
    memset(&it, 0, sizeof(it));
    if (cavmd_trajectory_item_check(NULL) != CAVMD_ERR_INVALID_VALUE)
        return 8;
    if (cavmd_trajectory_item_check(&it) != CAVMD_OK) /* N == 0: nothing is required */
        return 9;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1000;
    it.d_image = (const cavmd_int3*)(uintptr_t)0x2004;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x3000;
    it.d_time = (const double*)(uintptr_t)0x4008;
    it.Lx = 10.0;
    it.Ly = 11.0;
    it.Lz = 12.0;
    it.N = 501;
    if (cavmd_trajectory_item_check(&it) != CAVMD_OK)
        return 10;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1008;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 11;
    it.d_pos = NULL;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 12;
    it.d_pos = (const cavmd_double4*)(uintptr_t)0x1000;
    it.d_image = (const cavmd_int3*)(uintptr_t)0x2002;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 13;
    it.d_image = NULL;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 14;
    it.d_image = (const cavmd_int3*)(uintptr_t)0x2004;
    it.d_vel = (const cavmd_double4*)(uintptr_t)0x3008;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 15;
    it.d_vel = NULL; /* no velocities: fine */
    it.d_time = (const double*)(uintptr_t)0x4004;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 16;
    it.d_time = NULL; /* no clock: fine */
    if (cavmd_trajectory_item_check(&it) != CAVMD_OK)
        return 17;
    it.Ly = 0.0;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 18;
    it.Ly = HUGE_VAL;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 19;
    it.Ly = 11.0;
    it.N = CAVMD_BATCH_MAX_ITEM_N + 1u;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_CAPACITY)
        return 20;
    it.N = CAVMD_BATCH_MAX_ITEM_N;
    if (cavmd_trajectory_item_check(&it) != CAVMD_OK)
        return 21;
    it.reserved0 = 1;
    if (cavmd_trajectory_item_check(&it) != CAVMD_ERR_INVALID_VALUE)
        return 22;
    it.reserved0 = 0;
    it.N = 501;
    /* null handles are refused before anything else */
    if (cavmd_trajectory_create(NULL, 1, &it, 501, 1, 8, 1, 0.0, &t) != CAVMD_ERR_INVALID_VALUE || t != NULL)
        return 23;
    if (cavmd_trajectory_create(NULL, 1, &it, 501, 1, 8, 1, 0.0, NULL) != CAVMD_ERR_INVALID_VALUE)
        return 24;
    if (cavmd_trajectory_destroy(NULL) != CAVMD_OK)
        return 25;
    if (cavmd_trajectory_set_items(NULL, 0, 1, &it) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_record(NULL, NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_rows(NULL, NULL, &rows) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_read(NULL, NULL, 0, 1, 0, 1, frame) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_reset(NULL, NULL) != CAVMD_ERR_INVALID_VALUE
        || cavmd_trajectory_device_ptr(NULL, &series, &drows) != CAVMD_ERR_INVALID_VALUE)
        return 26;
    {
        cavmd_workspace* ws = NULL;
        const int s = cavmd_create(-1, 1000, &ws);
        if (s == CAVMD_OK)
        {
            cavmd_trajectory_layout(501, 1, &lay);
            if (cavmd_trajectory_create(ws, 0, &it, 501, 1, 8, 1, 0.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 0, 1, 0.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 8, 0, 0.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 0, 1, 8, 1, 0.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 2, 8, 1, 0.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 8, 1, -1.0, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 8, 1, HUGE_VAL, &t) != CAVMD_ERR_INVALID_VALUE
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 8, 2, 1.0, &t) != CAVMD_ERR_INVALID_VALUE /* time rule, period 2 */
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, 8, 1, 1.0, &t) != CAVMD_ERR_INVALID_VALUE /* time rule, no d_time */
                || cavmd_trajectory_create(ws, 1, &it, 500, 1, 8, 1, 0.0, &t) != CAVMD_ERR_CAPACITY      /* N > max_N */
                || cavmd_trajectory_create(ws, 1, &it, 501, 1, (size_t)(CAVMD_TRAJECTORY_MAX_BYTES / lay.frame_bytes) + 1, 1, 0.0, &t)
                       != CAVMD_ERR_CAPACITY
                || t != NULL)
                return 27;
            printf("device present\n");
            cavmd_destroy(ws);
        }
        else if (s == CAVMD_ERR_NO_DEVICE && ws == NULL)
            printf("no device: no workspace, hence no trajectory object\n");
        else
            return 28;
    }
    printf("TRAJECTORY-ABI-OK\n");
    return 0;
}
