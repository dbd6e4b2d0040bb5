// Host-only, and no HIP include: the arithmetic of a snapshot blob (include/cavmd.h, "save and restore") and the check of one
// against the shape of the object it is to be loaded into.  A plain C++ program compiles this header with the host compiler
// (tests/snapshot_check_host.cpp does, under the sanitizers); the table layer (cavmd_item_table.hpp) builds bytes / save / load
// on it and cavmd_snapshot_check forwards to snapshot_check.
//
// A blob is a cavmd_snapshot_header followed by the object's device arrays as they are, in declared order, each section padded
// with zero bytes to a multiple of 16:
//   a state object (verlet, bath, draw, thermalize, bussi_batch)   the n_items states of record_bytes each
//   a series object (recorder, ledger, trajectory)                 n_counters x n_items counter words of 8 bytes, then the whole
//                                                                  ring of n_items x capacity x record_bytes bytes
//   a ledger under the run clock's time rule (word[0] = 1)         those two, then last_time (n_items doubles)
//   the field recorder                                             a series object's two, then d_ref_rows (n_items x
//                                                                  max_references words), d_now (n_items x n_k x 2 doubles) and
//                                                                  d_refs (n_items x max_references x n_k x 2 doubles)
//   the field recorder under the run clock's time rule             those five, then last_time and last_reference_time
//   (word[1] = max_references | kSnapshotFieldTimed)                (2 x n_items doubles)
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "cavmd.h"

namespace cavmd
{
constexpr size_t kSnapshotMaxSections = 6;
constexpr uint32_t kSnapshotFieldTimed = 0x10000u; // in word[1] of a field recorder's header, above max_references (<= 16)

inline uint64_t snapshot_pad16(uint64_t x)
{
    return (x + 15u) & ~(uint64_t)15u;
}

// the unpadded sizes of the sections that follow a header of this shape, in the blob's order; returns how many there are
// (0 for a kind that is none of the nine)
inline size_t snapshot_sections(const cavmd_snapshot_header& h, uint64_t sizes[kSnapshotMaxSections])
{
    const uint64_t n = h.n_items;
    switch (h.kind)
    {
    case CAVMD_SNAPSHOT_VERLET:
    case CAVMD_SNAPSHOT_BATH:
    case CAVMD_SNAPSHOT_DRAW:
    case CAVMD_SNAPSHOT_THERMALIZE:
    case CAVMD_SNAPSHOT_BUSSI_BATCH:
        sizes[0] = n * h.record_bytes;
        return 1;
    case CAVMD_SNAPSHOT_RECORDER:
    case CAVMD_SNAPSHOT_LEDGER:
    case CAVMD_SNAPSHOT_TRAJECTORY:
    case CAVMD_SNAPSHOT_FIELD_RECORDER:
        sizes[0] = sizeof(uint64_t) * h.n_counters * n;
        sizes[1] = n * h.capacity * h.record_bytes;
        if (h.kind == CAVMD_SNAPSHOT_LEDGER && h.word[0] != 0) // word[0] = 1: taken under the run clock's time rule
        {
            sizes[2] = sizeof(double) * n; // last_time
            return 3;
        }
        if (h.kind != CAVMD_SNAPSHOT_FIELD_RECORDER)
            return 2;
    {
        const uint64_t max_refs = h.word[1] & (kSnapshotFieldTimed - 1); // word[0] = n_k, word[1] = max_references (| timed)
        sizes[2] = sizeof(uint64_t) * n * max_refs;
        sizes[3] = sizeof(double) * 2 * n * h.word[0];
        sizes[4] = sizeof(double) * 2 * n * max_refs * h.word[0];
        if (!(h.word[1] & kSnapshotFieldTimed))
            return 5;
        sizes[5] = sizeof(double) * 2 * n; // taken under the run clock's time rule: last_time, last_reference_time
        return 6;
    }
    default:
        return 0;
    }
}

// The header of an object of this shape, `bytes` included.  Every create bounds the products: n_items <= 2^16, a ring by 2^32
// bytes, n_k <= 256 and max_references <= 16, so nothing here overflows 64 bits.
inline cavmd_snapshot_header snapshot_header_make(uint32_t kind, uint64_t n_items, uint64_t capacity, uint64_t record_bytes,
                                                  uint32_t n_counters, uint32_t word0, uint32_t word1)
{
    cavmd_snapshot_header h;
    memset(&h, 0, sizeof(h));
    h.magic = CAVMD_SNAPSHOT_MAGIC;
    h.version = CAVMD_SNAPSHOT_VERSION;
    h.kind = kind;
    h.n_items = (uint32_t)n_items;
    h.n_counters = n_counters;
    h.capacity = capacity;
    h.record_bytes = record_bytes;
    h.word[0] = word0;
    h.word[1] = word1;
    uint64_t sizes[kSnapshotMaxSections];
    const size_t count = snapshot_sections(h, sizes);
    h.bytes = sizeof(h);
    for (size_t k = 0; k < count; ++k)
        h.bytes += snapshot_pad16(sizes[k]);
    return h;
}

// cavmd_snapshot_check: reads the 64 header bytes of `blob` and nothing behind them
inline int snapshot_check(const void* blob, size_t bytes, const cavmd_snapshot_header* expected)
{
    if (!blob || !expected)
        return CAVMD_ERR_INVALID_VALUE;
    cavmd_snapshot_header h;
    if (bytes < sizeof(h))
        return CAVMD_ERR_INVALID_VALUE;
    memcpy(&h, blob, sizeof(h)); // a blob need not be aligned
    if (h.magic != CAVMD_SNAPSHOT_MAGIC || h.version != CAVMD_SNAPSHOT_VERSION)
        return CAVMD_ERR_INVALID_VALUE;
    if (h.kind != expected->kind || h.n_items != expected->n_items || h.n_counters != expected->n_counters
        || h.capacity != expected->capacity || h.record_bytes != expected->record_bytes || h.word[0] != expected->word[0]
        || h.word[1] != expected->word[1])
        return CAVMD_ERR_INVALID_VALUE;
    if (h.reserved[0] != 0 || h.reserved[1] != 0)
        return CAVMD_ERR_INVALID_VALUE;
    if (h.bytes != (uint64_t)bytes || h.bytes != expected->bytes)
        return CAVMD_ERR_INVALID_VALUE;
    return CAVMD_OK;
}
} // namespace cavmd
