// cavmd_tile_schedule.hpp -- which particle rows a block of the dipole reduction loads, and in which order.  Plain C++ (no HIP
// header), so that the host can enumerate the very schedule the kernels run (tests/rolling_schedule_host.cpp).
//
// A tile is BLOCK * UNROLL particles; row u of a tile is its particles u * BLOCK .. (u + 1) * BLOCK - 1, one per lane.  A block
// owns the `nfull` full tiles at first, first + step, ...  The ROLLING loop (UNROLL >= 2) keeps UNROLL rows in flight per lane
// from its first tile to its last: it waits for row (k, u) only, issues row (k + 1, u) at once -- the later rows of tile k stay
// in flight meanwhile -- and then does the arithmetic of (k, u).  A lane therefore never has more than UNROLL rows outstanding
// (what the plain loop has right after tile_load), and never none while tiles are left: the ~57 VALU operations per particle run
// under the block's own loads at CONSTANT bytes in flight.  Nothing is issued past the last tile: the loop's steady part runs
// only while a next tile exists, and the last tile is drained by code that holds no load at all (one predicate around the
// loads would do, but the compiler's wait counts are merged where paths join, and the path without the load turns every counted
// wait behind it into a full one).  Two register sets (tile k in set k & 1) so that no row is ever copied.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAVMD_HD __host__ __device__ __forceinline__
#else
#define CAVMD_HD inline
#endif

// Diagnostic hook (csrc/microbench_persistent.hip): per-block time stamps at numbered points; nothing in the product.  Point 8
// is here: the rows of the block's first tile have been issued.
#ifndef CAVMD_PSTAMP
#define CAVMD_PSTAMP(k)
#endif

namespace cavmd
{

// the full tiles of one block: first particle of tile k = first + k * step
struct TileSchedule
{
    size_t first, step;
    unsigned nfull;
};

// strided deal: tile t of the N / tile full tiles belongs to block t % G
CAVMD_HD TileSchedule strided_tiles(unsigned N, unsigned G, unsigned b, unsigned tile)
{
    const unsigned full_tiles = N / tile;
    TileSchedule s;
    s.first = (size_t)b * tile;
    s.step = (size_t)G * tile;
    s.nfull = full_tiles > b ? (full_tiles - b + G - 1) / G : 0;
    return s;
}

// first particle (lane 0's) of row u of the block's k-th tile; k < nfull
CAVMD_HD size_t tile_row_base(const TileSchedule& s, unsigned k, unsigned u, unsigned block)
{
    return s.first + (size_t)k * s.step + (size_t)u * block;
}

// The rolling loop's order of events.  issue(set, u, base): start the loads of a row into register set `set`; landed(set, u):
// wait for that row, and for nothing issued after it; consume(set, u, k, base): the row's arithmetic.  `set`, `u` are constants
// once the calls are inlined and the u loops unrolled.  first_issued(): once, when the rows of the block's first tile are on
// their way and none has been waited for (the single-launch kernel waits there for the kernel arguments it did not need so far).
template <int UNROLL, class Issue, class Landed, class Consume, class FirstIssued>
CAVMD_HD void rolling_rows(const TileSchedule& s, unsigned block, Issue&& issue, Landed&& landed, Consume&& consume,
                           FirstIssued&& first_issued)
{
    if (s.nfull == 0)
        return;
    // tile k from `set` while tile k + 1 goes into the other set (k + 1 < nfull)
    auto roll = [&](int set, unsigned k) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            landed(set, u);
            issue(1 - set, u, tile_row_base(s, k + 1, u, block));
            consume(set, u, k, tile_row_base(s, k, u, block));
        }
    };
    // the block's last tile: nothing left to issue
    auto drain = [&](int set, unsigned k) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
        {
            landed(set, u);
            consume(set, u, k, tile_row_base(s, k, u, block));
        }
    };
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
        issue(0, u, tile_row_base(s, 0, u, block));
    CAVMD_PSTAMP(8);
    first_issued();
    unsigned k = 0;
    for (; k + 2 < s.nfull; k += 2)
    {
        roll(0, k);
        roll(1, k + 1);
    }
    if (k + 2 == s.nfull)
    {
        roll(0, k);
        drain(1, k + 1);
    }
    else
        drain(0, k);
}
template <int UNROLL, class Issue, class Landed, class Consume>
CAVMD_HD void rolling_rows(const TileSchedule& s, unsigned block, Issue&& issue, Landed&& landed, Consume&& consume)
{
    rolling_rows<UNROLL>(s, block, issue, landed, consume, [] {});
}

} // namespace cavmd
