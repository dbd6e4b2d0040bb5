// Stand-alone check of the rolling tile loop's schedule (csrc/cavmd_tile_schedule.hpp), built and run by
// tests/test_rolling_schedule_host.py under AddressSanitizer and UBSan.  No GPU: rolling_rows is the very driver the kernels
// run, here with callbacks that record instead of loading.
//
// For every N in [1, 6000], G in {1, 5, 16, 17, 256} and every block b < G, with the strided deal, BLOCK = 256, UNROLL = 2:
//   - every index a lane loads is < N, lies in a full tile, and that tile belongs to block b (tile % G == b);
//   - every particle of the block's full tiles is loaded exactly once, and the blocks together load every full-tile particle
//     exactly once;
//   - per lane, rows are issued in (tile, u) ascending order, consumed in the same order, every row is waited for before it is
//     consumed and after it was issued, a row is issued into a register set only after that set's previous row u was consumed,
//     and no lane ever has more than UNROLL rows outstanding, nor none while rows are left to issue.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cavmd_tile_schedule.hpp"

namespace
{
constexpr unsigned BLOCK = 256;
constexpr int UNROLL = 2;
constexpr unsigned TILE = BLOCK * UNROLL;

struct Row
{
    size_t base;
    bool busy, waited;
};

[[noreturn]] void fail(const char* what, unsigned N, unsigned G, unsigned b)
{
    std::fprintf(stderr, "FAIL: %s (N = %u, G = %u, block %u)\n", what, N, G, b);
    std::exit(1);
}
} // namespace

int main()
{
    const unsigned grids[] = {1, 5, 16, 17, 256};
    unsigned long long rows_checked = 0;
    std::vector<unsigned char> loaded;
    for (unsigned G : grids)
        for (unsigned N = 1; N <= 6000; ++N)
        {
            const unsigned full_tiles = N / TILE;
            loaded.assign((size_t)full_tiles * TILE, 0);
            for (unsigned b = 0; b < G; ++b)
            {
                const cavmd::TileSchedule s = cavmd::strided_tiles(N, G, b, TILE);
                Row regs[2][UNROLL] = {};
                unsigned issued = 0, landed = 0, consumed = 0, outstanding = 0; // outstanding: issued, not yet waited for
                const unsigned total = s.nfull * UNROLL;
                cavmd::rolling_rows<UNROLL>(
                    s, BLOCK,
                    [&](int set, int u, size_t base) {
                        // order: the issued rows are (0,0), (0,1), (1,0), ... = (tile, u) ascending
                        const unsigned k = issued / UNROLL;
                        if (issued >= total || (int)(issued % UNROLL) != u || set != (int)(k & 1))
                            fail("row issued out of order or past the last tile", N, G, b);
                        if (base != s.first + (size_t)k * s.step + (size_t)u * BLOCK)
                            fail("row issued at a wrong address", N, G, b);
                        if (regs[set][u].busy)
                            fail("row issued into registers that still hold an unconsumed row", N, G, b);
                        for (unsigned lane = 0; lane < BLOCK; ++lane)
                        {
                            const size_t i = base + lane;
                            if (i >= N)
                                fail("index >= N", N, G, b);
                            if (i >= (size_t)full_tiles * TILE || (i / TILE) % G != b)
                                fail("index outside the block's full tiles", N, G, b);
                            if (loaded[i]++)
                                fail("particle loaded twice", N, G, b);
                        }
                        regs[set][u] = Row {base, true, false};
                        ++issued;
                        if (++outstanding > (unsigned)UNROLL)
                            fail("more than UNROLL rows outstanding", N, G, b);
                    },
                    [&](int set, int u) {
                        if (!regs[set][u].busy)
                            fail("wait for a row that was not issued", N, G, b);
                        // loads return in order: the wait must be for the oldest row in flight
                        if (regs[set][u].waited || regs[set][u].base != s.first + (size_t)(landed / UNROLL) * s.step
                                                                            + (size_t)(landed % UNROLL) * BLOCK)
                            fail("wait for a row that is not the oldest in flight", N, G, b);
                        regs[set][u].waited = true;
                        ++landed;
                        --outstanding;
                    },
                    [&](int set, int u, unsigned k, size_t base) {
                        if (consumed != k * UNROLL + (unsigned)u || set != (int)(k & 1))
                            fail("row consumed out of order", N, G, b);
                        if (!regs[set][u].busy || !regs[set][u].waited || regs[set][u].base != base)
                            fail("row consumed before it was issued and waited for", N, G, b);
                        // between its first and last row a lane is never without loads in flight: when this row's
                        // arithmetic starts, the rows after it are outstanding (all UNROLL - 1 of them while rows are left)
                        const unsigned left = total - consumed - 1;
                        if (outstanding != (left < (unsigned)UNROLL ? left : (unsigned)UNROLL))
                            fail("rows in flight during the arithmetic: not min(UNROLL, rows left)", N, G, b);
                        regs[set][u].busy = false;
                        ++consumed;
                        ++rows_checked;
                    });
                if (issued != total || consumed != total || outstanding != 0)
                    fail("not every row of the block was issued and consumed", N, G, b);
            }
            for (size_t i = 0; i < loaded.size(); ++i)
                if (loaded[i] != 1)
                    fail("a full-tile particle was not loaded exactly once", N, G, 0);
        }
    std::printf("rolling schedule ok: %llu rows\n", rows_checked);
    return 0;
}
