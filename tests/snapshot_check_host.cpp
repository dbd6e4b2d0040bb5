// Stand-alone: the host-only half of save and restore (csrc/cavmd_snapshot.hpp) driven by a plain C++ program, built with
// AddressSanitizer and UBSan by tests/test_snapshot_host.py.  Every blob lives in a heap block of exactly its length, so a read
// behind it is caught.  For one shape of each of the nine kinds: the accepted blob; each header field altered, one at a time;
// every truncation from 0 to 64 bytes; `bytes` off by one in both directions; blobs of every length up to header + 64, with a
// header that claims that length and with one that claims the right length; the section arithmetic against sizes worked out
// by hand.  Prints "snapshot check ok: <cases>" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "cavmd_snapshot.hpp"

namespace
{
long cases = 0;

[[noreturn]] void fail(const char* what, unsigned kind, long detail)
{
    std::printf("FAILED: %s (kind %u, %ld)\n", what, kind, detail);
    std::exit(1);
}

// the status of a blob of exactly `length` bytes that begins with the first min(length, 64) bytes of `h`
int status(const cavmd_snapshot_header& h, size_t length, size_t claimed, const cavmd_snapshot_header& expected)
{
    std::unique_ptr<unsigned char[]> blob(new unsigned char[length ? length : 1]);
    std::memset(blob.get(), 0xA5, length ? length : 1);
    std::memcpy(blob.get(), &h, length < sizeof(h) ? length : sizeof(h));
    cases += 1;
    return cavmd::snapshot_check(blob.get(), claimed, &expected);
}

void one_kind(const cavmd_snapshot_header& good, uint64_t by_hand)
{
    const unsigned kind = good.kind;
    const size_t total = (size_t)good.bytes;
    if (good.bytes != by_hand)
        fail("bytes by hand", kind, (long)good.bytes);
    if (sizeof(good) != 64 || good.bytes % 16 != 0)
        fail("header size or padding", kind, (long)sizeof(good));
    if (status(good, total, total, good) != CAVMD_OK)
        fail("the accepted blob", kind, 0);
    // each field altered, one at a time, in the blob; then in what is expected
    for (int side = 0; side < 2; ++side)
        for (int field = 0; field < 12; ++field)
        {
            cavmd_snapshot_header h = good;
            switch (field)
            {
            case 0: h.magic ^= 1; break;
            case 1: h.version += 1; break;
            case 2: h.kind = h.kind % 9 + 1; break;
            case 3: h.n_items += 1; break;
            case 4: h.n_counters += 1; break;
            case 5: h.capacity += 1; break;
            case 6: h.record_bytes += 8; break;
            case 7: h.word[0] += 1; break;
            case 8: h.word[1] += 1; break;
            case 9: h.bytes += 16; break;
            case 10: h.reserved[0] = 1; break;
            case 11: h.reserved[1] = 0x80000000u; break;
            }
            const bool blob_side = side == 0;
            if (!blob_side && (field == 0 || field == 1 || field >= 10))
                continue; // magic, version and the reserved words are not taken from `expected`
            if (status(blob_side ? h : good, total, total, blob_side ? good : h) != CAVMD_ERR_INVALID_VALUE)
                fail("an altered field was accepted", kind, field * 2 + side);
        }
    // every truncation of the header, the claimed length truthful
    for (size_t length = 0; length <= 64; ++length)
        if (length != total && status(good, length, length, good) != CAVMD_ERR_INVALID_VALUE)
            fail("a truncated blob was accepted", kind, (long)length);
    // bytes off by one in both directions (the block is as long as claimed)
    if (status(good, total - 1, total - 1, good) != CAVMD_ERR_INVALID_VALUE || status(good, total + 1, total + 1, good) != CAVMD_ERR_INVALID_VALUE)
        fail("bytes off by one was accepted", kind, 0);
    // every length up to header + 64: with the right header, and with a header that claims this very length
    for (size_t length = 0; length <= sizeof(good) + 64; ++length)
    {
        if (length != total && status(good, length, length, good) != CAVMD_ERR_INVALID_VALUE)
            fail("a blob of another length was accepted", kind, (long)length);
        cavmd_snapshot_header h = good;
        h.bytes = length;
        if (length != total && status(h, length, length, good) != CAVMD_ERR_INVALID_VALUE)
            fail("a blob that claims another length was accepted", kind, (long)length);
    }
    cavmd_snapshot_header none = good;
    if (cavmd::snapshot_check(nullptr, total, &good) != CAVMD_ERR_INVALID_VALUE
        || cavmd::snapshot_check(&none, sizeof(none), nullptr) != CAVMD_ERR_INVALID_VALUE)
        fail("a null pointer was accepted", kind, 0);
    cases += 2;
}
} // namespace

int main()
{
    using cavmd::snapshot_header_make;
    // state objects: 64 + pad16(n x state)
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_VERLET, 3, 0, 32, 0, 0, 0), 64 + 96);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_BATH, 1, 0, 32, 0, 0, 0), 64 + 32);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_DRAW, 5, 0, 64, 0, 0x9E3779B9u, 0x7F4A7C15u), 64 + 320);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_THERMALIZE, 2, 0, 64, 0, 0, 0), 64 + 128);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_BUSSI_BATCH, 1, 0, 48, 0, 0, 0), 64 + 48);
    // series objects: 64 + pad16(8 x counters x n) + pad16(n x capacity x record)
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_RECORDER, 3, 8, 128, 4, 0, 0), 64 + 96 + 3072);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_LEDGER, 1, 2, 192, 4, 0, 0), 64 + 32 + 384);
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_TRAJECTORY, 3, 4, 64 + 2 * 48 + 32, 5, 2, 0), 64 + 128 + 3 * 4 * 192);
    // the field recorder: + pad16(8 n refs) + pad16(16 n n_k) + pad16(16 n refs n_k); n = 3, n_k = 5, refs = 3
    one_kind(snapshot_header_make(CAVMD_SNAPSHOT_FIELD_RECORDER, 3, 8, 160, 5, 5, 3), 64 + 128 + 3840 + 80 + 240 + 720);
    // a kind that is none of the nine has no sections, and no object expects it
    uint64_t sizes[cavmd::kSnapshotMaxSections];
    cavmd_snapshot_header odd = snapshot_header_make(77, 1, 0, 32, 0, 0, 0);
    if (cavmd::snapshot_sections(odd, sizes) != 0 || odd.bytes != 64)
        fail("an unknown kind has sections", 77, (long)odd.bytes);
    if (cavmd::snapshot_pad16(0) != 0 || cavmd::snapshot_pad16(1) != 16 || cavmd::snapshot_pad16(16) != 16 || cavmd::snapshot_pad16(17) != 32)
        fail("pad16", 0, 0);
    std::printf("snapshot check ok: %ld cases\n", cases);
    return 0;
}
