// Stand-alone driver for the host-only pieces of gk_screen (genome-kmers_amd/csrc/gkm_screen_host.h):
// offset validation, the chunk and overlap arithmetic, mapping a byte position back to (sequence,
// offset) and the knobs' values, built with -fsanitize=address,undefined by tests/test_screen_host.py.
// Every buffer is heap-allocated at its exact size so that a read or write past an end is caught.
// Prints "ok" and exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_screen_host.h"

using namespace gkm::screen;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

// For one batch (read lengths) and one chunk size: the windows of all chunks partition the windows of
// the batch, none twice and none missed; every position is owned exactly once; every window a chunk
// answers lies inside the bytes it holds; consecutive chunks overlap by K - 1 bytes.
static void check_partition(const std::vector<uint64_t> &lens, uint32_t K, uint64_t chunk_value) {
    std::vector<uint64_t> offsets(lens.size() + 1, 0);
    for (size_t j = 0; j < lens.size(); ++j) offsets[j + 1] = offsets[j] + lens[j];
    const uint64_t total = offsets.back();
    const std::string value = std::to_string(chunk_value);
    const uint64_t chunk = chunk_bytes(value.c_str(), K);
    CHECK(chunk >= K && chunk == (chunk_value < K ? K : chunk_value));
    std::vector<int> owned(total, 0), answered(total, 0);
    const uint64_t n = chunk_count(total, chunk, K);
    uint64_t next = 0, prev_end = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t start, nslots, nbytes;
        chunk_range(total, chunk, K, i, &start, &nslots, &nbytes);
        CHECK(start == next && nslots >= 1 && nbytes >= nslots && nbytes <= chunk && start + nbytes <= total);
        CHECK(i + 1 == n || nslots == chunk - (K - 1));
        CHECK(nbytes == (total - start < chunk ? total - start : chunk));
        // the overlap with the chunk before: K - 1 bytes (fewer only where the batch ends first)
        if (i > 0) CHECK(prev_end == (start + (K - 1) < total ? start + (K - 1) : total));
        prev_end = start + nbytes;
        for (uint64_t p = start; p < start + nslots; ++p) {
            ++owned[p];
            uint64_t seq, off;
            locate(offsets.data(), lens.size(), p, &seq, &off);
            CHECK(offsets[seq] <= p && p < offsets[seq + 1] && off == p - offsets[seq]);
            if (p + K <= offsets[seq + 1]) {  // a window starts here: its bytes are in the chunk
                ++answered[p];
                CHECK(p + K <= start + nbytes);
            }
        }
        next = start + nslots;
    }
    CHECK(next == total);
    uint64_t windows = 0, want = 0;
    for (uint64_t p = 0; p < total; ++p) {
        CHECK(owned[p] == 1 && answered[p] <= 1);
        windows += answered[p];
    }
    for (uint64_t len : lens) want += len >= K ? len - K + 1 : 0;
    CHECK(windows == want);
}

int main() {
    // offsets: start at 0, never decrease, no sequence over 2^32 - 1 bytes; the culprit's index
    {
        uint64_t at = 99;
        std::vector<uint64_t> ok = {0, 0, 5, 5, 9, 9};
        CHECK(validate_offsets(ok.data(), 5, &at) == kOffsetsOk);
        CHECK(validate_offsets(ok.data(), 0, &at) == kOffsetsOk);  // (reads offsets[0] only)
        std::vector<uint64_t> one = {0};
        CHECK(validate_offsets(one.data(), 0, &at) == kOffsetsOk);
        std::vector<uint64_t> late = {1, 5};
        CHECK(validate_offsets(late.data(), 1, &at) == kOffsetsStart && at == 0);
        std::vector<uint64_t> down = {0, 4, 9, 8, 12};
        CHECK(validate_offsets(down.data(), 4, &at) == kOffsetsDecrease && at == 2);
        std::vector<uint64_t> edge = {0, 3, 3 + 0xFFFFFFFFull};
        CHECK(validate_offsets(edge.data(), 2, &at) == kOffsetsOk);
        std::vector<uint64_t> big = {0, 3, 4 + 0xFFFFFFFFull, 5 + 0xFFFFFFFFull};
        CHECK(validate_offsets(big.data(), 3, &at) == kOffsetsLong && at == 1);
        std::vector<uint64_t> huge = {0, ~0ull};
        CHECK(validate_offsets(huge.data(), 1, &at) == kOffsetsLong && at == 0);
    }
    // the path knob's values
    CHECK(parse_path(nullptr) == 0 && parse_path("bytes") == 1 && parse_path("keys") == 2);
    CHECK(parse_path("") == -1 && parse_path("key") == -1 && parse_path("Bytes") == -1 && parse_path("keys ") == -1 &&
          parse_path("1") == -1);
    // the chunk knob: lowers the default, never raises it, never below one window
    CHECK(chunk_bytes(nullptr, 31) == kChunkBytes && chunk_bytes("", 31) == kChunkBytes &&
          chunk_bytes("0", 31) == kChunkBytes);
    CHECK(chunk_bytes("abc", 31) == kChunkBytes && chunk_bytes("12x", 31) == kChunkBytes &&
          chunk_bytes("-5", 31) == kChunkBytes);
    CHECK(chunk_bytes("1500", 31) == 1500 && chunk_bytes("31", 31) == 31 && chunk_bytes("5", 31) == 31 &&
          chunk_bytes("1", 1) == 1);
    CHECK(chunk_bytes("99999999999", 31) == kChunkBytes && chunk_bytes("18446744073709551615", 31) == kChunkBytes);
    CHECK(chunk_bytes(nullptr, 0xFFFFFFFFu) == 0xFFFFFFFFull && chunk_step(0xFFFFFFFFull, 0xFFFFFFFFu) == 1);
    CHECK(chunk_count(0, 100, 31) == 0 && chunk_count(1, 100, 31) == 1 && chunk_count(70, 100, 31) == 1 &&
          chunk_count(71, 100, 31) == 2 && chunk_count(~0ull, kChunkBytes, 31) >= 1);
    // the partition of the windows, for chunk sizes K, K + 1, a few primes and larger ones
    {
        const std::vector<std::vector<uint64_t>> batches = {
            {150, 150, 150, 150},
            {0, 1, 30, 31, 32, 0, 0, 500, 3, 31, 31, 1, 0},
            {1000},
            {7},
            {0, 0, 0},
            {31, 31, 31, 31, 31, 31, 31, 31},
            {64, 0, 64, 1, 64, 2, 64, 30, 64},
        };
        const uint32_t ks[] = {1, 2, 3, 11, 31, 32, 40};
        for (const auto &lens : batches)
            for (uint32_t K : ks) {
                const uint64_t sizes[] = {K, K + 1ull, K + 2ull, 37, 41, 53, 97, 101, 127, 256, 599, 1024, 100000};
                for (uint64_t size : sizes) check_partition(lens, K, size);
            }
    }
    // locate: empty sequences at a position are passed over; the first and last byte of a sequence
    {
        std::vector<uint64_t> offsets = {0, 0, 0, 4, 4, 10, 10};
        uint64_t seq, off;
        locate(offsets.data(), 6, 0, &seq, &off);
        CHECK(seq == 2 && off == 0);
        locate(offsets.data(), 6, 3, &seq, &off);
        CHECK(seq == 2 && off == 3);
        locate(offsets.data(), 6, 4, &seq, &off);
        CHECK(seq == 4 && off == 0);
        locate(offsets.data(), 6, 9, &seq, &off);
        CHECK(seq == 4 && off == 5);
    }
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}
