// Stand-alone driver for the plain-C++ pieces of gk_match (genome-kmers_amd/csrc/gkm_match_host.h): the
// neighbour comparison of both paths, the byte path's whole per-position routine, the packed maximum,
// the cap's range and the chunk arithmetic at an overlap of C - 1 (gkm_screen_host.h's with C in the
// place of K), built with -fsanitize=address,undefined by tests/test_match_host.py.  Every buffer is
// heap-allocated at its exact size so that a read or write past an end is caught.
//   match_driver self          the edge cases below; prints "ok"
//   match_driver bytes FILE    FILE: u64 sba_len, n, total, nseq, C; sba; u32 starts[n] (sorted order);
//                              read bytes[total]; u64 offsets[nseq + 1].  Prints "len first count" per
//                              byte of the batch, by match::bytes_match as the kernel calls it.
//   match_driver keys FILE     FILE: u64 K, n, total, nseq, C; u64 keys[n] ascending; read bytes; offsets.
//                              Prints the same, by the key path's steps: m and q as the kernel forms
//                              them, the insertion point, match::key_match_len, the prefix's range.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_match_host.h"

using namespace gkm;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> out;
    FILE *f = std::fopen(path, "rb");
    if (!f) return out;
    std::fseek(f, 0, SEEK_END);
    const long len = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)len);
    if (len && std::fread(out.data(), 1, (size_t)len, f) != (size_t)len) out.clear();
    std::fclose(f);
    return out;
}

static void fill_lut(uint8_t *lut4) {
    for (int b = 0; b < 256; ++b) lut4[b] = code4((uint32_t)b);
}

static int run_bytes(const char *path) {
    const std::vector<uint8_t> file = read_file(path);
    if (file.size() < 40) return 2;
    uint64_t h[5];
    std::memcpy(h, file.data(), 40);
    const uint64_t sba_len = h[0], n = h[1], total = h[2], nseq = h[3];
    const int C = (int)h[4];
    if (file.size() != 40 + sba_len + 4 * n + total + 8 * (nseq + 1)) return 2;
    const uint8_t *at = file.data() + 40;
    // the sba with the one '$' that is known to follow it on the device, at its exact size
    std::vector<uint8_t> sba(at, at + sba_len);
    sba.push_back('$');
    sba.shrink_to_fit();
    at += sba_len;
    std::vector<uint32_t> starts(n);
    if (n) std::memcpy(starts.data(), at, 4 * n);
    at += 4 * n;
    std::vector<uint8_t> reads(at, at + total);
    reads.shrink_to_fit();
    at += total;
    std::vector<uint64_t> offsets(nseq + 1);
    std::memcpy(offsets.data(), at, 8 * (nseq + 1));
    uint8_t *lut4 = new uint8_t[256];
    fill_lut(lut4);
    for (uint64_t j = 0; j < nseq; ++j)
        for (uint64_t p = offsets[j]; p < offsets[j + 1]; ++p) {
            const uint64_t room = offsets[j + 1] - p;
            const int m = room < (uint64_t)C ? (int)room : C;
            uint32_t len, count;
            uint64_t first;
            match::bytes_match(sba.data(), starts.data(), n, m, lut4, SoughtBytes{reads.data() + p, lut4}, &len, &first,
                               &count);
            std::printf("%u %llu %u\n", len, (unsigned long long)first, count);
        }
    delete[] lut4;
    return 0;
}

static int run_keys(const char *path) {
    const std::vector<uint8_t> file = read_file(path);
    if (file.size() < 40) return 2;
    uint64_t h[5];
    std::memcpy(h, file.data(), 40);
    const int K = (int)h[0], C = (int)h[4];
    const uint64_t n = h[1], total = h[2], nseq = h[3];
    if (file.size() != 40 + 8 * n + total + 8 * (nseq + 1) || K < 1 || K > 32 || C < 1 || C > K) return 2;
    const uint8_t *at = file.data() + 40;
    std::vector<uint64_t> keys(n);
    if (n) std::memcpy(keys.data(), at, 8 * n);
    at += 8 * n;
    std::vector<uint8_t> reads(at, at + total);
    reads.shrink_to_fit();
    at += total;
    std::vector<uint64_t> offsets(nseq + 1);
    std::memcpy(offsets.data(), at, 8 * (nseq + 1));
    for (uint64_t j = 0; j < nseq; ++j)
        for (uint64_t p = offsets[j]; p < offsets[j + 1]; ++p) {
            const uint64_t room = offsets[j + 1] - p;
            const int lim = room < (uint64_t)C ? (int)room : C;
            uint64_t key = 0;
            int m = 0;
            for (; m < lim; ++m) {  // the clean symbols from p on, as the kernel takes them from its LDS codes
                const uint32_t b = reads[p + m];
                if (!(b == 'A' || b == 'C' || b == 'G' || b == 'T')) break;
                key = (key << 2) | canon_code<2>(b, nullptr);
            }
            uint32_t len = 0, count = 0;
            uint64_t first = 0;
            if (m > 0) {
                const uint64_t q = key << (2 * (K - m));
                const uint64_t pos = (uint64_t)(std::lower_bound(keys.begin(), keys.end(), q) - keys.begin());
                const bool has_prev = pos > 0, has_next = pos < n;
                len = (uint32_t)match::key_match_len(q, m, has_prev ? keys[pos - 1] : 0, has_prev,
                                                     has_next ? keys[pos] : 0, has_next, K);
                if (len) {
                    const int shift = 2 * (K - (int)len);
                    const uint64_t prefix = q >> shift;
                    uint64_t lo = 0, hi = n;
                    while (lo < hi) {
                        const uint64_t mid = (lo + hi) >> 1;
                        if ((keys[mid] >> shift) < prefix) lo = mid + 1;
                        else hi = mid;
                    }
                    first = lo;
                    hi = n;
                    while (lo < hi) {
                        const uint64_t mid = (lo + hi) >> 1;
                        if ((keys[mid] >> shift) <= prefix) lo = mid + 1;
                        else hi = mid;
                    }
                    count = (uint32_t)(lo - first);
                }
            }
            std::printf("%u %llu %u\n", len, (unsigned long long)first, count);
        }
    return 0;
}

// the windows of all chunks at cap C partition the matches' starts: every position owned once, every
// match a chunk answers (up to C bytes, inside its read) inside the bytes the chunk holds
static void check_partition(const std::vector<uint64_t> &lens, uint32_t C, uint64_t chunk_value) {
    std::vector<uint64_t> offsets(lens.size() + 1, 0);
    for (size_t j = 0; j < lens.size(); ++j) offsets[j + 1] = offsets[j] + lens[j];
    const uint64_t total = offsets.back();
    const std::string value = std::to_string(chunk_value);
    const uint64_t chunk = match::chunk_bytes(value.c_str(), C);
    CHECK(chunk >= C && chunk == (chunk_value < C ? C : chunk_value));
    std::vector<int> owned(total, 0);
    const uint64_t n = screen::chunk_count(total, chunk, C);
    uint64_t next = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t start, nslots, nbytes;
        screen::chunk_range(total, chunk, C, i, &start, &nslots, &nbytes);
        CHECK(start == next && nslots >= 1 && nbytes >= nslots && nbytes <= chunk && start + nbytes <= total);
        for (uint64_t p = start; p < start + nslots; ++p) {
            ++owned[p];
            uint64_t seq, off;
            screen::locate(offsets.data(), lens.size(), p, &seq, &off);
            const uint64_t room = offsets[seq + 1] - p, m = room < C ? room : C;
            CHECK(p + m <= start + nbytes);
        }
        next = start + nslots;
    }
    CHECK(next == total);
    for (uint64_t p = 0; p < total; ++p) CHECK(owned[p] == 1);
}

static int run_self() {
    using match::key_common;
    using match::key_match_len;
    // key_common: words 0 and 2^64 - 1, K = 1, 31, 32
    CHECK(key_common(0, 0, 32) == 32 && key_common(~0ull, ~0ull, 32) == 32 && key_common(0, ~0ull, 32) == 0);
    CHECK(key_common(0, 1, 32) == 31 && key_common(0, 2, 32) == 31 && key_common(0, 4, 32) == 30);
    CHECK(key_common(~0ull, ~0ull - 1, 32) == 31 && key_common(~0ull, ~0ull >> 2, 32) == 0);
    CHECK(key_common(1ull << 63, 0, 32) == 0 && key_common(1ull << 61, 0, 32) == 1);
    CHECK(key_common(0, 1, 1) == 0 && key_common(2, 3, 1) == 0 && key_common(3, 3, 1) == 1);
    const uint64_t top31 = (1ull << 62) - 1;  // the all-T 31-mer
    CHECK(key_common(top31, top31, 31) == 31 && key_common(top31, 0, 31) == 0 && key_common(top31, top31 - 1, 31) == 30);
    CHECK(key_common(top31, top31 >> 2, 31) == 0 && key_common(1ull << 60, 0, 31) == 0 && key_common(1ull << 58, 0, 31) == 1);
    // key_match_len: m = 0, a missing neighbour on either side, both missing (an empty index), the cut at m
    CHECK(key_match_len(0, 0, 0, true, 0, true, 32) == 0);
    CHECK(key_match_len(~0ull, 32, 0, false, 0, false, 32) == 0);
    CHECK(key_match_len(~0ull, 32, ~0ull - 1, true, 0, false, 32) == 31);
    CHECK(key_match_len(0, 32, 0, false, 1, true, 32) == 31);
    CHECK(key_match_len(0, 32, 0, false, 0, true, 32) == 32);
    CHECK(key_match_len(~0ull, 32, 0, true, ~0ull, true, 32) == 32);
    CHECK(key_match_len(3ull << 62, 1, 3ull << 62, false, ~0ull, true, 32) == 1);   // "T" then zeros against all-T
    CHECK(key_match_len(0, 5, 0, false, 0, true, 32) == 5);                         // equal words: cut at m
    CHECK(key_match_len(1, 1, 0, true, 0, false, 1) == 0 && key_match_len(1, 1, 0, true, 1, true, 1) == 1);
    CHECK(key_match_len(top31, 31, top31 - 3, true, 0, false, 31) == 30);
    // the packed maximum: a longer match wins, then the earlier position; 0 is "nothing yet"
    using match::best_pack;
    CHECK(best_pack(5, 7) > best_pack(4, 0) && best_pack(5, 7) > best_pack(5, 8) && best_pack(1, 0xFFFFFFFFu) > 0);
    CHECK(match::best_len(best_pack(4096, 17)) == 4096 && match::best_pos(best_pack(4096, 17)) == 17);
    CHECK(match::best_pos(best_pack(1, 0xFFFFFFFFu)) == 0xFFFFFFFFu && match::best_len(0) == 0 && match::best_pos(0) == 0);
    // the cap
    CHECK(match::resolve_cap(31, 0) == 31 && match::resolve_cap(31, 1) == 1 && match::resolve_cap(31, 31) == 31 &&
          match::resolve_cap(31, 32) == 0);
    CHECK(match::resolve_cap(0, 0) == 0 && match::resolve_cap(0, 1) == 1 && match::resolve_cap(0, 4096) == 4096 &&
          match::resolve_cap(0, 4097) == 0 && match::resolve_cap(5000, 5000) == 5000);
    // the chunk knob: lowers the default, never raises it, never below one match
    CHECK(match::chunk_bytes(nullptr, 31) == match::kChunkBytes && match::chunk_bytes("0", 31) == match::kChunkBytes &&
          match::chunk_bytes("abc", 31) == match::kChunkBytes && match::chunk_bytes("99999999999", 31) == match::kChunkBytes);
    CHECK(match::chunk_bytes("1500", 31) == 1500 && match::chunk_bytes("5", 31) == 31 && match::chunk_bytes("1", 1) == 1 &&
          match::chunk_bytes("100", 4096) == 4096);
    CHECK(match::kChunkBytes / match::kMaxCap >= 1024);  // the overlap stays far below a chunk
    {
        const std::vector<std::vector<uint64_t>> batches = {
            {150, 150, 150, 150}, {0, 1, 30, 31, 32, 0, 0, 500, 3, 31, 31, 1, 0}, {1000}, {7}, {0, 0, 0},
            {64, 0, 64, 1, 64, 2, 64, 30, 64},
        };
        const uint32_t caps[] = {1, 2, 3, 12, 31, 32, 40, 200};
        for (const auto &lens : batches)
            for (uint32_t C : caps) {
                const uint64_t sizes[] = {C, C + 1ull, C + 2ull, 37, 41, 97, 127, 256, 599, 100000};
                for (uint64_t size : sizes) check_partition(lens, C, size);
            }
    }
    // bytes_match_len: a '$' on the index side at every offset, the last byte of the sba; no byte after
    // a '$' is read (the buffers end right after it)
    {
        uint8_t *lut4 = new uint8_t[256];
        fill_lut(lut4);
        const char *q = "ACGTNACGT";
        for (int cut = 0; cut <= 9; ++cut) {
            std::vector<uint8_t> sba(q, q + cut);
            sba.push_back('$');
            sba.shrink_to_fit();
            for (int m = 0; m <= 9; ++m)
                CHECK(match::bytes_match_len(sba.data(), lut4, SoughtBytes{(const uint8_t *)q, lut4}, m) == (cut < m ? cut : m));
        }
        // a difference before the '$', a byte outside the alphabet in the read (code 0: it ends the match)
        std::vector<uint8_t> sba = {'A', 'C', 'T', 'T', '$'};
        CHECK(match::bytes_match_len(sba.data(), lut4, SoughtBytes{(const uint8_t *)q, lut4}, 9) == 2);
        const uint8_t bad[] = {'A', 'C', 'x', 'T'};
        CHECK(match::bytes_match_len(sba.data(), lut4, SoughtBytes{bad, lut4}, 4) == 2);
        // an index of one k-mer that is the sba's last byte; an empty index
        std::vector<uint8_t> one = {'G', '$'};
        std::vector<uint32_t> starts = {0};
        uint32_t len, count;
        uint64_t first;
        const uint8_t g[] = {'G', 'G', 'A'};
        match::bytes_match(one.data(), starts.data(), 1, 3, lut4, SoughtBytes{g, lut4}, &len, &first, &count);
        CHECK(len == 1 && first == 0 && count == 1);
        match::bytes_match(one.data(), starts.data(), 1, 1, lut4, SoughtBytes{g + 2, lut4}, &len, &first, &count);
        CHECK(len == 0 && first == 0 && count == 0);
        match::bytes_match(one.data(), starts.data(), 0, 3, lut4, SoughtBytes{g, lut4}, &len, &first, &count);
        CHECK(len == 0 && first == 0 && count == 0);
        match::bytes_match(one.data(), starts.data(), 1, 0, lut4, SoughtBytes{g, lut4}, &len, &first, &count);
        CHECK(len == 0 && first == 0 && count == 0);
        delete[] lut4;
    }
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "self") == 0) return run_self();
    if (argc == 3 && std::strcmp(argv[1], "bytes") == 0) return run_bytes(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "keys") == 0) return run_keys(argv[2]);
    std::fprintf(stderr, "usage: match_driver self | bytes FILE | keys FILE\n");
    return 2;
}
