// Stand-alone driver for the host-only pieces of gk_lookup (genome-kmers_amd/csrc/gkm_lookup_host.h):
// query validation, the canonical form of a query and the chunk arithmetic, built with
// -fsanitize=address,undefined by tests/test_lookup_host.py.  Every buffer is heap-allocated at its
// exact size so that a read or write past an end is caught.  Prints "ok" and exits 0 when every check
// holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_lookup_host.h"

using namespace gkm::lookup;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static std::string canon_of(const std::string &q) {
    std::vector<uint8_t> in(q.begin(), q.end()), out(q.size());
    canonical_query(in.data(), (uint32_t)in.size(), out.data());
    return std::string(out.begin(), out.end());
}

static std::string revcomp(const std::string &q) {
    std::string r(q.size(), 'A');
    for (size_t i = 0; i < q.size(); ++i) r[i] = (char)complement((uint8_t)q[q.size() - 1 - i]);
    return r;
}

int main() {
    // validation: the first bad byte's flat index, the ACGT flag
    {
        const char *rows = "ACGTACGTNNRYACGT";  // 4 queries of 4
        std::vector<uint8_t> q(rows, rows + 16);
        bool acgt = true;
        CHECK(validate_queries(q.data(), 4, 4, &acgt) == -1 && !acgt);
        CHECK(validate_queries(q.data(), 2, 4, &acgt) == -1 && acgt);
        q[9] = 'a';
        CHECK(validate_queries(q.data(), 4, 4, &acgt) == 9 && !acgt);
        q[9] = '$';
        CHECK(validate_queries(q.data(), 4, 4, &acgt) == 9);
        q[9] = 'X';
        CHECK(validate_queries(q.data(), 4, 4, &acgt) == 9);
        q[9] = 0;
        CHECK(validate_queries(q.data(), 4, 4, &acgt) == 9);
        CHECK(validate_queries(q.data(), 0, 4, &acgt) == -1 && acgt);
        // blocks of every length around the vector width, a bad byte at every position
        for (size_t len = 0; len <= 100; ++len)
            for (size_t at = 0; at <= len; ++at) {
                std::vector<uint8_t> blk(len);
                for (size_t i = 0; i < len; ++i) blk[i] = (uint8_t) "ACGT"[(i * 7 + len) & 3];
                if (at < len) blk[at] = 'N';
                CHECK(block_is_acgt(blk.data(), len) == (at == len));
                CHECK(block_is_acgt_scalar(blk.data(), len) == (at == len));
                bool a = false;
                if (len) CHECK(validate_queries(blk.data(), 1, (uint32_t)len, &a) == -1 && a == (at == len));
            }
        for (int b = 0; b < 256; ++b) {
            const bool letter = b != '$' && std::strchr("ABCDGHKMNRSTVWY", b) != nullptr && b != 0;
            CHECK((query_class((uint8_t)b) != 0) == letter);
        }
    }
    // complement: an involution over the alphabet, the reference's pairs
    for (const char *p = "ABCDGHKMNRSTVWY"; *p; ++p) CHECK(complement(complement((uint8_t)*p)) == (uint8_t)*p);
    CHECK(complement('A') == 'T' && complement('C') == 'G' && complement('R') == 'Y' && complement('K') == 'M' &&
          complement('B') == 'V' && complement('D') == 'H' && complement('N') == 'N' && complement('S') == 'S' &&
          complement('W') == 'W');
    // canonical form: min(q, revcomp(q)); equal for a query and its reverse complement; palindromes
    {
        uint32_t x = 12345u;
        const char *alpha = "ABCDGHKMNRSTVWY";
        for (int trial = 0; trial < 2000; ++trial) {
            x = x * 1664525u + 1013904223u;
            const size_t len = 1 + (x >> 8) % 70;
            std::string q(len, 'A');
            for (size_t i = 0; i < len; ++i) {
                x = x * 1664525u + 1013904223u;
                q[i] = (trial & 1) ? "ACGT"[(x >> 10) & 3] : alpha[(x >> 10) % 15];
            }
            const std::string r = revcomp(q), want = r < q ? r : q;
            CHECK(canon_of(q) == want);
            CHECK(canon_of(r) == want);
        }
        CHECK(canon_of("ACGT") == "ACGT");  // reverse palindrome
        CHECK(canon_of("T") == "A");
        CHECK(canon_of("TTTT") == "AAAA");
    }
    // chunk arithmetic: the chunks tile [0, m) in order, all full but the last
    {
        CHECK(chunk_size(nullptr, 31) == kChunk && chunk_size("", 31) == kChunk && chunk_size("0", 31) == kChunk);
        CHECK(chunk_size("abc", 31) == kChunk && chunk_size("12x", 31) == kChunk && chunk_size("1500", 31) == 1500);
        CHECK(chunk_size(nullptr, 1) == kChunk && chunk_size(nullptr, 64) == kChunk && chunk_size(nullptr, 65) < kChunk);
        CHECK(chunk_size(nullptr, 1u << 20) == 64 && chunk_size(nullptr, 0xFFFFFFFFu) == 1);
        // the knob lowers the chunk, never raises it
        CHECK(chunk_size("5", 31) == 5 && chunk_size("5", 0xFFFFFFFFu) == 1 && chunk_size("99999999999", 31) == kChunk);
        CHECK(chunk_size("18446744073709551615", 1u << 20) == 64);
        const uint64_t ms[] = {1, 2, 999, 1000, 1001, 4000, (1ull << 20) + 1, ~0ull};
        const uint64_t cs[] = {1, 7, 1000, 1500, 1ull << 20, 1ull << 40, ~0ull};
        for (uint64_t m : ms)
            for (uint64_t c : cs) {
                const uint64_t n = chunk_count(m, c);
                CHECK(n >= 1 && (n - 1) <= m / c);
                if (n > 100000) continue;  // (covered by the closed form above)
                uint64_t next = 0;
                for (uint64_t i = 0; i < n; ++i) {
                    uint64_t off, len;
                    chunk_range(m, c, i, &off, &len);
                    CHECK(off == next && len >= 1 && len <= c && (i + 1 == n || len == c));
                    next = off + len;
                }
                CHECK(next == m);
            }
    }
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}
