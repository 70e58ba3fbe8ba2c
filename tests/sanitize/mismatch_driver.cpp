// Stand-alone driver for the host-only pieces of gk_lookup_mismatch
// (genome-kmers_amd/csrc/gkm_mismatch_host.h): the reverse complement of a query, its 2-bit word and
// 4-bit words, the chunk arithmetic and the hit-record sort and split, built with
// -fsanitize=address,undefined by tests/test_mismatch_host.py.  Every buffer is heap-allocated at its
// exact size so that a read or write past an end is caught.  Prints "ok" and exits 0 when every check
// holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_mismatch_host.h"

using namespace gkm::mismatch;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static std::string revcomp(const std::string &q) {
    std::vector<uint8_t> in(q.begin(), q.end()), out(q.size());
    reverse_complement(in.data(), (uint32_t)in.size(), out.data());
    return std::string(out.begin(), out.end());
}

static uint64_t enc2(const std::string &q) {
    std::vector<uint8_t> in(q.begin(), q.end());
    return encode2(in.data(), (uint32_t)in.size());
}

static void enc4(const std::string &q, uint64_t out[2]) {
    std::vector<uint8_t> in(q.begin(), q.end());
    encode4(in.data(), (uint32_t)in.size(), out);
}

// the expected 4-bit code, spelt out: '$' 0, then the alphabet in byte order
static uint32_t want_code4(char b) {
    const char *order = "ABCDGHKMNRSTVWY";
    const char *at = std::strchr(order, b);
    return (b != 0 && at) ? (uint32_t)(at - order) + 1 : 0;
}

int main() {
    // reverse complement: the reference's pairs, IUPAC letters included; an involution
    CHECK(revcomp("A") == "T" && revcomp("ACGT") == "ACGT" && revcomp("AACG") == "CGTT");
    CHECK(revcomp("ABCDGHKMNRSTVWY") == "RWBASYNKMDCHGVT");
    CHECK(revcomp("NNAC") == "GTNN" && revcomp("RYKM") == "KMRY" && revcomp("SWN") == "NWS");
    {
        uint32_t x = 99u;
        const char *alpha = "ABCDGHKMNRSTVWY";
        for (int trial = 0; trial < 500; ++trial) {
            x = x * 1664525u + 1013904223u;
            std::string q(1 + (x >> 8) % 32, 'A');
            for (char &ch : q) {
                x = x * 1664525u + 1013904223u;
                ch = alpha[(x >> 10) % 15];
            }
            CHECK(revcomp(revcomp(q)) == q);
        }
    }
    // 2-bit word: first base most significant, right-aligned, at qlen 1, 16, 17, 31, 32
    CHECK(enc2("A") == 0 && enc2("C") == 1 && enc2("G") == 2 && enc2("T") == 3);
    CHECK(enc2("ACGT") == 0x1Bull && enc2("TA") == 0xCull);
    for (uint32_t len : {1u, 16u, 17u, 31u, 32u}) {
        const std::string a(len, 'A'), t(len, 'T'), c(len, 'C');
        CHECK(enc2(a) == 0);
        CHECK(enc2(t) == (len == 32 ? ~0ull : (1ull << (2 * len)) - 1));  // the all-T 32-mer is 2^64 - 1
        CHECK(enc2(c) == (len == 32 ? ~0ull : (1ull << (2 * len)) - 1) / 3);
        std::string g = a;
        g[0] = 'G';  // the first base lands in the top pair of the prefix
        CHECK(enc2(g) == 2ull << (2 * (len - 1)));
        g = a;
        g[len - 1] = 'G';
        CHECK(enc2(g) == 2ull);
        // the distance formula of the key path: popcount((x | x >> 1) & 0x5555...) counts bases
        const uint64_t x = enc2(a) ^ enc2(t);
        CHECK((uint32_t)__builtin_popcountll((x | (x >> 1)) & 0x5555555555555555ull) == len);
    }
    // 4-bit words: symbol t in nibble t % 16 of word t / 16, zero from qlen on
    for (uint32_t len : {1u, 15u, 16u, 17u, 31u, 32u}) {
        std::string q(len, 'A');
        const char *alpha = "ABCDGHKMNRSTVWY";
        for (uint32_t t = 0; t < len; ++t) q[t] = alpha[(t * 7 + len) % 15];
        uint64_t w[2];
        enc4(q, w);
        for (uint32_t t = 0; t < 32; ++t) {
            const uint32_t nib = (uint32_t)(w[t >> 4] >> (4 * (t & 15))) & 15u;
            CHECK(nib == (t < len ? want_code4(q[t]) : 0u));
        }
        enc4(std::string(len, 'Y'), w);  // code 15 everywhere: every nibble of the prefix set
        const uint32_t n0 = len < 16 ? len : 16, n1 = len - n0;
        CHECK(w[0] == (n0 == 16 ? ~0ull : (1ull << (4 * n0)) - 1));
        CHECK(w[1] == (n1 == 16 ? ~0ull : (1ull << (4 * n1)) - 1));
    }
    for (int b = 0; b < 256; ++b) CHECK(code4((uint8_t)b) == want_code4((char)b));
    CHECK(code4('$') == 0 && code4('A') == 1 && code4('N') == 9 && code4('Y') == 15);
    // chunk arithmetic: the knob only lowers the chunk; the chunks tile [0, m)
    {
        CHECK(chunk_size(nullptr) == kChunk && chunk_size("") == kChunk && chunk_size("0") == kChunk);
        CHECK(chunk_size("abc") == kChunk && chunk_size("12x") == kChunk && chunk_size("7") == 7);
        CHECK(chunk_size("65536") == kChunk && chunk_size("65537") == kChunk && chunk_size("65535") == 65535);
        CHECK(chunk_size("18446744073709551615") == kChunk);
        const uint64_t ms[] = {1, 2, 15, 16, 17, 1000, kChunk, kChunk + 1, 1ull << 32};
        const uint64_t cs[] = {1, 7, 16, kChunk};
        for (uint64_t m : ms)
            for (uint64_t c : cs) {
                const uint64_t n = chunk_count(m, c);
                CHECK(n >= 1 && (n - 1) <= m / c);
                if (n > 100000) continue;
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
    // hit records: ascending (query, kmer_num, strand), ties on (query, kmer_num) by strand
    {
        const HitRecord in[] = {
            {7, 2, 1, 1}, {7, 2, 0, 0}, {1ull << 33, 0, 3, 0}, {5, 0, 2, 1}, {5, 0, 1, 0},
            {0, 0xFFFFFFFFu, 0, 1}, {0, 0xFFFFFFFFu, 4, 0}, {6, 2, 2, 0}, {5, 1, 0, 1},
        };
        const uint64_t n = sizeof in / sizeof in[0];
        std::vector<HitRecord> rec(in, in + n);
        std::vector<uint32_t> q(n);
        std::vector<uint64_t> num(n);
        std::vector<uint8_t> mm(n), st(n);
        sort_and_split(rec.data(), n, q.data(), num.data(), mm.data(), st.data());
        const uint32_t want_q[] = {0, 0, 0, 1, 2, 2, 2, 0xFFFFFFFFu, 0xFFFFFFFFu};
        const uint64_t want_num[] = {5, 5, 1ull << 33, 5, 6, 7, 7, 0, 0};
        const uint8_t want_mm[] = {1, 2, 3, 0, 2, 0, 1, 4, 0}, want_st[] = {0, 1, 0, 1, 0, 0, 1, 0, 1};
        for (uint64_t i = 0; i < n; ++i)
            CHECK(q[i] == want_q[i] && num[i] == want_num[i] && mm[i] == want_mm[i] && st[i] == want_st[i]);
        // nothing to sort: no array is touched (null pointers)
        sort_and_split(nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    }
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}
