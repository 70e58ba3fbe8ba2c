// Stand-alone driver for the two comparisons behind gk_lcp (genome-kmers_amd/csrc/gkm_lcp_host.h):
// keys_lcp over encoded keys and bytes_lcp over sequence bytes, built with
// -fsanitize=address,undefined by tests/test_lcp_host.py.  Every buffer is a heap buffer of its exact
// size, so a read before it or past its end is caught; a count-leading-zeros of 0 is undefined
// behaviour, so equal keys that reached it would be caught too.  keys_lcp is checked against a naive
// symbol-by-symbol loop, bytes_lcp against the definition spelt out here.
// Prints "ok" and exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_lcp_host.h"

using namespace gkm::lcp;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

// the key of `symbols` codes of `bits` bits, right-aligned in W words, word 0 most significant
static std::vector<uint64_t> encode(const std::vector<uint8_t> &codes, int bits, int W) {
    std::vector<uint64_t> k(W, 0);
    const int symbols = (int)codes.size();
    for (int s = 0; s < symbols; ++s) {
        const int lo = (symbols - 1 - s) * bits;  // bit index of the symbol's bit 0 in the W-word integer
        k[W - 1 - lo / 64] |= (uint64_t)codes[s] << (lo % 64);
    }
    return k;
}

static uint32_t naive_keys_lcp(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, uint32_t cap) {
    uint32_t t = 0;
    while (t < a.size() && t < cap && a[t] == b[t]) ++t;
    return t;
}

template <int W>
static void check_keys(int bits) {
    const int max_symbols = 64 * W / bits;
    const int min_symbols = 64 * (W - 1) / bits + 1;  // the fewest symbols that need W words
    for (int symbols : {min_symbols, min_symbols + 1, (min_symbols + max_symbols) / 2, max_symbols - 1, max_symbols}) {
        if (symbols < min_symbols || symbols > max_symbols) continue;
        std::vector<uint8_t> a(symbols);
        for (auto &c : a) c = (uint8_t)(rnd() & ((1u << bits) - 1));
        const std::vector<uint64_t> ka = encode(a, bits, W);
        const uint32_t caps[] = {1, (uint32_t)symbols / 2 + 1, (uint32_t)std::max(1, symbols - 1),
                                 (uint32_t)symbols, (uint32_t)symbols + 1, 1u << 24};
        // equal keys: the cap or the symbol count, and no count-leading-zeros of 0
        for (uint32_t cap : caps) CHECK(keys_lcp<W>(ka.data(), ka.data(), bits, symbols, cap) == std::min<uint32_t>(symbols, cap));
        // a first difference at every symbol: every word, both ends of every word
        for (int d = 0; d < symbols; ++d) {
            for (int rep = 0; rep < 3; ++rep) {
                std::vector<uint8_t> b = a;
                b[d] ^= (uint8_t)(1 + rnd() % ((1u << bits) - 1));  // another code at d
                for (int s = d + 1; s < symbols; ++s)
                    if (rep) b[s] = (uint8_t)(rnd() & ((1u << bits) - 1));  // anything after it
                const std::vector<uint64_t> kb = encode(b, bits, W);
                for (uint32_t cap : caps) {
                    const uint32_t want = naive_keys_lcp(a, b, cap);
                    CHECK(want == std::min<uint32_t>(d, cap));
                    CHECK(keys_lcp<W>(ka.data(), kb.data(), bits, symbols, cap) == want);
                    CHECK(keys_lcp<W>(kb.data(), ka.data(), bits, symbols, cap) == want);
                }
            }
        }
    }
    // the extreme keys: all zeros against all ones differ at the first symbol
    const int symbols = max_symbols;
    std::vector<uint64_t> zeros(W, 0), ones(W, ~0ull);
    CHECK(keys_lcp<W>(zeros.data(), ones.data(), bits, symbols, symbols) == 0);
    CHECK(keys_lcp<W>(ones.data(), ones.data(), bits, symbols, symbols) == (uint32_t)symbols);
    CHECK(keys_lcp<W>(zeros.data(), zeros.data(), bits, symbols, 7) == 7);
    std::vector<uint64_t> last = ones;
    last[W - 1] ^= 1;  // the last symbol differs
    CHECK(keys_lcp<W>(ones.data(), last.data(), bits, symbols, symbols) == (uint32_t)symbols - 1);
}

// the definition: the largest k in 0..cap at which the windows compare equal at kmer_len = k
static bool equal_at(const std::string &s, size_t a, size_t b, uint32_t k) {
    for (uint32_t t = 0;; ++t) {
        const bool oa = s[a + t] == '$', ob = s[b + t] == '$';
        if (oa || ob) return oa && ob;
        if (s[a + t] != s[b + t]) return false;
        if (t == k - 1) return true;
    }
}
static uint32_t naive_bytes_lcp(const std::string &s, size_t a, size_t b, uint32_t cap) {
    uint32_t best = 0;
    for (uint32_t k = 1; k <= cap; ++k)
        if (equal_at(s, a, b, k)) best = k;
    return best;
}

static void check_bytes_case(const std::string &text, size_t a, size_t b, uint32_t cap, uint32_t want) {
    // the exact bytes on the heap, nothing after them: the text ends in '$' (the pad's role)
    std::vector<uint8_t> buf(text.begin(), text.end());
    CHECK(naive_bytes_lcp(text, a, b, cap) == want);
    CHECK(bytes_lcp(buf.data(), a, b, cap) == want);
    CHECK(bytes_lcp(buf.data(), b, a, cap) == want);
}

static void check_bytes() {
    check_bytes_case("ACGT$ACGA$", 0, 5, 10, 3);  // a differing base
    check_bytes_case("ACGT$ACGA$", 0, 5, 3, 3);   // ... at the cap
    check_bytes_case("ACGT$ACGA$", 0, 5, 2, 2);   // ... beyond the cap
    check_bytes_case("ACG$ACGT$", 0, 4, 10, 3);   // '$' on one side
    check_bytes_case("ACG$ACGT$", 0, 4, 3, 3);    // ... at the cap: not reached
    check_bytes_case("ACG$ACG$", 0, 4, 10, 10);   // '$' on both sides: equal at every length
    check_bytes_case("ACG$ACG$", 0, 4, 1 << 16, 1 << 16);
    check_bytes_case("ACG$ACG$", 0, 4, 3, 3);     // '$' on both sides at the cap
    check_bytes_case("$A$", 0, 2, 5, 5);          // '$' on both sides at offset 0
    check_bytes_case("$A$", 0, 1, 5, 0);          // '$' on one side at offset 0
    check_bytes_case("AAAA$", 0, 1, 8, 3);        // a window inside the other: its '$' ends the prefix
    check_bytes_case("AAAA$", 3, 3, 8, 8);        // a k-mer against itself
    check_bytes_case("AC$", 0, 1, 1, 0);          // cap 1
    check_bytes_case("AA$", 0, 1, 1, 1);
    // random texts over a small alphabet with '$' inside, every pair of starts of a few, several caps
    for (int round = 0; round < 40; ++round) {
        std::string text;
        const size_t len = 2 + rnd() % 40;
        for (size_t i = 0; i < len; ++i) text.push_back("AAC$"[rnd() % 4]);
        text.push_back('$');
        for (int pair = 0; pair < 30; ++pair) {
            const size_t a = rnd() % text.size(), b = rnd() % text.size();
            for (uint32_t cap : {1u, 2u, 5u, 64u}) check_bytes_case(text, a, b, cap, naive_bytes_lcp(text, a, b, cap));
        }
    }
}

int main() {
    check_keys<1>(2);
    check_keys<2>(2);
    check_keys<3>(2);
    check_keys<4>(2);
    check_keys<1>(4);
    check_keys<2>(4);
    check_keys<3>(4);
    check_keys<4>(4);
    check_bytes();
    CHECK(min_unique_of(0, 5) == 1);
    CHECK(min_unique_of(4, 5) == 5);
    CHECK(min_unique_of(5, 5) == kNeverUnique);
    CHECK(kTile == kThreads * kItems && kThreads % 64 == 0);
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}
