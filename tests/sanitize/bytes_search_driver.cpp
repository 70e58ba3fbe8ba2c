// Stand-alone driver for the byte path's comparison and range search
// (genome-kmers_amd/csrc/gkm_bytes_search.h: bytes_cmp, bytes_range and the Sought adaptors of
// gk_lookup, gk_join and gk_screen), built with -fsanitize=address,undefined by
// tests/test_bytes_search_host.py.  An sba is a heap block that ends exactly at its last contig's '$',
// with no pad, the starts, queries and reads are heap blocks of their exact size, and the starts reach
// up to that '$': a read of a byte after the '$' that ends a contig is caught.  The starts are sorted
// by a brute-force comparison of materialised strings of 4-bit codes (cut after a '$', the canonical
// form on canonical orders); the expected first / count of a sought k-mer are the numbers of strings
// below it and equal to it.  Prints "ok" and exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gkm_bytes_search.h"

using namespace gkm;

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

static const char kAlpha[] = "ABCDGHKMNRSTVWY";
static uint8_t g_lut4[256];

// the complement on bytes, written out apart from kComp4
static char comp(char b) {
    static const char from[] = "ATCGRYKMBVDHSWN", to[] = "TAGCYRMKVBHDSWN";
    const char *at = std::strchr(from, b);
    return at && b ? to[at - from] : b;
}
static std::string revcomp(const std::string &w) {
    std::string r(w.rbegin(), w.rend());
    for (char &c : r) c = comp(c);
    return r;
}
static std::string random_word(size_t len, const char *letters) {
    std::string w(len, 'A');
    for (char &c : w) c = letters[rnd() % std::strlen(letters)];
    return w;
}
// the 4-bit codes of w, cut after the first code 0 ('$' or a byte outside the alphabet)
static std::string codes(const std::string &w) {
    std::string s;
    for (char c : w) {
        s.push_back((char)g_lut4[(uint8_t)c]);
        if (s.back() == 0) break;
    }
    return s;
}

using Block = std::unique_ptr<uint8_t[]>;
static Block heap(const std::string &s) {
    Block b(new uint8_t[s.size()]);
    std::memcpy(b.get(), s.data(), s.size());
    return b;
}

// the k-mers of an sba that are at least min_len long, sorted at sort_len
struct Index {
    Block sba;
    std::string text;  // the sba's bytes, for the brute-force side only
    std::unique_ptr<uint32_t[]> starts;
    uint64_t n = 0;
    bool canon = false;
    // the string the k-mer at start p compares as at length k
    std::string mat(uint32_t p, int k) const {
        const std::string w = text.substr(p, std::min<size_t>(k, text.find('$', p) + 1 - p));
        if (!canon) return codes(w);
        return std::min(codes(w), codes(revcomp(w)));  // (whole k-mers only)
    }
};
static Index make_index(const std::vector<std::string> &contigs, int sort_len, int min_len, bool canon) {
    Index ix;
    for (const std::string &c : contigs) ix.text += c + '$';
    ix.sba = heap(ix.text);
    ix.canon = canon;
    std::vector<uint32_t> st;
    for (size_t p = 0; p < ix.text.size(); ++p)
        if (ix.text[p] != '$' && ix.text.find('$', p) - p >= (size_t)min_len) st.push_back((uint32_t)p);
    std::stable_sort(st.begin(), st.end(),
                     [&](uint32_t a, uint32_t b) { return ix.mat(a, sort_len) < ix.mat(b, sort_len); });
    ix.n = st.size();
    ix.starts.reset(new uint32_t[st.size()]);
    std::copy(st.begin(), st.end(), ix.starts.get());
    return ix;
}

// the strings of an index at length k, and a search's answer against their brute-force counts
struct Expect {
    const Index &ix;
    int k;
    std::vector<std::string> mats;
    Expect(const Index &ix_, int k_) : ix(ix_), k(k_) {
        for (uint64_t i = 0; i < ix.n; ++i) mats.push_back(ix.mat(ix.starts[i], k));
        CHECK(std::is_sorted(mats.begin(), mats.end()));
    }
    void counts(const std::string &want, uint64_t *less, uint32_t *equal) const {
        *less = 0;
        *equal = 0;
        for (const std::string &m : mats) {
            *less += m < want;
            *equal += m == want;
        }
    }
    template <bool CANON, class Sought>
    void search(const Sought &sought, uint64_t less, uint32_t equal) const {
        uint64_t first = ~0ull;
        uint32_t count = ~0u;
        bytes_range<CANON>(ix.sba.get(), ix.starts.get(), ix.n, k, g_lut4, sought, &first, &count);
        CHECK(first == less && count == equal);
    }
    // every source of a sought k-mer w of letters: gk_lookup's LDS column and its bytes, the bytes
    // as a strand given forward, and the reverse complement's bytes given as the other strand
    template <bool CANON>
    void all_forms(const std::string &w) const {
        uint64_t less;
        uint32_t equal;
        counts(codes(w), &less, &equal);
        Block col(new uint8_t[(size_t)(k - 1) * 256 + 1]);
        for (int t = 0; t < k; ++t) col[(size_t)t * 256] = g_lut4[(uint8_t)w[t]];
        search<CANON>(SoughtLds{col.get()}, less, equal);
        const Block q = heap(w), r = heap(revcomp(w));
        search<CANON>(SoughtBytes{q.get(), g_lut4}, less, equal);
        search<CANON>(SoughtStrand{q.get(), g_lut4, k, false}, less, equal);
        search<CANON>(SoughtStrand{r.get(), g_lut4, k, true}, less, equal);
    }
    // gk_screen's form: the read's window in place, as it stands and as its other strand, with any bytes
    template <bool CANON>
    void window(const std::string &w) const {
        const Block q = heap(w);
        for (int rc = 0; rc < 2; ++rc) {
            std::string s(w);
            if (rc) {  // (a byte outside the alphabet is its own complement: code 0 either way)
                std::reverse(s.begin(), s.end());
                for (char &c : s) c = comp(c);
            }
            uint64_t less;
            uint32_t equal;
            counts(codes(s), &less, &equal);
            search<CANON>(SoughtStrand{q.get(), g_lut4, k, rc != 0}, less, equal);
        }
    }
};

static std::string canonical(const std::string &w) { return std::min(w, revcomp(w)); }

template <bool CANON>
static void check_index(const std::vector<std::string> &contigs, const std::vector<std::string> &other, int k) {
    // forward orders hold every k-mer, those cut short by a '$' too, sorted at 64 >= k: the searches
    // at k are gk_lookup's with a query below the sort length.  Canonical orders are whole k-mers.
    const Index ix = make_index(contigs, CANON ? k : 64, CANON ? k : 1, CANON);
    const Expect ex(ix, k);
    uint64_t whole = 0, palindromes = 0, short_ones = 0;
    for (uint64_t i = 0; i < ix.n; ++i) {
        const uint32_t p = ix.starts[i];
        const std::string w = ix.text.substr(p, k);
        if (w.find('$') != std::string::npos) {  // cut short: a window whose bad byte meets its '$'
            ++short_ones;
            std::string v = w.substr(0, w.find('$') + 1);
            v.back() = "$X"[i & 1];
            v.resize(k, 'C');
            ex.window<CANON>(v);
            continue;
        }
        ++whole;
        palindromes += w == revcomp(w);
        ex.all_forms<CANON>(CANON ? canonical(w) : w);  // every k-mer present
        std::string nb(w);                              // a neighbour one substitution away
        nb[i % k] = kAlpha[(std::strchr(kAlpha, nb[i % k]) - kAlpha + 1 + i % 14) % 15];
        ex.all_forms<CANON>(nb);
        if (i % 3 == 0) {  // as a window of a read: both strands, and one byte outside the alphabet
            ex.window<CANON>(w);
            const char bad[] = {'$', 'X', 'a', '\0', '\xff'};
            for (int at : {0, k / 2, k - 1}) {
                std::string v(w);
                v[at] = bad[(i / 3 + at) % 5];
                ex.window<CANON>(v);
            }
        }
    }
    CHECK(whole > 0 && palindromes > 0 && (CANON || k == 1 || short_ones > 0));  // (at 1 none is cut short)
    // below every k-mer and above every k-mer
    ex.all_forms<CANON>(std::string(k, 'A'));
    ex.all_forms<CANON>(std::string(k, 'Y'));
    // gk_join's form: the whole k-mers of a second sba, sought where they lie in it
    const Index a = make_index(other, k, k, CANON);
    const Index b = make_index(contigs, k, k, CANON);
    const Expect eb(b, k);
    uint32_t shared = 0;
    for (uint64_t i = 0; i < a.n; ++i) {
        const uint8_t *pa = a.sba.get() + a.starts[i];
        uint64_t less;
        uint32_t equal;
        eb.counts(a.mat(a.starts[i], k), &less, &equal);
        shared += equal != 0;
        eb.search<CANON>(SoughtStrand{pa, g_lut4, k, CANON && canon_is_rc<4>(pa, k, g_lut4)}, less, equal);
    }
    CHECK(a.n > 0 && shared > 0 && (k < 31 || shared < a.n));  // (at 1 and 2 every k-mer may be shared)
}

int main() {
    for (int b = 0; b < 256; ++b) g_lut4[b] = code4((uint32_t)b);
    for (int i = 0; i < 15; ++i) {  // the codes follow the byte order, '$' below every letter
        CHECK(g_lut4[(uint8_t)kAlpha[i]] == i + 1 && kAlpha[i] > '$' && (i == 0 || kAlpha[i] > kAlpha[i - 1]));
        CHECK(comp_sym<4>(i + 1) == g_lut4[(uint8_t)comp(kAlpha[i])]);
    }
    CHECK(g_lut4['$'] == 0 && comp_sym<4>(0) == 0);
    // palindromes of 64 and of 33 (a self-complementary letter in the middle): the windows about
    // their centres are palindromes of every tested length
    const std::string h32 = random_word(32, kAlpha), h16 = random_word(16, "ACGT");
    const std::string p64 = h32 + revcomp(h32), p33 = h16 + "N" + revcomp(h16);
    const std::string rep = random_word(70, "AC"), mixed = random_word(66, kAlpha);
    // the sba ends with a contig of one base: the last starts are within every k of the block's end
    const std::vector<std::string> contigs = {p64, "T", rep, p33, mixed.substr(0, 40), rep.substr(3, 64) + "G",
                                              random_word(5, "ACGT"), mixed, "A"};
    // a second sba: shares k-mers with the first on both strands, and holds others
    const std::vector<std::string> other = {revcomp(mixed), random_word(65, kAlpha), rep.substr(1, 66), "C",
                                            p33 + "A", p64.substr(0, 64)};
    for (int k : {1, 2, 31, 32, 33, 64}) {
        check_index<false>(contigs, other, k);
        check_index<true>(contigs, other, k);
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
