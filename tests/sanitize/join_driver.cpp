// Stand-alone driver for the index arithmetic of gk_join's key path
// (genome-kmers_amd/csrc/gkm_join_host.h): the merge-path diagonal search, the tile count and the
// bounds the tile kernels search their staged slices with, built with -fsanitize=address,undefined by
// tests/test_join_host.py.  Every list is a heap buffer of its exact size, so a read before a list or
// past its end is caught.  Each split is checked against a naive merge; the tiles between consecutive
// splits must cover both lists exactly once; and the tile kernel's lookup is replayed on the host over
// exactly the slice it stages (B's slice plus one element), against a search of the whole list.
// Prints "ok" and exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gkm_join_host.h"

using namespace gkm::join;

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

// n strictly ascending values drawn from [0, range) (range >= n), plus the extremes if asked
static std::vector<uint64_t> ascending(size_t n, uint64_t range, bool extremes = false) {
    std::vector<uint64_t> v;
    while (v.size() < n) {
        v.push_back(range == UINT64_MAX ? rnd() : rnd() % range);
        if (v.size() == n) {
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        }
    }
    if (extremes && n >= 2) {
        v.front() = 0;
        v.back() = UINT64_MAX;
    }
    return v;
}

// a list in the kernels' form: every key repeated 1..3 times, heads = the first index of each run
static void with_heads(const std::vector<uint64_t> &u, std::vector<uint64_t> *keys, std::vector<uint32_t> *heads) {
    keys->clear();
    heads->clear();
    for (uint64_t x : u) {
        heads->push_back((uint32_t)keys->size());
        for (uint64_t r = 1 + rnd() % 3; r > 0; --r) keys->push_back(x);
    }
}

// ia[d] = the number of A elements among the first d of the merged order, A first on a tie
static std::vector<uint64_t> naive_splits(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    std::vector<uint64_t> ia(a.size() + b.size() + 1);
    size_t i = 0, j = 0;
    for (size_t d = 0; d <= a.size() + b.size(); ++d) {
        ia[d] = i;
        if (i < a.size() && (j == b.size() || a[i] <= b[j])) ++i;
        else ++j;
    }
    return ia;
}

static void check_pair(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    const uint64_t na = a.size(), nb = b.size();
    const uint64_t *pa = na ? a.data() : nullptr, *pb = nb ? b.data() : nullptr;
    std::vector<uint64_t> ka, kb;
    std::vector<uint32_t> ha, hb;
    with_heads(a, &ka, &ha);
    with_heads(b, &kb, &hb);
    // every diagonal, the keys as they stand and through group heads
    const std::vector<uint64_t> want = naive_splits(a, b);
    for (uint64_t d = 0; d <= na + nb; ++d) {
        CHECK(diagonal_split(pa, nullptr, na, pb, nullptr, nb, d) == want[d]);
        CHECK(diagonal_split(ka.data(), ha.data(), na, kb.data(), hb.data(), nb, d) == want[d]);
    }
    // the tiles: consecutive splits cover both lists exactly once
    const uint64_t tiles = tile_count(na, nb);
    CHECK(tiles * kTile >= na + nb && (tiles == 0 || (tiles - 1) * kTile < na + nb));
    std::vector<uint32_t> seen_a(na, 0), seen_b(nb, 0), first(na, 0), count(na, 0);
    uint64_t prev_i = 0, prev_j = 0;
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint64_t d0 = t * kTile, d1 = std::min<uint64_t>(d0 + kTile, na + nb);
        const uint64_t i0 = diagonal_split(pa, nullptr, na, pb, nullptr, nb, d0);
        const uint64_t i1 = diagonal_split(pa, nullptr, na, pb, nullptr, nb, d1);
        const uint64_t j0 = d0 - i0, j1 = d1 - i1;
        CHECK(i0 == prev_i && j0 == prev_j && i1 >= i0 && j1 >= j0 && i1 <= na && j1 <= nb);
        CHECK((i1 - i0) + (j1 - j0) == d1 - d0);
        prev_i = i1;
        prev_j = j1;
        for (uint64_t i = i0; i < i1; ++i) ++seen_a[i];
        for (uint64_t j = j0; j < j1; ++j) ++seen_b[j];
        // the tile kernel's lookup over a copy of exactly what it stages: B[j0, j1 + ext)
        const uint32_t bt = (uint32_t)(j1 - j0) + (j1 < nb ? 1u : 0u);
        CHECK(bt <= kTile + 1);
        std::vector<uint64_t> stage(b.begin() + j0, b.begin() + j0 + bt);
        for (uint64_t i = i0; i < i1; ++i) {
            const uint32_t r = lower_bound_u64(stage.data(), bt, a[i]);
            first[i] = r < bt ? (uint32_t)(j0 + r) : (uint32_t)nb;
            count[i] = r < bt && stage[r] == a[i];
        }
    }
    CHECK(prev_i == na && prev_j == nb);
    for (uint32_t s : seen_a) CHECK(s == 1);
    for (uint32_t s : seen_b) CHECK(s == 1);
    for (uint64_t i = 0; i < na; ++i) {
        const auto lb = std::lower_bound(b.begin(), b.end(), a[i]);
        CHECK(first[i] == (uint32_t)(lb - b.begin()));
        CHECK(count[i] == (uint32_t)(lb != b.end() && *lb == a[i]));
    }
}

// join_mask_kernel's group search: positions [0, n) cut into runs by ascending heads, heads[0] = 0
static void check_mask(const std::vector<uint32_t> &heads, uint64_t n, uint32_t tile) {
    const uint64_t nu = heads.size();
    std::vector<uint32_t> group(n, 0);
    for (uint64_t p0 = 0; p0 < n; p0 += tile) {
        const uint64_t p1 = std::min<uint64_t>(p0 + tile, n);
        const uint64_t u0 = upper_bound_u32<uint64_t>(heads.data(), nu, p0) - 1;
        const uint64_t u1 = upper_bound_u32<uint64_t>(heads.data(), nu, p1 - 1);
        CHECK(u1 > u0 && u1 - u0 <= (uint64_t)tile + 1);
        std::vector<uint32_t> stage(heads.begin() + u0, heads.begin() + u1);
        for (uint64_t p = p0; p < p1; ++p)
            group[p] = (uint32_t)(u0 + upper_bound_u32<uint32_t>(stage.data(), (uint32_t)stage.size(), p) - 1);
    }
    for (uint64_t u = 0; u < nu; ++u) {
        const uint64_t end = u + 1 < nu ? heads[u + 1] : n;
        for (uint64_t p = heads[u]; p < end; ++p) CHECK(group[p] == u);
    }
}

int main() {
    const std::vector<uint64_t> none;
    // empty sides, one element, the extremes as ordinary keys
    check_pair(none, none);
    check_pair(none, {5});
    check_pair({5}, none);
    check_pair({5}, {5});
    check_pair({5}, {6});
    check_pair({6}, {5});
    check_pair({0}, {0});
    check_pair({UINT64_MAX}, {UINT64_MAX});
    check_pair({0, UINT64_MAX}, {0, UINT64_MAX});
    check_pair({0}, {UINT64_MAX});
    check_pair({UINT64_MAX}, {0});
    check_pair({0, 1, UINT64_MAX - 1, UINT64_MAX}, {1, UINT64_MAX});
    check_pair(none, ascending(300, 1000));
    check_pair(ascending(300, 1000), none);
    // every diagonal of lists up to a few hundred elements: dense ranges (many ties), sparse ones
    for (int trial = 0; trial < 60; ++trial) {
        const size_t na = rnd() % 300, nb = rnd() % 300;
        const uint64_t range = trial % 3 == 0 ? 400 : trial % 3 == 1 ? 5000 : UINT64_MAX;
        check_pair(ascending(na, range), ascending(nb, range));
    }
    {  // equal lists; all of A below B and the reverse; interleaved; the extremes shared
        const std::vector<uint64_t> v = ascending(257, 100000);
        check_pair(v, v);
        std::vector<uint64_t> lo = ascending(200, 1000), hi = ascending(220, 1000);
        for (uint64_t &x : hi) x += 1000;
        check_pair(lo, hi);
        check_pair(hi, lo);
        hi.front() = lo.back();  // one tie where the lists meet
        check_pair(lo, hi);
        check_pair(hi, lo);
        check_pair(ascending(250, UINT64_MAX, true), ascending(199, UINT64_MAX, true));
        std::vector<uint64_t> even, odd;
        for (uint64_t i = 0; i < 200; ++i) (i & 1 ? odd : even).push_back(i);
        check_pair(even, odd);
        check_pair(odd, even);
    }
    {  // several tiles: ties that straddle the tile boundaries, skew, and disjoint ranges
        const std::vector<uint64_t> a = ascending(3 * kTile + 77, 4 * kTile, false);
        for (size_t cut = 0; cut <= 8; ++cut) {  // each cut shifts every later boundary by one element
            const std::vector<uint64_t> b(a.begin() + cut, a.end());
            check_pair(a, b);
            check_pair(b, a);
        }
        check_pair(ascending(2 * kTile + 5, UINT64_MAX, true), ascending(kTile - 3, UINT64_MAX, true));
        check_pair(ascending(4 * kTile, 5 * kTile), ascending(30, 5 * kTile));
        check_pair(ascending(30, 5 * kTile), ascending(4 * kTile, 5 * kTile));
        std::vector<uint64_t> lo = ascending(kTile + 10, 3 * kTile), hi = ascending(kTile + 900, 3 * kTile);
        for (uint64_t &x : hi) x += 3 * kTile;
        check_pair(lo, hi);
        check_pair(hi, lo);
    }
    // the mask's group search: single positions, one group over everything, a group larger than a tile
    check_mask({0}, 1, 8);
    check_mask({0}, 100, 8);
    check_mask({0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, 10, 4);
    check_mask({0, 3, 4, 40, 41, 63}, 64, 8);
    check_mask({0, 5000}, 5001, 2048);
    for (int trial = 0; trial < 40; ++trial) {
        const uint64_t n = 1 + rnd() % 700;
        std::vector<uint32_t> heads{0};
        for (uint64_t p = 1; p < n; ++p)
            if (rnd() % (1 + trial % 9) == 0) heads.push_back((uint32_t)p);
        check_mask(heads, n, trial % 2 ? 16 : 64);
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
